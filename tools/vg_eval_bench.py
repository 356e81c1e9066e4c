"""VG-CPT evaluation cost on one GPU: the Recall@K kernel (cpt_vg_recall_ranks + the float64 reductions) on a synthetic split the size of
VG150's test set against the host restatement of eval_vg (scoring.eval_vg_reference), and end-to-end drivers.val_vg pairs/s on
Oscar-base (random weights) at 16 pairs per step.

    python tools/vg_eval_bench.py [--images 26446] [--host-images 1000] [--pairs 320] [--dtype bf16]

The split: per image 2-62 boxes (geometric, mean about 12, as VG150's test images), every ordered pair a candidate, 51 score slots.
The host restatement runs on the first --host-images images and is scaled to the split by candidate count.  One JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpt_amd import config as cfgmod, drivers, scoring as S, synth          # noqa: E402
from cpt_amd.modeling_rec import REC_MLM_CPT                                   # noqa: E402


def split(n_img, seed=0, C=51):
    """CSR table (as scoring.vg_eval_table returns it) of a synthetic split, built without keys; scores (n, C) on the host."""
    rng = np.random.Generator(np.random.PCG64(seed))
    boxes = np.clip(rng.geometric(1 / 11.0, size=n_img) + 1, 2, 62)
    n = boxes * (boxes - 1)
    cand_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    cand = np.empty((int(n.sum()), 3), dtype=np.int32)
    gt_off, gt = [0], []
    for i, b in enumerate(boxes):
        s, o = np.nonzero(~np.eye(b, dtype=bool))
        lo = cand_off[i]
        cand[lo:lo + n[i], 0], cand[lo:lo + n[i], 1], cand[lo:lo + n[i], 2] = s, o, np.arange(lo, lo + n[i])
        ng = int(rng.integers(1, 2 + b // 2))
        j = rng.integers(0, n[i], size=ng)
        gt.append(np.stack([s[j], o[j], rng.integers(1, C, size=ng)], 1))
        gt_off.append(gt_off[-1] + ng)
    gt = np.concatenate(gt).astype(np.int32)
    table = {"cand_off": torch.from_numpy(cand_off), "cand": torch.from_numpy(cand), "gt_off": torch.tensor(gt_off, dtype=torch.int32),
             "gt": torch.from_numpy(gt), "gt_img": torch.from_numpy(np.repeat(np.arange(n_img), np.diff(gt_off))).long(),
             "images": ["%d.jpg" % i for i in range(n_img)], "n_rows": int(n.sum()), "n_slots": C}
    scores = torch.from_numpy(rng.standard_normal((int(n.sum()), C), dtype=np.float32))
    return table, scores


def host_restatement(table, scores, n_img):
    """eval_vg_reference on the first n_img images of the table (keys rebuilt from it)."""
    preds, gts = {}, []
    co, go = table["cand_off"].tolist(), table["gt_off"].tolist()
    for i in range(n_img):
        for s, o, r in table["cand"][co[i]:co[i + 1]].tolist():
            preds["%d.jpg_%d_%d" % (i, s, o)] = scores[r]
        gts.append({"img_path": "%d.jpg" % i, "relations": table["gt"][go[i]:go[i + 1]].numpy()})
    t = time.perf_counter()
    S.eval_vg_reference(preds, gts)
    return time.perf_counter() - t, co[n_img]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=26446)
    ap.add_argument("--host-images", type=int, default=1000)
    ap.add_argument("--pairs", type=int, default=320, help="pairs scored end to end (after one warm-up batch)")
    ap.add_argument("--batch-pairs", type=int, default=16)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "bf16x3"])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    table, scores = split(a.images)
    sd = scores.to(dev)
    S.vg_recall_device(sd, table)                      # tables to the device, workspace, warm-up
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    k_ms, all_ms = [], []
    for _ in range(a.reps):
        ev[0].record()
        ranks = S.vg_recall_ranks_device(sd, table)
        ev[1].record()
        res = S.vg_recall_from_ranks(ranks, table)     # (returns python floats: includes the device -> host copies)
        ev[2].record()
        torch.cuda.synchronize()
        k_ms.append(ev[0].elapsed_time(ev[1]))
        all_ms.append(ev[0].elapsed_time(ev[2]))
    host_s, host_cands = host_restatement(table, scores, min(a.host_images, a.images))
    host_split_s = host_s * table["n_rows"] / max(host_cands, 1)

    cfg = cfgmod.oscar_base()
    m = REC_MLM_CPT(cfg)
    m.load_state_dict(synth.init_state_dict(cfg, 1, head="cpt"))
    m.tie_weights()
    m.to(dev).eval()
    m.set_compute_dtype(a.dtype)
    idx2pred = {i + 1: [2000 + 3 * i + j for j in range(i % 3 + 1)] for i in range(50)}
    b = synth.make_batch(6, cfg, seed=5, max_seq_len=70, img_seq_len=60)
    rows = torch.tensor([(s, 10 + j) for s in range(6) for j in range(s % 3 + 1)], dtype=torch.int64)
    pairs = [{"img_key": "%d.jpg_0_1" % i, "input_ids": b["input_ids"], "segment_ids": b["segment_ids"],
              "attention_mask": b["attention_mask"], "mask_token_pos": rows, "img_feats": b["img_feats"][0]} for i in range(a.pairs)]
    drivers.val_vg(m, pairs[:a.batch_pairs], idx2pred, dev, batch_pairs=a.batch_pairs)
    torch.cuda.synchronize()
    t = time.perf_counter()
    drivers.val_vg(m, pairs, idx2pred, dev, batch_pairs=a.batch_pairs)
    torch.cuda.synchronize()
    pps = a.pairs / (time.perf_counter() - t)
    split_pairs = table["n_rows"] // 2                 # every unordered pair is one TSV row (forward + reverse scored together)
    split_scoring_s = split_pairs / pps
    print(json.dumps({"images": a.images, "candidates": table["n_rows"], "gt_triplets": int(table["gt"].size(0)),
                      "recall_kernel_ms": round(float(np.median(k_ms)), 3), "recall_total_ms": round(float(np.median(all_ms)), 3),
                      "host_restatement_s_split": round(host_split_s, 2), "host_restatement_images": min(a.host_images, a.images),
                      "R@20": round(res["recall"][20], 6), "dtype": a.dtype, "val_vg_pairs_per_s": round(pps, 1),
                      "batch_pairs": a.batch_pairs, "split_scoring_s": round(split_scoring_s, 1),
                      "recall_share_of_scoring": float("%.3g" % (np.median(all_ms) / 1e3 / split_scoring_s))}), flush=True)


if __name__ == "__main__":
    main()
