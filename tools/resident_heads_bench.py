"""Resident sets with head tables on one GPU: drivers.val_vg, val_vcr, val_vcr_qar and train_batch on host items against the same drivers on a
ResidentSet (cpt_amd/resident.py: from_pairs, from_vcr, from_vcr_qar, from_train_batches).  Oscar-base in bf16, seeded synthetic items:
  val_vg       256 pairs padded 70 + 60 (6 sequences each, 8 pairs per image sharing ONE feature array), 16 pairs per step
  val_vcr      128 questions of 4 choices padded 165 + 45, 8 questions per step (Oscar-base, not Oscar-large)
  val_vcr_qar  64 questions of 4 + 4 sequences padded 165 + 45, 4 questions per step
  train_batch  16 batches of 4 sequences padded 70 + 50, dropout 0.1: the whole optimizer step (batch, label grid, forward, backward, FusedAdamW)
               on the host clock
Host and resident passes share one process and are interleaved, ``--reps`` rounds (at least 5) after one warm pass each, as
tools/resident_bench.py runs them; the median is reported beside every round and a speed-up is claimed only where every resident round beats
every host round.

  python tools/resident_heads_bench.py [--reps 5] [--out profiles/resident_heads_bench.txt]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o res -- python tools/resident_heads_bench.py --trace-run
        a run of its own: the batches of the trimmed val_vg walk, each built 20 times by cpt_gather_batch, 20 times by cpt_gather_batch_heads
        with only the five outputs of cpt_gather_batch, and 20 times by cpt_gather_batch_heads with the label grid (training batches)
  python tools/resident_heads_bench.py --kernel-stats DIR/.../res_kernel_stats.csv --out ...     adds the kernels' launch times"""
import argparse
import csv
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gqa_vcr_bench as GB  # noqa: E402
import rec_eval_bench as REB  # noqa: E402
import resident_bench as RB  # noqa: E402
from cpt_amd import config as cfgmod, drivers, resident, synth  # noqa: E402
from cpt_amd import train as TR  # noqa: E402
from cpt_amd.modeling_vcr import NSPCPT, VCRQAR_NSPCPT  # noqa: E402

VG_LT, VG_LI = 70, 60


def vg_pairs(n, cfg, per_image=8):
    pairs, feats = [], None
    for i in range(n):
        b = synth.make_batch(6, cfg, seed=100 + i, max_seq_len=VG_LT, img_seq_len=VG_LI, vary_regions=True)
        if i % per_image == 0:
            feats, regions = b["img_feats"][0].clone(), b["attention_mask"][0, VG_LT:].clone()
        mask = b["attention_mask"].clone()
        mask[:, VG_LT:] = regions
        rows = [(s, 10 + j) for s in range(6) for j in range(s % 3 + 1)]
        pairs.append({"img_key": "%d.jpg_%d_%d" % (i // per_image, i % per_image, (i + 1) % per_image), "input_ids": b["input_ids"],
                      "segment_ids": b["segment_ids"], "attention_mask": mask, "mask_token_pos": torch.tensor(rows, dtype=torch.int64), "img_feats": feats})
    rng = np.random.Generator(np.random.PCG64(3))
    idx2pred = {i: [int(t) for t in rng.integers(1000, 30000, 1 + i % 3)] for i in range(1, 51)}
    return pairs, idx2pred


def vcr_questions(n, cfg):
    out = []
    for i in range(n):
        b = synth.make_batch(4, cfg, seed=300 + i, max_seq_len=GB.LT, img_seq_len=GB.LI, vary_regions=True)
        mask = b["attention_mask"].clone()
        mask[:, GB.LT:] = mask[0, GB.LT:]
        out.append({"input_ids": b["input_ids"].numpy(), "segment_ids": b["segment_ids"].numpy(), "input_mask": mask.numpy(),
                    "img_feats": b["img_feats"][0].clone(), "label": i % 4, "q_id": i})
    return out


def qar_questions(n, cfg):
    out = []
    for i in range(n):
        parts = []
        for k in range(2):
            b = synth.make_batch(4, cfg, seed=500 + 2 * i + k, max_seq_len=GB.LT, img_seq_len=GB.LI, vary_regions=True)
            if k == 0:
                feats, regions = b["img_feats"][0].clone(), b["attention_mask"][0, GB.LT:].clone()
            mask = b["attention_mask"].clone()
            mask[:, GB.LT:] = regions
            parts.append({"input_ids": b["input_ids"].numpy(), "segment_ids": b["segment_ids"].numpy(), "input_mask": mask.numpy()})
        out.append({"q_a": parts[0], "qa_r": parts[1], "n_ans": 4, "n_rats": 4, "label": (i % 4, (2 * i) % 4), "q_id": i, "img_feats": feats})
    return out


def trace_run(dev, cfg, reps=20):
    pairs, _ = vg_pairs(64, cfg)
    rs = resident.upload(resident.from_pairs(pairs), dev)
    batches = [synth.make_batch(4, cfg, seed=700 + i, max_seq_len=70, img_seq_len=50, vary_regions=True) for i in range(4)]
    ts = resident.upload(resident.from_train_batches(batches), dev, "bf16")       # (another store dtype: the two pairs of kernels differ by name)
    sf = rs.seq_first
    plans = []
    for i in range(0, len(pairs), 16):
        seqs = np.arange(sf[i], sf[i + 16])
        plans.append((torch.as_tensor(seqs.astype(np.int32)).to(dev),) + resident.extent(rs.tables, seqs))
    tplans = [(torch.as_tensor(s.astype(np.int32)).to(dev),) + resident.extent(ts.tables, s, labelled=True) for s in ts.batch_indices()]
    for _ in range(reps):
        for seq, lt, li in plans:
            rs.gather(seq, lt, li, mask_pos=False)
            rs.gather(seq, lt, li, mask_pos=False, heads=())
        for seq, lt, li in tplans:
            ts.gather(seq, lt, li, mask_pos=False)
            ts.gather(seq, lt, li, mask_pos=False, heads=("label_grid",))
    torch.cuda.synchronize()
    print("trace run: %d VG batches of 96 sequences trimmed to %s; %d training batches of 4 sequences trimmed to %s (label grid: %s more bytes)"
          % (len(plans), sorted({p[1:] for p in plans}), len(tplans), [p[1:] for p in tplans], [4 * (p[1] + p[2]) * 8 for p in tplans]))


def kernel_stats(path):
    """{(kernel, store dtype): (launches, average us)}: the VG store of the trace run is fp32, the training store bf16."""
    out = {}
    for r in csv.DictReader(open(path)):
        for k in ("gather_batch_heads_kernel", "gather_batch_kernel"):
            if k in r["Name"]:
                key = (k, "fp32" if "float" in r["Name"] else "bf16")
                calls, avg = int(r["Calls"]), float(r["AverageNs"]) / 1e3
                c0, a0 = out.get(key, (0, 0.0))
                out[key] = (c0 + calls, (a0 * c0 + avg * calls) / (c0 + calls))
                break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = cfgmod.oscar_base()
    if a.trace_run:
        return trace_run(dev, cfg)
    reps = max(a.reps, 5)
    lines = ["resident_heads_bench: Oscar-base, bf16, one GPU; median of %d interleaved rounds after one warm pass per side" % reps]

    def section(title, rs, t_tables, t_upload):
        lines.extend(["", title, "  store: %.1f MB (%d feature rows of %d blocks, %d head rows); tables built on the host in %.2f s, uploaded in %.2f s (once per split)"
                      % (rs.nbytes / 1e6, int(rs.tables["block_rows"].sum()), len(rs.tables["block_rows"]), rs.tables["n_heads"], t_tables, t_upload)])

    m = REB.model(dev)
    pairs, idx2pred = vg_pairs(256, m.config)
    rs, tt, tu = RB.timed_upload(resident.from_pairs(pairs), dev)
    section("val_vg: %d pairs (%d sequences), padded %d + %d, 8 pairs per image share one feature array, 16 pairs per step" % (len(pairs), 6 * len(pairs), VG_LT, VG_LI),
            rs, tt, tu)
    for name, opts in (("plain", {}), ("trim=True", dict(trim=True))):
        run = lambda resident_=None: {"scores": drivers.val_vg(m, pairs, idx2pred, dev, batch_pairs=16, resident=resident_, **opts)[0].cpu()}
        lines.extend(RB.report(name, len(pairs), "pairs", *RB.rounds(run, lambda: run(rs), reps)))
    rs.free()
    del rs, m
    torch.cuda.empty_cache()

    m = GB.model(NSPCPT, cfgmod.oscar_base(), dev).eval()
    qs = vcr_questions(128, m.config)
    rs, tt, tu = RB.timed_upload(resident.from_vcr(qs), dev)
    section("val_vcr: %d questions of 4 choices, padded %d + %d, 8 questions per step (Oscar-base)" % (len(qs), GB.LT, GB.LI), rs, tt, tu)
    for name, opts in (("plain", {}), ("trim=True", dict(trim=True))):
        run = lambda resident_=None: drivers.val_vcr(m, qs, dev, batch_questions=8, resident=resident_, **opts)
        lines.extend(RB.report(name, len(qs), "questions", *RB.rounds(run, lambda: run(rs), reps)))
    rs.free()
    del rs, m
    torch.cuda.empty_cache()

    m = GB.model(VCRQAR_NSPCPT, cfgmod.oscar_base(), dev).eval()
    qq = qar_questions(64, m.config)
    rs, tt, tu = RB.timed_upload(resident.from_vcr_qar(qq), dev)
    section("val_vcr_qar: %d questions of 4 + 4 sequences, padded %d + %d, 4 questions per step" % (len(qq), GB.LT, GB.LI), rs, tt, tu)
    for name, opts in (("plain", {}), ("trim=True", dict(trim=True))):
        run = lambda resident_=None: drivers.val_vcr_qar(m, qq, dev, batch_questions=4, resident=resident_, **opts)
        lines.extend(RB.report(name, len(qq), "questions", *RB.rounds(run, lambda: run(rs), reps)))
    rs.free()
    del rs, m
    torch.cuda.empty_cache()

    m = REB.model(dev)
    drivers.set_dropout(m, 0.1)
    batches = [synth.make_batch(4, m.config, seed=700 + i, max_seq_len=70, img_seq_len=50, vary_regions=True) for i in range(16)]
    rs, tt, tu = RB.timed_upload(resident.from_train_batches(batches), dev)
    section("train_batch: %d batches of 4 sequences, padded 70 + 50, dropout 0.1, FusedAdamW; the whole pass on the host clock" % len(batches), rs, tt, tu)
    opts = types.SimpleNamespace(learning_rate=1e-6, warmup_steps=1, num_train_steps=10 ** 6, lr_mul=1.0)
    opt = TR.FusedAdamW(m, lr=1e-6)
    feed = rs.batch_indices()
    for name, kw in (("plain", {}), ("trim=True", dict(trim=True))):
        host = lambda: {"n": np.int64(drivers.train_batch(m, opt, batches, opts, dev, **kw)[0])}
        res = lambda: {"n": np.int64(drivers.train_batch(m, opt, feed, opts, dev, resident=rs, **kw)[0])}
        th, tr, _ = RB.rounds(host, res, reps)
        lines.extend(RB.report(name + " (the parameters move between passes: results not compared here)", len(batches), "steps", th, tr, True)[:3])
        lines.append("    resident / host %.3f; every resident round beats every host round: %s"
                     % (float(np.median(th)) / float(np.median(tr)), "yes" if max(tr) < min(th) else "NO (no speed-up claimed)"))
    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        lines.extend(["", "kernel launch times (rocprofv3 --kernel-trace --stats, a run of its own, 20 launches per batch and kernel):",
                      "  4 trimmed VG batches of 96 sequences out of an fp32 store, the five outputs of cpt_gather_batch from either entry point;",
                      "  4 trimmed training batches of 4 sequences out of a bf16 store, cpt_gather_batch against cpt_gather_batch_heads WITH the label grid",
                      "  (B x (Lt' + Li') x 8 bytes more per launch, about 3 KB)"])
        for (k, dt), (calls, us) in sorted(ks.items(), key=lambda x: (x[0][1], x[0][0])):
            lines.append("  %-28s %s store %6d launches, average %.2f us" % (k, dt, calls, us))
        for dt, what in (("fp32", "the five old outputs: accepted up to 1.10"), ("bf16", "with the label grid: reported, no bar")):
            if ("gather_batch_heads_kernel", dt) in ks and ("gather_batch_kernel", dt) in ks:
                lines.append("  gather_batch_heads / gather_batch, %s store = %.3f (%s)"
                             % (dt, ks[("gather_batch_heads_kernel", dt)][1] / ks[("gather_batch_kernel", dt)][1], what))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
