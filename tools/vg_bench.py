"""VG-CPT predicate scoring step on Oscar-base shapes (random weights): the device route (cpt_model_fwd_rows on the predicate
word-piece columns with the full-vocabulary log-sum-exp, then cpt_mean_logprob_scores) against the reference's own call form
(REC_MLM_CPT.forward without mask_token_pos: every row through the vocabulary head, then softmax and gather), same box, same run.

    python tools/vg_bench.py [--pairs 16 64] [--steps 10] [--dtype bf16]

For the head's kernel times (decoder GEMM writing [n_rows][V] fp32 into the workspace, row log-sum-exp, column gather, scores) run
`rocprofv3 --kernel-trace --stats -- python tools/vg_bench.py --kernels`: that mode runs only the scoring route, three times.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpt_amd import config as cfgmod, scoring as S, synth          # noqa: E402
from cpt_amd.modeling_rec import REC_MLM_CPT                         # noqa: E402


def batch(n_pairs, cfg, dev):
    b = synth.make_batch(6 * n_pairs, cfg, seed=5, max_seq_len=70, img_seq_len=60)
    rows = []
    for s in range(6 * n_pairs):
        rows += [(s, 10 + j) for j in range(s % 3 + 1)]
    return {k: v.to(dev) for k, v in b.items()}, torch.tensor(rows, dtype=torch.int64, device=dev)


def timed(fn, steps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "bf16x3"])
    ap.add_argument("--kernels", action="store_true", help="only the scoring route, three times (for a rocprofv3 kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = cfgmod.oscar_base()
    m = REC_MLM_CPT(cfg)
    m.load_state_dict(synth.init_state_dict(cfg, 1, head="cpt"))
    m.tie_weights()
    m.to(dev).eval()
    m.set_compute_dtype(a.dtype)
    idx2pred = {i + 1: [2000 + 3 * i + j for j in range(i % 3 + 1)] for i in range(50)}
    cols = S.vg_candidates(idx2pred)[0].to(dev)
    for n_pairs in a.pairs:
        d, mtp = batch(n_pairs, cfg, dev)
        with torch.no_grad():
            if a.kernels:
                for _ in range(3):
                    S.vg_predicate_scores(m, d["input_ids"], d["segment_ids"], d["attention_mask"], d["img_feats"], mtp, idx2pred)
                torch.cuda.synchronize()
                continue

            def rows():
                S.vg_predicate_scores(m, d["input_ids"], d["segment_ids"], d["attention_mask"], d["img_feats"], mtp, idx2pred)

            def all_rows():
                out = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"])[0]
                p = out[mtp[:, 0], mtp[:, 1]].softmax(-1)
                return p[:, cols].log()

            t_rows = timed(rows, a.steps)
            torch.cuda.empty_cache()
            t_all = timed(all_rows, a.steps)
        print(json.dumps({"pairs": n_pairs, "sequences": 6 * n_pairs, "head_rows": int(mtp.size(0)), "dtype": a.dtype,
                          "val_vg_step_ms": round(t_rows, 3), "all_row_route_ms": round(t_all, 3)}), flush=True)


if __name__ == "__main__":
    main()
