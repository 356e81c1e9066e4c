"""Device-resident evaluation sets on one GPU: drivers.val_rec and drivers.val_gqa on host items against the same drivers on a ResidentSet
(cpt_amd/resident.py).  The setting of tools/rec_eval_bench.py: Oscar-base in bf16, 64 seeded synthetic ragged queries of 4..40 proposal
sequences (padded 70 + 50, 36 regions), 4 queries per batch, the evaluation table built once for both sides; plain, with trim=True and with
max_sequences=64.  val_gqa as tools/gqa_vcr_bench.py runs it: 512 questions padded 165 + 45, 1853 labels, 256 questions per step.
Host and resident passes share one process and are interleaved, ``--reps`` rounds (at least 5) after one warm pass each; the median is
reported beside every round.  A speed-up is claimed only where EVERY resident round beats EVERY host round of the same run.  Building the
tables, the upload and the store's bytes are reported on their own: they are paid once per split, not per pass.

  python tools/resident_bench.py [--reps 5] [--out profiles/resident_bench.txt]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o res -- python tools/resident_bench.py --trace-run
        a run of its own: the batches of the trimmed val_rec walk, each built 20 times by cpt_gather_batch out of the store and 20 times by
        cpt_trim_batch out of the padded device batch -- the same output shapes, the same bytes written
  python tools/resident_bench.py --kernel-stats DIR/.../res_kernel_stats.csv --out ...     adds the two kernels' launch times"""
import argparse
import csv
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gqa_vcr_bench as GB  # noqa: E402
import rec_eval_bench as REB  # noqa: E402
from cpt_amd import _lib as L, drivers, resident, scoring, synth  # noqa: E402


def gqa_questions(cfg, n_labels=1853):
    rng = np.random.Generator(np.random.PCG64(0))
    labels = ["%d x%d" % (int(t), i) for i, t in enumerate(rng.integers(1000, 30000, n_labels))]
    qs = []
    for i in range(2):
        b = synth.make_batch(256, cfg, seed=20 + i, max_seq_len=GB.LT, img_seq_len=GB.LI)
        for j in range(256):
            qs.append({"input_ids": b["input_ids"][j], "segment_ids": b["segment_ids"][j], "input_mask": b["attention_mask"][j],
                       "img_feats": b["img_feats"][j], "mask_token_pos": [int(b["mask_token_pos"][j])], "q_id": np.array([i * 256 + j]),
                       "igt": [int(x) for x in rng.integers(0, n_labels, 1 + j % 3)]})
    return qs, labels


def timed_upload(items, dev, feature_dtype="fp32"):
    t0 = time.perf_counter()
    t = resident.tables(items)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    rs = resident.upload(t, dev, feature_dtype)
    torch.cuda.synchronize()
    return rs, t1 - t0, time.perf_counter() - t1


def rounds(host, res, reps):
    """Interleaved rounds after one warm pass each -> (host seconds, resident seconds); the two sides' results are compared once."""
    a, b = host(), res()
    torch.cuda.synchronize()
    same = all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a if isinstance(a[k], (np.ndarray, torch.Tensor)))
    th, tr = [], []
    for _ in range(reps):
        for fn, ts in ((host, th), (res, tr)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
    return th, tr, same


def report(name, n, unit, th, tr, same):
    mh, mr = float(np.median(th)), float(np.median(tr))
    wins = max(tr) < min(th)
    return ["  %s" % name,
            "    host items  %9.1f %s/s   rounds: %s" % (n / mh, unit, " ".join("%.1f" % (n / x) for x in th)),
            "    resident    %9.1f %s/s   rounds: %s" % (n / mr, unit, " ".join("%.1f" % (n / x) for x in tr)),
            "    resident / host %.3f; every resident round beats every host round: %s; results equal bit for bit: %s"
            % (mh / mr, "yes" if wins else "NO (no speed-up claimed)", "yes" if same else "NO")]


def trace_run(m, qs, rs, dev, reps=20):
    """The batches of the trimmed walk, built by cpt_gather_batch out of the store and by cpt_trim_batch out of the padded device batch."""
    t = rs.tables
    sf = t["seq_first"]
    st = L.stream_ptr()
    batches = []
    for i in range(0, len(qs), 4):
        seqs = np.arange(sf[i], sf[min(i + 4, len(qs))])
        lt, li = resident.extent(t, seqs)
        pad = {k: torch.cat([q[k] for q in qs[i:i + 4]], 0).to(dev).contiguous() for k in ("input_ids", "segment_ids", "attention_mask", "img_feats")}
        batches.append((torch.as_tensor(seqs.astype(np.int32)).to(dev), lt, li, pad))
    for _ in range(reps):
        for seq, lt, li, pad in batches:
            rs.gather(seq, lt, li)
            B, Lt = pad["input_ids"].shape
            Li, D = pad["img_feats"].shape[1:]
            e = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)
            ids, tt, mask, feats = e(B, lt), e(B, lt), e(B, lt + li), torch.empty((B, li, D), dtype=torch.float32, device=dev)
            L.check(L.lib().cpt_trim_batch(pad["input_ids"].data_ptr(), pad["segment_ids"].data_ptr(), None, pad["attention_mask"].data_ptr(),
                                           pad["img_feats"].data_ptr(), B, Lt, Li, D, lt, li, ids.data_ptr(), tt.data_ptr(), None, mask.data_ptr(),
                                           feats.data_ptr(), st), "cpt_trim_batch")
    torch.cuda.synchronize()
    return [(s.numel(), lt, li) for s, lt, li, _ in batches]


def kernel_stats(path):
    out = {}
    for r in csv.DictReader(open(path)):
        for k in ("gather_batch_kernel", "trim_batch_kernel"):
            if k in r["Name"]:
                calls, avg = int(r["Calls"]), float(r["AverageNs"]) / 1e3
                c0, a0 = out.get(k, (0, 0.0))
                out[k] = (c0 + calls, (a0 * c0 + avg * calls) / (c0 + calls))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = REB.model(dev)
    qs, gts = REB.refcoco_queries(a.queries, m.config)
    n_seq = sum(q["input_ids"].size(0) for q in qs)
    rs, t_tables, t_upload = timed_upload(resident.from_queries(qs), dev)
    if a.trace_run:
        shapes = trace_run(m, qs, rs, dev)
        print("trace run: %d batches, B %d..%d, trimmed to %s" % (len(shapes), min(s[0] for s in shapes), max(s[0] for s in shapes),
                                                                 sorted({s[1:] for s in shapes})))
        return
    reps = max(a.reps, 5)
    col_ids = sorted({int(c) for q in qs for s in q["colors"] for c in s} | {synth.NONE_ID})
    table = scoring.rec_eval_table(qs, gts, synth.NONE_ID, col_ids, device=dev)
    lines = ["resident_bench: Oscar-base, bf16, one GPU; median of %d interleaved rounds after one warm pass per side" % reps, "",
             "val_rec: %d queries (%d sequences), padded 70 + 50, 36 regions, 4 queries per batch, evaluation table built once" % (len(qs), n_seq),
             "  store: %.1f MB fp32 features + tables (%d feature rows of %d blocks); tables built on the host in %.2f s, uploaded in %.2f s (once per split)"
             % (rs.nbytes / 1e6, int(rs.tables["block_rows"].sum()), len(rs.tables["block_rows"]), t_tables, t_upload)]
    for name, opts in (("plain", {}), ("trim=True", dict(trim=True)), ("max_sequences=64", dict(max_sequences=64))):
        th, tr, same = rounds(lambda: drivers.val_rec(m, qs, gts, synth.NONE_ID, dev, table=table, **opts),
                              lambda: drivers.val_rec(m, qs, gts, synth.NONE_ID, dev, table=table, resident=rs, **opts), reps)
        lines += report(name, len(qs), "queries", th, tr, same)
    half, _, t_half = timed_upload(resident.from_queries(qs), dev, "bf16")
    th, tr, same = rounds(lambda: drivers.val_rec(m, qs, gts, synth.NONE_ID, dev, table=table),
                          lambda: drivers.val_rec(m, qs, gts, synth.NONE_ID, dev, table=table, resident=half), reps)
    lines += report("plain, bf16 feature store (%.1f MB, uploaded in %.2f s)" % (half.nbytes / 1e6, t_half), len(qs), "queries", th, tr, same)
    rs.free()
    half.free()
    del rs, half
    torch.cuda.empty_cache()
    gq, labels = gqa_questions(m.config)
    tok = GB.IdTokenizer()
    grs, t_tables, t_upload = timed_upload(resident.from_questions(gq), dev)
    lines += ["", "val_gqa: %d questions, padded %d + %d, %d labels, 256 questions per step" % (len(gq), GB.LT, GB.LI, len(labels)),
              "  store: %.1f MB; tables built in %.2f s, uploaded in %.2f s" % (grs.nbytes / 1e6, t_tables, t_upload)]
    th, tr, same = rounds(lambda: drivers.val_gqa(m, gq, labels, tok, dev), lambda: drivers.val_gqa(m, gq, labels, tok, dev, resident=grs), reps)
    lines += report("plain", len(gq), "questions", th, tr, same)
    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        lines += ["", "kernel launch times (rocprofv3 --kernel-trace --stats, a run of its own: the 16 batches of the trimmed val_rec walk, 20 times each,",
                  "built by cpt_gather_batch out of the store and by cpt_trim_batch out of the padded device batch: the same output shapes):"]
        for k, (calls, us) in sorted(ks.items()):
            lines.append("  %-22s %6d launches, average %.2f us" % (k, calls, us))
        if len(ks) == 2:
            ratio = ks["gather_batch_kernel"][1] / ks["trim_batch_kernel"][1]
            lines.append("  gather / trim = %.3f (accepted up to 1.10)" % ratio)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
