"""RefCOCO REC evaluation on one GPU: drivers.val_rec against what a user runs without it, drivers.val_queries followed by scoring.accuracy.
Oscar-base in bf16 on seeded synthetic ragged queries (4..40 proposal sequences each, padded 70 + 50, 36 regions, 1..3 colours per sequence),
4 queries per batch.  Both variants share one process and are interleaved, ``--reps`` rounds (at least 5) after one warm pass each; the median
is reported beside every round, because val_queries rounds are known to scatter.

Per variant: queries/s of the whole pass (table building, batch assembly, H2D copies, the final read-back and the host accuracy loop included:
that is what a val loop pays), and per step the host time spent OUTSIDE the forward (the step's wall time on the host minus the time inside the
model call, microseconds: batch assembly + H2D + the selection call) and inside the selection call alone (scoring.select_regions_device /
scoring.rec_choose_device).  No synchronisation is added inside a pass; a call's own blocking H2D copy (the id tensor select_regions_device
uploads from pageable memory waits for the stream, so for the forward before it) counts as host time of that call -- the host is held there.

  python tools/rec_eval_bench.py [--reps 5] [--queries 64] [--out profiles/rec_eval_bench.txt]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o rec -- python tools/rec_eval_bench.py --trace-run      # a run of its own: 3 passes of each variant
  python tools/rec_eval_bench.py --kernel-stats DIR/.../rec_kernel_stats.csv --out ...               # adds the two kernels' launch times"""
import argparse
import csv
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpt_amd import config as cfgmod, drivers, scoring, synth  # noqa: E402
from cpt_amd.modeling_bert import BertImgForPreTraining  # noqa: E402
from cpt_amd.modeling_rec import REC_MLM_CPT  # noqa: E402


def model(dev):
    cfg = cfgmod.oscar_base()
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
    pre = BertImgForPreTraining(cfg)
    pre.load_state_dict(synth.init_state_dict(cfg, 1, head="pretrain"))
    pre.tie_weights()
    m = REC_MLM_CPT(cfg)
    m.copy_from_pretraining_model(pre)
    m.to(dev).set_compute_dtype("bf16")
    return m.eval()


def refcoco_queries(n, cfg, seed=0):
    """Ragged queries and one annotation each: every candidate its own box, the annotation a jittered copy of one of them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    qs, gts = [], []
    for i in range(n):
        P = int(rng.integers(4, 41))
        b = synth.make_batch(P, cfg, seed=1000 + i, max_seq_len=70, img_seq_len=50, n_regions=36)
        q = {k: b[k] for k in ("img_feats", "input_ids", "segment_ids", "attention_mask", "mask_token_pos")}
        q["colors"] = [[int(c) for c in rng.choice(synth.COLOR_IDS, size=int(rng.integers(1, 4)), replace=False)] for _ in range(P)]
        q["rects"] = []
        for c in q["colors"]:
            xy = rng.uniform(0, 400, (len(c), 2))
            wh = rng.uniform(20, 200, (len(c), 2))
            q["rects"].append([[float(x), float(y), float(x + w), float(y + h)] for (x, y), (w, h) in zip(xy, wh)])
        flat = [r for rs in q["rects"] for r in rs]
        r = flat[int(rng.integers(0, len(flat)))]
        gts.append([r[0] + float(rng.uniform(-3, 3)), r[1] + float(rng.uniform(-3, 3)), r[2] - r[0] + 1, r[3] - r[1] + 1])
        qs.append(q)
    return qs, gts


class StepClock(object):
    """Host time of every step of drivers._eval_pass, of the model call inside it and of the selection call inside it."""

    def __init__(self, m):
        self.reset()
        inner_pass = drivers._eval_pass

        def eval_pass(n_items, groups_of, outputs, step, device, bucket):
            def timed(idx, lo):
                t = time.perf_counter()
                out = step(idx, lo)
                self.step += time.perf_counter() - t
                self.steps += 1
                return out
            return inner_pass(n_items, groups_of, outputs, timed, device, bucket)
        drivers._eval_pass = eval_pass
        inner_fwd = m.forward

        def forward(*a, **kw):
            t = time.perf_counter()
            out = inner_fwd(*a, **kw)
            self.fwd += time.perf_counter() - t
            return out
        m.forward = forward
        for name in ("select_regions_device", "rec_choose_device"):
            setattr(scoring, name, self._timed_choice(getattr(scoring, name)))

    def _timed_choice(self, fn):
        def run(*a, **kw):
            t = time.perf_counter()
            out = fn(*a, **kw)
            self.choice += time.perf_counter() - t
            return out
        return run

    def reset(self):
        self.step = self.fwd = self.choice = 0.0
        self.steps = 0

    def take(self):
        out = ((self.step - self.fwd) / max(self.steps, 1) * 1e6, self.choice / max(self.steps, 1) * 1e6, self.steps)
        self.reset()
        return out


def variants(m, qs, gts, dev):
    def today():
        preds = drivers.val_queries(m, qs, synth.NONE_ID, dev)
        return scoring.accuracy({k: v[1] for k, v in preds.items()}, gts)

    def rec():
        return drivers.val_rec(m, qs, gts, synth.NONE_ID, dev)["accuracy"]
    col_ids = sorted({int(c) for q in qs for s in q["colors"] for c in s} | {synth.NONE_ID})
    table = scoring.rec_eval_table(qs, gts, synth.NONE_ID, col_ids, device=dev)

    def rec_table():
        return drivers.val_rec(m, qs, gts, synth.NONE_ID, dev, table=table)["accuracy"]
    return [("val_queries + scoring.accuracy", today), ("val_rec", rec), ("val_rec, table built once", rec_table)]


def kernel_stats(path):
    """{kernel name: (calls, average us)} of the selection kernels out of a rocprofv3 kernel_stats.csv."""
    out = {}
    for r in csv.DictReader(open(path)):
        for k in ("rec_choose_kernel", "select_regions_kernel"):
            if k in r["Name"]:
                out[k] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3)
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
    m = model(dev)
    qs, gts = refcoco_queries(a.queries, m.config)
    n_seq = sum(q["input_ids"].size(0) for q in qs)
    n_cand = sum(len(c) for q in qs for c in q["colors"])
    if a.trace_run:
        for _ in range(3):
            for _, run in variants(m, qs, gts, dev)[:2]:
                run()
        torch.cuda.synchronize()
        return
    reps = max(a.reps, 5)
    clock = StepClock(m)
    runs = variants(m, qs, gts, dev)
    acc = {}
    for name, run in runs:                               # one warm pass each
        acc[name] = run()
        torch.cuda.synchronize()
    assert len(set(acc.values())) == 1, acc             # the variants report the same accuracy
    clock.reset()
    times = {name: [] for name, _ in runs}
    host = {name: [] for name, _ in runs}
    for _ in range(reps):
        for name, run in runs:
            torch.cuda.synchronize()
            t = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t)
            host[name].append(clock.take())
    lines = ["rec_eval_bench: Oscar-base, bf16, one GPU; %d queries (%d sequences, %d candidates), padded 70 + 50, 4 queries per batch; accuracy %.2f"
             % (len(qs), n_seq, n_cand, acc[runs[0][0]]),
             "median of %d interleaved rounds after one warm pass per variant; host times per step (%d steps per pass), microseconds" % (reps, host[runs[0][0]][0][2]),
             "", "  %-32s %10s %8s %22s %20s   %s" % ("variant", "queries/s", "vs first", "host outside fwd us/step", "selection call us/step", "queries/s of every round")]
    base = None
    for name, _ in runs:
        rate = len(qs) / float(np.median(times[name]))
        base = base or rate
        lines.append("  %-32s %10.1f %8.3f %22.1f %20.1f   %s" % (name, rate, rate / base, float(np.median([h[0] for h in host[name]])),
                                                                float(np.median([h[1] for h in host[name]])), " ".join("%.1f" % (len(qs) / x) for x in times[name])))
    spread = {name: (max(times[name]) - min(times[name])) / float(np.median(times[name])) for name, _ in runs}
    lines += ["", "round-to-round spread (max - min) / median: " + ", ".join("%s %.1f%%" % (n, 100 * s) for n, s in spread.items())]
    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        lines += ["", "kernel launch times (rocprofv3 --kernel-trace --stats, a run of its own: 3 passes of each variant):"]
        for k, (calls, us) in sorted(ks.items()):
            lines.append("  %-24s %6d launches, average %.2f us" % (k, calls, us))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
