"""Length-aware training on one GPU: the few-shot step on padded batches with the options off (the parent commit's code path) and with
``trim=True`` (the drivers' host path), interleaved in one process on one card, bf16, dropout 0.

  GQA  Oscar-base, REC_MLM_CPT through drivers.train_gqa_batch; 4 sequences padded to 165 + 45
  VCR  Oscar-large, NSPCPT through drivers.train_vcr_batch; one question of 4 answer choices padded to 165 + 45
  Stated distribution (seeded, uniform, per sequence): text 12..40 word-pieces (GQA) or 30..110 (VCR), regions 10..45.

Per configuration: ms per optimizer step (one micro-step each: host batch assembly, H2D copies, forward, backward, clip and AdamW included -- what
a training loop pays) and encoder rows executed per step (B x (Lt' + Li') from engine.last_train_shape).  ``--steps`` micro-batches per round,
``--reps`` interleaved rounds after one warm round, the median round is reported.

The device path (``model.trim_training`` on padded device tensors) is timed apart on the GQA batches: per training forward cpt_train_extents,
the 8-byte read-back and cpt_trim_batch_labels, each apart (the launches between two stream events, the read-back on the host clock), and the
whole call on the host clock.

  python tools/train_trim_bench.py [--steps 16] [--reps 5] [--out profiles/train_trim_bench.txt]"""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpt_amd import config as cfgmod, drivers, synth  # noqa: E402
from cpt_amd.modeling_bert import BertImgForPreTraining  # noqa: E402
from cpt_amd.modeling_rec import REC_MLM_CPT  # noqa: E402
from cpt_amd.modeling_vcr import NSPCPT  # noqa: E402
from cpt_amd.train import AdamW, WarmupLinearSchedule, trim_training_batch  # noqa: E402

LT, LI, B, D = 165, 45, 4, 2054


def build(cls, cfg, dev):
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
    pre = BertImgForPreTraining(cfg)
    pre.load_state_dict(synth.init_state_dict(cfg, 1, head="pretrain"))
    pre.tie_weights()
    m = cls(cfg)
    m.copy_from_pretraining_model(pre)
    m.to(dev).set_compute_dtype("bf16")
    return m.train()


def sequences(rng, t_lo, t_hi):
    """B padded sequences: ids, segment ids, mask, features; one [MASK] per sequence."""
    ids = np.zeros((B, LT), np.int64)
    mask = np.zeros((B, LT + LI), np.int64)
    feats = np.zeros((B, LI, D), np.float32)
    for i in range(B):
        t, r = int(rng.integers(t_lo, t_hi + 1)), int(rng.integers(10, LI + 1))
        ids[i, :t] = rng.integers(1000, 30000, t)
        ids[i, 0], ids[i, t - 2], ids[i, t - 1] = synth.CLS, synth.MASK, synth.SEP
        mask[i, :t] = 1
        mask[i, LT:LT + r] = 1
        feats[i, :r] = np.maximum(rng.standard_normal((r, D), dtype=np.float32), 0)
    return ids, np.zeros((B, LT), np.int64), mask, feats


def gqa_batches(n, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for _ in range(n):
        ids, seg, mask, feats = sequences(rng, 12, 40)
        out.append({"input_ids": torch.from_numpy(ids), "segment_ids": torch.from_numpy(seg), "attention_mask": torch.from_numpy(mask),
                    "img_feats": torch.from_numpy(feats), "label_id": torch.from_numpy(rng.integers(0, 64, B))})
    return out


def vcr_batches(n, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for k in range(n):
        ids, seg, mask, feats = sequences(rng, 30, 110)
        out.append([{"input_ids": ids, "input_mask": mask, "segment_ids": seg, "img_feats": torch.from_numpy(feats), "label": k % 4, "q_id": k}])
    return out


def measure(m, run, steps, reps):
    """run(trim) does ``steps`` optimizer steps.  -> {trim: (median ms per step, rows per step, every round's ms per step)}."""
    rows = {}
    for trim in (False, True):               # the warm round, which also counts the rows
        shapes = []
        from cpt_amd import train as T
        inner = T._TrainState.workspace

        def spy(self, b, lt, li, n_rows=0):          # every training forward asks for its workspace with the shape that runs
            shapes.append((b, lt, li))
            return inner(self, b, lt, li, n_rows)
        T._TrainState.workspace = spy
        try:
            run(trim)
        finally:
            T._TrainState.workspace = inner
        torch.cuda.synchronize()
        rows[trim] = sum(s[0] * (s[1] + s[2]) for s in shapes) / float(steps)
    times = {False: [], True: []}
    for _ in range(reps):
        for trim in (False, True):
            torch.cuda.synchronize()
            t = time.perf_counter()
            run(trim)
            torch.cuda.synchronize()
            times[trim].append((time.perf_counter() - t) / steps * 1e3)
    return {trim: (float(np.median(times[trim])), rows[trim], times[trim]) for trim in (False, True)}


def report(title, res, lines):
    lines.append(title)
    lines.append("  %-10s %12s %10s %14s %10s   %s" % ("trim", "ms/step", "vs off", "rows/step", "vs off", "every round (ms/step)"))
    off = res[False]
    for trim in (False, True):
        ms, rows, every = res[trim]
        lines.append("  %-10s %12.3f %10.3f %14.1f %10.3f   %s" % ("on" if trim else "off", ms, ms / off[0], rows, rows / off[1], " ".join("%.3f" % x for x in every)))
    lines.append("")


def device_path(m, batches, dev, lines, iters=200):
    """The three pieces of the device path apart, on the first padded GQA batches (label grid form), and the whole call."""
    import ctypes  # noqa: F401
    from cpt_amd import _lib as L
    eng = m._engine()
    eng.ensure_packed()
    lib, st = L.lib(), L.stream_ptr()

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3

    t_ext, t_read, t_trim, t_all, cuts = [], [], [], [], []
    for b in batches[:8]:
        d = {k: v.to(dev) for k, v in b.items()}
        grid = drivers.gqa_label_grid(d["input_ids"], d["attention_mask"], d["label_id"], torch.arange(1000, 1064, device=dev))
        ids, seg, mask, feats = d["input_ids"], d["segment_ids"], d["attention_mask"], d["img_feats"]
        ext = torch.zeros(2, dtype=torch.int32, device=dev)
        extents = lambda: L.check(lib.cpt_train_extents(mask.data_ptr(), B, LT, LI, grid.data_ptr(), None, 0, ext.data_ptr(), st), "cpt_train_extents")
        t_ext.append(events(extents))
        reads = []
        for _ in range(iters):                      # launch, then the blocking 8-byte read-back: the launch's own time is taken off
            extents()
            t = time.perf_counter()
            lt2, li2 = ext.tolist()
            reads.append((time.perf_counter() - t) * 1e6)
        t_read.append(float(np.median(reads)))
        cuts.append((lt2, li2))
        o = [torch.empty((B, lt2), dtype=torch.int64, device=dev) for _ in range(2)] + [torch.empty((B, lt2 + li2), dtype=torch.int64, device=dev)
                                                                                      for _ in range(2)]
        fo = torch.empty((B, max(li2, 1), D), dtype=torch.float32, device=dev)
        t_trim.append(events(lambda: L.check(lib.cpt_trim_batch_labels(ids.data_ptr(), seg.data_ptr(), None, mask.data_ptr(), feats.data_ptr(),
                                                                       grid.data_ptr(), B, LT, LI, D, lt2, li2, o[0].data_ptr(), o[1].data_ptr(), None,
                                                                       o[2].data_ptr(), fo.data_ptr(), o[3].data_ptr(), st), "cpt_trim_batch_labels")))
        args = (eng, ids, seg, mask, None, feats, grid)
        trim_training_batch(*args)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(iters):
            trim_training_batch(*args)
        torch.cuda.synchronize()
        t_all.append((time.perf_counter() - t) / iters * 1e6)
    med = lambda x: float(np.median(x))
    lines.append("device path (model.trim_training), padded GQA batches, B = 4, 165 + 45, label grid form; medians over %d batches (cut to %s)"
                 % (len(cuts), ", ".join("%d+%d" % c for c in cuts)))
    lines.append("  cpt_train_extents, back to back between two stream events:        %8.1f us per launch" % med(t_ext))
    lines.append("  8-byte read-back behind the launch (host clock, blocking .tolist): %8.1f us" % med(t_read))
    lines.append("  cpt_trim_batch_labels, back to back between two stream events:     %8.1f us per launch" % med(t_trim))
    lines.append("  the whole call (extents, read-back, allocation of the trimmed tensors, trim), host clock: %.1f us per training forward" % med(t_all))
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["train_trim_bench: bf16, dropout 0, one GPU, 4 sequences padded to 165 + 45; %d optimizer steps per round, median of %d interleaved "
             "rounds after one warm round" % (a.steps, a.reps), ""]
    opts = types.SimpleNamespace(gradient_accumulation_steps=1, max_grad_norm=1.0)

    m = build(REC_MLM_CPT, cfgmod.oscar_base(), dev)
    opt = AdamW(m, lr=1e-5, eps=1e-6, weight_decay=0.05)
    sch = WarmupLinearSchedule(opt, warmup_steps=0, t_total=10 ** 6)
    gb = gqa_batches(a.steps)
    tokens = torch.arange(1000, 1064)
    res = measure(m, lambda trim: drivers.train_gqa_batch(m, opt, sch, gb, opts, dev, tokens, trim=trim), a.steps, a.reps)
    report("train_gqa_batch, Oscar-base: text 12..40, regions 10..45 per sequence (uniform)", res, lines)
    device_path(m, gb, dev, lines)
    del m, opt, sch
    torch.cuda.empty_cache()

    m = build(NSPCPT, cfgmod.oscar_large(), dev)
    opt = AdamW(m, lr=1e-5, eps=1e-6, weight_decay=0.05)
    sch = WarmupLinearSchedule(opt, warmup_steps=0, t_total=10 ** 6)
    vb = vcr_batches(a.steps)
    res = measure(m, lambda trim: drivers.train_vcr_batch(m, opt, sch, vb, opts, dev, trim=trim), a.steps, a.reps)
    report("train_vcr_batch, Oscar-large: text 30..110, regions 10..45 per sequence (uniform)", res, lines)

    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
