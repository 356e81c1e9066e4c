"""Length-aware evaluation on one GPU: drivers.val_gqa and drivers.val_queries on seeded synthetic data of stated length distributions, Oscar-base
in bf16, with the new options off (the parent commit's code path), with trim, with trim + bucket, and (val_queries) with max_sequences on top.
All runs share one process; the configurations are interleaved, ``--reps`` rounds, the median is reported.

  GQA      padded 165 + 45; per question text 8..30 word-pieces and 10..45 regions (uniform), 256 questions per batch
  RefCOCO  padded 70 + 50; per query 4..40 proposal sequences (uniform), 36 regions, text as synth.make_batch writes it (about 10 + one
           word-piece per region); 4 queries per batch, or whole queries up to 64 sequences with max_sequences

Per configuration: items/s (host batch assembly and the H2D copies included: that is what a val loop pays), encoder rows executed per item
(B x (Lt' + Li') of every forward, from engine.last_shape) and the H2D bytes of the batch tensors, computed from the shapes that were moved.

  python tools/eval_trim_bench.py [--reps 3] [--out profiles/eval_trim_bench.txt]
  python tools/eval_trim_bench.py --plain          # options never passed, rows from the padded shape: runs on the parent commit as well
  python tools/eval_trim_bench.py --device-path    # cpt_batch_extents + read-back + cpt_trim_batch per forward on a padded device batch, and
                                                   # cpt_pad_cast over the same rows as the yardstick (run it under rocprofv3 --kernel-trace --stats)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpt_amd import _lib as L, config as cfgmod, drivers, synth  # noqa: E402
from cpt_amd.modeling_bert import BertImgForPreTraining  # noqa: E402
from cpt_amd.modeling_rec import REC_MLM_CPT  # noqa: E402

D = 2054


class IdTokenizer(object):
    """Labels are written "<id> ..." here: the first piece of a label is its first word, its vocabulary id that number."""

    def tokenize(self, s):
        return s.split()

    def convert_tokens_to_ids(self, toks):
        return [int(t) if t.isdigit() else 100 for t in toks]


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


def gqa_questions(n, n_labels, seed=0, Lt=165, Li=45):
    rng = np.random.Generator(np.random.PCG64(seed))
    qs = []
    for i in range(n):
        t, r = int(rng.integers(8, 31)), int(rng.integers(10, 46))
        ids = np.zeros(Lt, np.int64)
        ids[:t] = rng.integers(1000, 30000, t)
        ids[0], ids[t - 2], ids[t - 1] = synth.CLS, synth.MASK, synth.SEP
        mask = np.zeros(Lt + Li, np.int64)
        mask[:t] = 1
        mask[Lt:Lt + r] = 1
        feats = np.zeros((Li, D), np.float32)
        feats[:r] = np.maximum(rng.standard_normal((r, D), dtype=np.float32), 0)
        qs.append({"input_ids": torch.from_numpy(ids), "segment_ids": torch.zeros(Lt, dtype=torch.int64), "input_mask": torch.from_numpy(mask),
                   "img_feats": torch.from_numpy(feats), "mask_token_pos": [t - 2], "q_id": np.array([i]),
                   "igt": [int(x) for x in rng.integers(0, n_labels, 1 + i % 3)]})
    return qs


def refcoco_queries(n, cfg, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    qs = []
    for i in range(n):
        P = int(rng.integers(4, 41))
        b = synth.make_batch(P, cfg, seed=1000 + i, max_seq_len=70, img_seq_len=50, n_regions=36)
        q = {k: b[k] for k in ("img_feats", "input_ids", "segment_ids", "attention_mask", "mask_token_pos")}
        q["colors"] = [[int(c) for c in rng.choice(synth.COLOR_IDS, size=int(rng.integers(1, 4)), replace=False)] for _ in range(P)]
        q["rects"] = [[[0, 0, 10, 10]] * len(c) for c in q["colors"]]
        qs.append(q)
    return qs


class Counter(object):
    """Rows executed and batch bytes moved, from the shape of every forward (engine.last_shape; the padded shape where the engine has none)."""

    def __init__(self, m, padded):
        self.eng, self.padded = m._engine(), padded
        inner = self.eng.forward

        def run(*a, **kw):
            out = inner(*a, **kw)
            B = a[0].size(0)
            shape = getattr(self.eng, "last_shape", None) or (B,) + self.padded
            self.rows += shape[0] * (shape[1] + shape[2])
            # input_ids + segment_ids + attention_mask (int64), img_feats (fp32), mask_token_pos (int64)
            self.h2d += shape[0] * (8 * (2 * shape[1] + shape[1] + shape[2]) + 4 * shape[2] * D + 8)
            return out
        self.eng.forward = run
        self.reset()

    def reset(self):
        self.rows, self.h2d = 0, 0


def measure(configs, run, n_items, counter, reps):
    """configs: [(name, kwargs)].  One warm pass each, then ``reps`` interleaved rounds."""
    times = {name: [] for name, _ in configs}
    stats = {}
    for name, kw in configs:
        counter.reset()
        run(**kw)
        torch.cuda.synchronize()
        stats[name] = (counter.rows / n_items, counter.h2d / n_items)
    for _ in range(reps):
        for name, kw in configs:
            torch.cuda.synchronize()
            t = time.perf_counter()
            run(**kw)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t)
    return [(name, n_items / float(np.median(times[name])), [n_items / x for x in times[name]], stats[name][0], stats[name][1]) for name, _ in configs]


def report(title, unit, rows, lines):
    lines.append(title)
    lines.append("  %-34s %12s %10s %14s %16s   %s" % ("configuration", unit + "/s", "vs off", "rows/" + unit, "H2D bytes/" + unit, "every round"))
    base = rows[0][1]
    for name, rate, all_rates, r, h in rows:
        lines.append("  %-34s %12.1f %10.3f %14.1f %16.0f   %s" % (name, rate, rate / base, r, h, " ".join("%.1f" % x for x in all_rates)))
    lines.append("")


def device_path(dev, iters=20):
    """The device path on a padded GQA batch of 256 (text 8..30, regions 10..45): per forward cpt_batch_extents + the 8-byte read-back +
    cpt_trim_batch; beside it cpt_pad_cast (fp32 -> fp32, K = 2054 -> 2112) over the same B x Li' feature rows, the project's yardstick for a
    row copy.  Host-clock figures here; kernel times come from the rocprofv3 run this mode is meant for."""
    m = model(dev)
    eng = m._engine()
    eng.ensure_packed()
    qs = gqa_questions(256, 8)
    ids = torch.stack([q["input_ids"] for q in qs]).to(dev)
    seg = torch.stack([q["segment_ids"] for q in qs]).to(dev)
    mask = torch.stack([q["input_mask"] for q in qs]).to(dev)
    feats = torch.stack([q["img_feats"] for q in qs]).to(dev)
    mpos = torch.tensor([q["mask_token_pos"][0] for q in qs]).to(dev)
    out = eng._trim_batch(ids, seg, mask, None, feats, mpos)
    lt2, li2 = out[0].size(1), out[4].size(1)
    dst = torch.empty((256 * li2, 2112), device=dev, dtype=torch.float32)
    src = out[4].contiguous()
    st = L.stream_ptr()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        eng._trim_batch(ids, seg, mask, None, feats, mpos)
    torch.cuda.synchronize()
    t_trim = (time.perf_counter() - t) / iters * 1e6
    t = time.perf_counter()
    for _ in range(iters):
        L.check(L.lib().cpt_pad_cast(src.data_ptr(), dst.data_ptr(), L.CPT_F32, 256 * li2, D, 2112, st), "cpt_pad_cast")
    torch.cuda.synchronize()
    t_pad = (time.perf_counter() - t) / iters * 1e6
    moved = 256 * li2 * D * 4 * 2 + 256 * (3 * lt2 + li2) * 8 * 2
    print("device path, B = 256, 165 + 45 -> %d + %d: extents + read-back + trim %.1f us per forward (host clock, allocation of the trimmed tensors "
          "included); trim moves %.1f MB (read + write)" % (lt2, li2, t_trim, moved / 1e6))
    print("yardstick cpt_pad_cast fp32 on the same %d x %d rows: %.1f us per call (host clock, back to back)" % (256 * li2, D, t_pad))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gqa", type=int, default=768)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--device-path", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.device_path:
        device_path(dev)
        return
    m = model(dev)
    lines = ["eval_trim_bench: Oscar-base, bf16, one GPU; median of %d interleaved rounds after one warm pass per configuration" % a.reps, ""]
    n_labels = 1853
    rng = np.random.Generator(np.random.PCG64(0))
    labels = ["%d x%d" % (int(t), i) for i, t in enumerate(rng.integers(1000, 30000, n_labels))]
    tok = IdTokenizer()
    qs = gqa_questions(a.gqa, n_labels)
    counter = Counter(m, (165, 45))
    gqa_cfgs = [("off", {})] if a.plain else [("off", {}), ("trim", dict(trim=True)), ("trim + bucket", dict(trim=True, bucket=True))]
    rows = measure(gqa_cfgs, lambda **kw: drivers.val_gqa(m, qs, labels, tok, dev, **kw), len(qs), counter, a.reps)
    report("val_gqa: %d questions, padded 165 + 45, text 8..30, regions 10..45, 256 per batch, %d label columns" % (len(qs), n_labels), "question", rows,
           lines)
    del qs
    queries = refcoco_queries(a.queries, m.config)
    n_seq = sum(q["input_ids"].size(0) for q in queries)
    counter.padded = (70, 50)
    q_cfgs = [("off (4 queries per batch)", {})]
    if not a.plain:
        q_cfgs += [("trim", dict(trim=True)), ("trim + bucket", dict(trim=True, bucket=True)),
                   ("trim + bucket + max_sequences=64", dict(trim=True, bucket=True, max_sequences=64))]
    rows = measure(q_cfgs, lambda **kw: drivers.val_queries(m, queries, synth.NONE_ID, dev, **kw), len(queries), counter, a.reps)
    report("val_queries: %d queries (%d sequences), padded 70 + 50, 4..40 proposals per query, 36 regions" % (len(queries), n_seq), "query", rows, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
