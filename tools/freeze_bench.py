"""Layer freezing on one GPU: the whole optimizer step (zero_grad, training forward, backward, FusedAdamW.step) with the first trainable
stage at 0 (the full step: the yardstick), 1 (embedding side frozen), 7 (layers 0..5 frozen too) and 13 (the head alone), Oscar-base, bf16,
dropout 0.1.

  RefCOCO  REC_MLM_CPT on synth.make_batch at 4 and at 32 sequences (70 + 50)
  GQA      REC_MLM_CPT at 4 sequences padded to 165 + 45

The stages are interleaved in one process on one card: per round every stage runs ``--steps`` optimizer steps, timed on the host clock
around a device synchronisation; ``--reps`` rounds after one warm round, the median round is reported.  One model, one optimizer per stage
(an optimizer that has stepped keeps its stage).  Also recorded: device-side profiler events of one step (torch.profiler: kernels, memsets
and copies, the library's and torch's) and the elements one AdamW launch covers.  No ratio is a pass condition.

  python tools/freeze_bench.py [--steps 16] [--reps 5] [--out profiles/freeze_bench.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpt_amd import config as cfgmod, synth, train  # noqa: E402
from cpt_amd.modeling_rec import REC_MLM_CPT  # noqa: E402

STAGES = (0, 1, 7, 13)
SHAPES = [("RefCOCO, 4 sequences, 70 + 50", 4, 70, 50), ("RefCOCO, 32 sequences, 70 + 50", 32, 70, 50), ("GQA, 4 sequences padded to 165 + 45", 4, 165, 45)]


def build(dev):
    cfg = cfgmod.oscar_base()
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.1
    m = REC_MLM_CPT(cfg)
    m.load_state_dict(synth.init_state_dict(cfg, 1, head="cpt"))
    m.tie_weights()
    m.to(dev).set_compute_dtype("bf16")
    return m.train(), cfg


def one_step(m, opt, d):
    opt.zero_grad()
    loss, _ = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], masked_lm_labels=d["colors"],
                mask_token_pos=d["mask_token_pos"])
    loss.backward()
    opt.step()


def set_stage(m, s):
    """Stage s through the public calls."""
    n = m.config.num_hidden_layers
    return train.unfreeze(m) if s == 0 else train.train_head_only(m) if s == n + 1 else train.freeze_layers(m, s - 1)


def device_events(m, opt, d):
    """Device-side profiler events of one optimizer step -- kernels, memsets and copies -- or None where this torch build's profiler
    cannot be imported or records no device activity.  A failing step raises as it would without the profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
    except ImportError:
        return None
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        one_step(m, opt, d)
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    return n or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m, cfg = build(dev)
    opts = {}
    for s in STAGES:          # one optimizer per stage, bound while the model is at that stage
        set_stage(m, s)
        opts[s] = train.FusedAdamW(m, lr=1e-6, weight_decay=0.05)
        opts[s].trainable_elements()          # (lays the optimizer out for this stage)
    lines = ["freeze_bench: Oscar-base, bf16, dropout 0.1, one GPU; stages %s interleaved, %d optimizer steps per round, median of %d rounds after "
             "one warm round; the whole optimizer step on the host clock" % (", ".join(map(str, STAGES)), a.steps, a.reps), ""]
    for title, B, lt, li in SHAPES:
        batches = [{k: v.to(dev) for k, v in synth.make_batch(B, cfg, seed=100 + i, max_seq_len=lt, img_seq_len=li, vary_regions=True).items()}
                   for i in range(a.steps)]
        times = {s: [] for s in STAGES}
        for rnd in range(a.reps + 1):
            for s in STAGES:
                set_stage(m, s)
                torch.cuda.synchronize()
                t = time.perf_counter()
                for d in batches:
                    one_step(m, opts[s], d)
                torch.cuda.synchronize()
                if rnd:
                    times[s].append((time.perf_counter() - t) / a.steps * 1e3)
        lines.append(title)
        lines.append("  %-6s %10s %8s %10s %14s   %s" % ("stage", "ms/step", "vs 0", "dev events", "AdamW elements", "every round (ms/step)"))
        base = float(np.median(times[0]))
        for s in STAGES:
            set_stage(m, s)
            n = device_events(m, opts[s], batches[0])
            lo, hi = opts[s].trainable_elements()
            ms = float(np.median(times[s]))
            lines.append("  %-6d %10.3f %8.3f %10s %14d   %s" % (s, ms, ms / base, "n/a" if n is None else str(n), hi - lo, " ".join("%.3f" % x for x in times[s])))
        lines.append("")
    train.unfreeze(m)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
