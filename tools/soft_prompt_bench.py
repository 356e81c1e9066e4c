"""Frozen soft-template step against the full training step of the same build, interleaved in one process.

Oscar-base, bf16, dropout 0.1: 32 and 4 sequences of L = 70 + 50, and 4 sequences at the GQA length (165 + 45).  For each shape the two
steps alternate (full, frozen, full, frozen, ...) so that clock and thermal drift hit both; step time is the median over the timed rounds
of one forward + backward + optimizer step (full: FusedAdamW over the flat buffer; frozen: torch.optim.AdamW over the template), launch
count comes from the torch profiler's kernel events of one step.  Writes profiles/soft_prompt_bench.txt.

    python tools/soft_prompt_bench.py [--rounds 20] [--warmup 5]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cpt_amd import config as cfgmod  # noqa: E402
from cpt_amd import soft_prompt, synth  # noqa: E402
from cpt_amd.modeling_rec import REC_MLM_CPT  # noqa: E402
from cpt_amd.train import FusedAdamW  # noqa: E402

SHAPES = [("32 x (70 + 50)", 32, 70, 50), ("4 x (70 + 50)", 4, 70, 50), ("4 x (165 + 45), GQA length", 4, 165, 45)]


def build(dev, frozen):
    cfg = cfgmod.oscar_base()
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.1
    m = REC_MLM_CPT(cfg)
    m.load_state_dict(synth.init_state_dict(cfg, 1234, head="cpt"))
    m.tie_weights()
    m.to(dev).train()
    m.set_compute_dtype("bf16")
    if frozen:
        w = soft_prompt.attach(m)
        return m, torch.optim.AdamW([w], lr=0.02, eps=1e-8)
    return m, FusedAdamW(m, lr=5e-5)


def batch(cfg, B, Lt, Li, dev):
    import _softcheck as S
    b = S.plant_slots(synth.make_batch(B, cfg, seed=7, max_seq_len=Lt, img_seq_len=Li))
    # the prompt of the reference: twenty slot ids in a row behind [CLS] would overwrite the synthetic text; three per sequence are enough
    # to exercise the gather and the per-slot sum
    return {k: v.to(dev) for k, v in b.items()}


def step(m, opt, d):
    opt.zero_grad()
    loss = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], masked_lm_labels=d["colors"],
             mask_token_pos=d["mask_token_pos"])[0]
    loss.backward()
    opt.step()


def timed(m, opt, d):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    step(m, opt, d)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launches(m, opt, d):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step(m, opt, d)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_prompt_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    full, fopt = build(dev, False)
    froz, zopt = build(dev, True)
    lines = ["soft-template frozen step vs full step: Oscar-base bf16, dropout 0.1, %s, median of %d interleaved rounds (%d warm-up)"
             % (torch.cuda.get_device_name(0), args.rounds, args.warmup),
             "%-30s %12s %12s %8s %10s %10s" % ("shape", "full ms", "frozen ms", "ratio", "full knl", "frozen knl")]
    for name, B, Lt, Li in SHAPES:
        d = batch(full.config, B, Lt, Li, dev)
        tf, tz = [], []
        for r in range(args.warmup + args.rounds):
            a, b = timed(full, fopt, d), timed(froz, zopt, d)
            if r >= args.warmup:
                tf.append(a)
                tz.append(b)
        mf, mz = statistics.median(tf), statistics.median(tz)
        try:
            kf, kz = launches(full, fopt, d), launches(froz, zopt, d)
        except Exception as e:      # the launch count is a side figure: a profiler that cannot run leaves it out
            print("launch count unavailable:", str(e)[:120])
            kf = kz = -1
        lines.append("%-30s %12.3f %12.3f %8.3f %10d %10d" % (name, mf, mz, mz / mf, kf, kz))
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
