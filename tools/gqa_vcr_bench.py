"""GQA-CPT and VCR Q->A driver timing on one GPU (bf16, L = 165 + 45): drivers.val_gqa (Oscar-base, 1853 answer labels, 256 questions per
step) and drivers.val_vcr (Oscar-large, 8 questions x 4 choices per step) end to end, and the training step at 4 sequences per GPU with the
device clip (FusedAdamW.clip_grad_norm_device, cpt_grad_clip) against the same step with torch.nn.utils.clip_grad_norm_ over the gradient views,
alternated in the same process; kernel launches per step (torch.profiler).

    python tools/gqa_vcr_bench.py [--iters 50] [--json out.json]"""
import argparse
import json
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
from cpt_amd.train import AdamW, WarmupLinearSchedule  # noqa: E402

LT, LI = 165, 45


class IdTokenizer(object):
    """Labels are written "<id> ..." here: the first piece of a label is its first word, its vocabulary id that number."""

    def tokenize(self, s):
        return s.split()

    def convert_tokens_to_ids(self, toks):
        return [int(t) if t.isdigit() else 100 for t in toks]


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e3


def launches(fn):
    from torch.profiler import profile, ProfilerActivity
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as p:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in p.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def model(cls, cfg, dev):
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
    pre = BertImgForPreTraining(cfg)
    pre.load_state_dict(synth.init_state_dict(cfg, 1, head="pretrain"))
    pre.tie_weights()
    m = cls(cfg)
    m.copy_from_pretraining_model(pre)
    m.to(dev).set_compute_dtype("bf16")
    return m


def clip_ab(m, loss_fn, iters, out, tag):
    """The training step with either clip, alternated five times: medians, launches."""
    opt = AdamW(m, lr=1e-5, eps=1e-6, weight_decay=0.01)

    def step(device_clip):
        loss_fn().backward()
        if device_clip:
            opt.clip_grad_norm_device(1.0)
        else:
            torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        m.zero_grad()
    td, tt = [], []
    for _ in range(5):
        td.append(timed(lambda: step(True), iters))
        tt.append(timed(lambda: step(False), iters))
    out[tag] = {"device_clip_ms": float(np.median(td)), "torch_clip_ms": float(np.median(tt)), "device_clip_ms_all": td, "torch_clip_ms_all": tt,
                "launches_device_clip": launches(lambda: step(True)), "launches_torch_clip": launches(lambda: step(False))}
    print("%s train step, 4 sequences: device clip %.3f ms (%d launches), torch clip %.3f ms (%d launches), ratio %.3f"
          % (tag, out[tag]["device_clip_ms"], out[tag]["launches_device_clip"], out[tag]["torch_clip_ms"], out[tag]["launches_torch_clip"],
             out[tag]["device_clip_ms"] / out[tag]["torch_clip_ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    rng = np.random.Generator(np.random.PCG64(0))
    # ---- GQA-CPT: Oscar-base, 1853 labels ----
    cfg = cfgmod.oscar_base()
    m = model(REC_MLM_CPT, cfg, dev).eval()
    n_labels = 1853
    labels = ["%d x%d" % (int(t), i) for i, t in enumerate(rng.integers(1000, 30000, n_labels))]
    tok = IdTokenizer()
    qs = []
    for i in range(2):
        b = synth.make_batch(256, cfg, seed=20 + i, max_seq_len=LT, img_seq_len=LI)
        for j in range(256):
            qs.append({"input_ids": b["input_ids"][j], "segment_ids": b["segment_ids"][j], "input_mask": b["attention_mask"][j],
                       "img_feats": b["img_feats"][j], "mask_token_pos": [int(b["mask_token_pos"][j])], "q_id": np.array([i * 256 + j]),
                       "igt": [int(x) for x in rng.integers(0, n_labels, 1 + j % 3)]})
    drivers.val_gqa(m, qs[:256], labels, tok, dev)
    torch.cuda.synchronize()
    t = time.perf_counter()
    drivers.val_gqa(m, qs, labels, tok, dev)
    torch.cuda.synchronize()
    out["val_gqa_questions_per_s"] = len(qs) / (time.perf_counter() - t)
    print("val_gqa: %.1f questions/s (%d questions, 256 per step, %d labels)" % (out["val_gqa_questions_per_s"], len(qs), n_labels))
    m.train()
    tb = {k: v.to(dev) for k, v in synth.make_batch(4, cfg, seed=5, max_seq_len=LT, img_seq_len=LI).items()}
    token_ids = torch.tensor([int(lb.split()[0]) for lb in labels], device=dev)
    grid = drivers.gqa_label_grid(tb["input_ids"], tb["attention_mask"], torch.tensor([3, 1, 4, 1]), token_ids)
    clip_ab(m, lambda: m(tb["input_ids"], tb["segment_ids"], tb["attention_mask"], img_feats=tb["img_feats"], masked_lm_labels=grid)[0], a.iters, out, "gqa")
    del m
    torch.cuda.empty_cache()
    # ---- VCR Q->A: Oscar-large, 4 choices ----
    cfg = cfgmod.oscar_large()
    m = model(NSPCPT, cfg, dev).eval()
    qs = []
    for i in range(64):
        b = synth.make_batch(4, cfg, seed=100 + i, max_seq_len=LT, img_seq_len=LI)
        qs.append({"input_ids": b["input_ids"].numpy(), "segment_ids": b["segment_ids"].numpy(), "input_mask": b["attention_mask"].numpy(),
                   "img_feats": b["img_feats"][0], "label": i % 4, "q_id": i})
    drivers.val_vcr(m, qs[:8], dev)
    torch.cuda.synchronize()
    t = time.perf_counter()
    drivers.val_vcr(m, qs, dev)
    torch.cuda.synchronize()
    out["val_vcr_questions_per_s"] = len(qs) / (time.perf_counter() - t)
    print("val_vcr: %.1f questions/s (%d questions of 4 choices, 8 per step)" % (out["val_vcr_questions_per_s"], len(qs)))
    m.train()
    blk, interval = drivers._vcr_block(qs[:1], dev)
    from cpt_amd import scoring as S
    cls_labels = S.nsp_choice_labels([2], interval, interval, dev)
    clip_ab(m, lambda: m(blk["input_ids"], blk["token_type_ids"], blk["attention_mask"], next_sentence_label=cls_labels, img_feats=blk["img_feats"])[0],
            a.iters, out, "vcr")
    # the whole driver pass, for the record: one window of 2 micro-steps
    opt = AdamW(m, lr=1e-5, eps=1e-6, weight_decay=0.01)
    sch = WarmupLinearSchedule(opt, warmup_steps=1, t_total=10 ** 6)
    opts = types.SimpleNamespace(gradient_accumulation_steps=2, max_grad_norm=1.0)
    out["train_vcr_batch_window_ms"] = timed(lambda: drivers.train_vcr_batch(m, opt, sch, [qs[:1], qs[1:2]], opts, dev), max(5, a.iters // 5))
    print("train_vcr_batch: %.3f ms per window of 2 micro-steps (host batch assembly included)" % out["train_vcr_batch_window_ms"])
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
