"""VCR Q->AR timing on one GPU (Oscar-base, bf16, L = 165 + 45): the evaluation step of 4 questions (16 + 16 sequences) as ONE encoder pass
(VCRQAR_NSPCPT.qar_forward) against the reference's two forward(head=...) passes, alternated in the same process; the training step at 1
question (4 + 4) per GPU; questions/s end to end through drivers.val_vcr_qar; and the kernel launches per step (torch.profiler).

    python tools/vcr_qar_bench.py [--iters 50]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cpt_amd import config as cfgmod, drivers, scoring as S, synth  # noqa: E402
from cpt_amd.modeling_bert import BertImgForPreTraining  # noqa: E402
from cpt_amd.modeling_vcr import VCRQAR_NSPCPT  # noqa: E402


def block(n, dev, seed):
    cfg = cfgmod.oscar_base()
    b = synth.make_batch(n, cfg, seed=seed, max_seq_len=165, img_seq_len=45)
    return {"input_ids": b["input_ids"].to(dev), "token_type_ids": b["segment_ids"].to(dev), "attention_mask": b["attention_mask"].to(dev),
            "img_feats": b["img_feats"].to(dev)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = cfgmod.oscar_base()
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
    pre = BertImgForPreTraining(cfg)
    pre.load_state_dict(synth.init_state_dict(cfg, 1, head="pretrain"))
    pre.tie_weights()
    m = VCRQAR_NSPCPT(cfg)
    m.copy_from_pretraining_model(pre)
    m.to(dev).eval().set_compute_dtype("bf16")
    qa, qr = block(16, dev, 1), block(16, dev, 2)

    def one_pass():
        with torch.no_grad():
            m.qar_forward(qa, qr, return_scores=True)

    def two_pass():
        with torch.no_grad():
            ra = m(qa["input_ids"], qa["token_type_ids"], qa["attention_mask"], img_feats=qa["img_feats"], head="ans")[0]
            rr = m(qr["input_ids"], qr["token_type_ids"], qr["attention_mask"], img_feats=qr["img_feats"], head="rat")[0]
            S.choice_scores(ra), S.choice_scores(rr)
    t1, t2 = [], []
    for _ in range(5):                 # alternated: clocks and caches treat both routes alike
        t1.append(timed(one_pass, a.iters))
        t2.append(timed(two_pass, a.iters))
    print("eval step, 4 questions (16 + 16 seq): one pass %.3f ms, two passes %.3f ms (median of 5), ratio %.2f"
          % (np.median(t1), np.median(t2), np.median(t1) / np.median(t2)))
    print("launches per eval step: one pass %d, two passes %d" % (launches(one_pass), launches(two_pass)))
    # training step, 1 question (4 + 4) per GPU
    from cpt_amd.train import AdamW
    m.train()
    opt = AdamW(m, lr=1e-5, eps=1e-6, weight_decay=0.01)
    ta, tr = block(4, dev, 3), block(4, dev, 4)
    la, lr = S.qar_choice_labels([1], [2], 4, 4)

    def train_step():
        loss = m.qar_forward(ta, tr, la, lr)[0]
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        m.zero_grad()
    print("train step, 1 question (4 + 4): %.3f ms, %d launches" % (timed(train_step, a.iters), launches(train_step)))
    m.eval()
    # end to end: val_vcr_qar over 64 questions
    rng = np.random.Generator(np.random.PCG64(0))
    qs = []
    for i in range(64):
        q = {"n_ans": 4, "n_rats": 4, "label": (i % 4, (i * 3) % 4), "q_id": i,
             "img_feats": torch.from_numpy(rng.standard_normal((45, cfg.img_feature_dim)).astype(np.float32))}
        for part, blk in (("q_a", block(4, "cpu", 10 + 2 * i)), ("qa_r", block(4, "cpu", 11 + 2 * i))):
            q[part] = {"input_ids": blk["input_ids"], "input_mask": blk["attention_mask"], "segment_ids": blk["token_type_ids"]}
        qs.append(q)
    drivers.val_vcr_qar(m, qs[:8], dev)
    torch.cuda.synchronize()
    t = time.perf_counter()
    drivers.val_vcr_qar(m, qs, dev)
    torch.cuda.synchronize()
    print("val_vcr_qar: %.1f questions/s (64 questions, 4 per step)" % (64 / (time.perf_counter() - t)))


if __name__ == "__main__":
    main()
