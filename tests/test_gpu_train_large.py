"""GPU: the NSP-CPT half of the training step -- NSPCPT (pooler, tanh, seq_relationship) and the two-head VCR Q->AR step (VCRQAR_NSPCPT:
cpt_train_fwd_rel2 / cpt_train_bwd_rel2, rel2_fwd / rel2_bwd) -- against the float64 oracle on the device (oracle.cpt_oracle.nsp_step_grads),
at Oscar-large width (hidden 1024, 16 heads, intermediate 4096: the VCR few-shot workload) and, for the pruned last layer under the NSP head,
at Oscar-base width.

Two layers (width, not depth, is what is new here).  Each case is one step with dropout 0.1 and the masks the library exports
(tests/test_gpu_dropout.py); the loss, the relation scores and EVERY parameter gradient go through tests/_gradcheck.py with its constants as
they stand: fixed bounds in fp32 / bf16x3, ``rel_kernel <= C * rel_emulation + FLOOR`` in bf16 against the oracle's bf16 design emulation.
``trim_padding`` stays False and each case asserts the shape the step ran on, so the row counts are the stated ones.

What hidden 1024 changes in csrc/train.hip::make_train_plan and the launchers: no `tail` (H % 192 != 0), no triple launch and no deferred
Q|K|V partials (weight gradients through gemm_tn_pair on 128 x 128 tiles), gemm_nn on its 128-row instantiations only (the GELU-gradient
epilogue with the partial-row bias sums included), ln_bwd / layernorm_rows_ex with four values per lane and the dropout keep bits at their
stated limit H <= 1024, the attention backward's phase split (2 B heads <= 256) ending at B = 8, a head count that is no multiple of 3.

No kernel fix was needed: every case is inside the bounds.  Worst kernel-to-emulation gradient ratio of this sweep: 1.5 (layer 1's query bias,
NSPCPT bf16, B = 8, L = 165 + 100, dropout 0.1; C = 2.5), most cases' worst sits at 1.1..1.4; fp32 stays below 3e-6 and bf16x3 below 2e-5 of their
fixed 2e-4 / 5e-4; the key biases hold at most 2e-5 (bf16, bound 1e-3), so the comparator's absolute rule stands here without an exception.
"""
import time

import pytest
import torch

import _gradcheck as G
from cpt_amd import config as cfgmod
from cpt_amd import synth
from oracle import cpt_oracle as O
from test_gpu_dropout import SEED, _drop_dict

pytestmark = pytest.mark.gpu
P = 0.1
WSEED = 1234
QAR_HEADS = (("cls_ans.weight", "cls_ans.bias"), ("cls_rat.weight", "cls_rat.bias"))
NSP_HEADS = (("cls.weight", "cls.bias"),)
FIXED_ORDER = ("cls_ans.weight", "cls_ans.bias", "cls_rat.weight", "cls_rat.bias", "bert.pooler.dense.weight")


def _cfg(width):
    return cfgmod.oscar_large(num_hidden_layers=2) if width == "large" else cfgmod.oscar_base(num_hidden_layers=2)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    weights, models, sd64s = {}, {}, {}

    def model(width, kind, mode):
        """(model, its float64 state on the device): NSPCPT / VCRQAR_NSPCPT as the drivers build them from the pre-training model, one per
        (width, kind, mode); cls_rat moved off cls_ans by a seeded offset as in tests/test_gpu_vcr_qar.py::_model."""
        from cpt_amd.modeling_bert import BertImgForPreTraining
        from cpt_amd.modeling_vcr import NSPCPT, VCRQAR_NSPCPT
        key = (width, kind, mode)
        if key not in models:
            cfg = _cfg(width)
            if width not in weights:
                weights[width] = synth.init_state_dict(cfg, WSEED, head="pretrain")
            pre = BertImgForPreTraining(cfg)
            pre.load_state_dict(weights[width])
            pre.tie_weights()
            m = (NSPCPT if kind == "nsp" else VCRQAR_NSPCPT)(cfg)
            m.copy_from_pretraining_model(pre)
            if kind == "qar":
                g = torch.Generator().manual_seed(WSEED + 1)
                with torch.no_grad():
                    m.cls_rat.weight.add_(torch.randn(m.cls_rat.weight.shape, generator=g) * 0.05)
                    m.cls_rat.bias.add_(torch.randn(m.cls_rat.bias.shape, generator=g) * 0.05)
            m.to(dev).train()
            m.set_compute_dtype(mode)
            assert m.trim_padding is False and not getattr(m, "trim_training", False)
            models[key] = m
            if (width, kind) not in sd64s:
                sd64s[(width, kind)] = {k: v.detach().to(dev, torch.float64) for k, v in m.state_dict().items()}
        return models[key], sd64s[(width, kind)]
    return dev, model


def _labels(lo, hi, B, n_rel):
    """Labels of one head block: they cycle over [0, n_rel); from B >= 3 the block's second row is ignored (-1) when it has one."""
    lab = [(i - lo) % n_rel for i in range(lo, hi)]
    if B >= 3 and hi - lo >= 2:
        lab[1] = -1
    return lab


def _run(env, width, kind, mode, B, Lt, Li, vary, p=P, B0=None, head=None, repeat=False):
    """One step of `kind` ("nsp": NSPCPT; "qar": VCRQAR_NSPCPT through qar_forward, or through forward(head=...) when `head` is given)
    against the oracle.  vary: make_batch's vary_regions (ragged region counts).  B0: rows [0, B0) are the Q->A block."""
    dev, model = env
    m, sd64 = model(width, kind, mode)
    cfg = m.config
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = p
    n_rel = m.num_seq_relations
    b = synth.make_batch(B, cfg, seed=1000 + B, max_seq_len=Lt, img_seq_len=Li, vary_regions=vary)
    d = {k: v.to(dev) for k, v in b.items()}
    if kind == "qar":
        B0 = {"ans": B, "rat": 0}[head] if head else B0
        lab = _labels(0, B0, B, n_rel) + _labels(B0, B, B, n_rel)
    else:
        lab = _labels(0, B, B, n_rel)
    lab = torch.tensor(lab, dtype=torch.long, device=dev)
    assert all(int((blk != -1).sum()) >= 1 for blk in ((lab[:B0], lab[B0:]) if kind == "qar" else (lab,)) if blk.numel())
    from cpt_amd.train import set_dropout_seed

    def step():
        set_dropout_seed(m, SEED, step=0)
        for prm in m.parameters():
            prm.grad = None
        if kind == "nsp":
            loss, rel = m(d["input_ids"], d["segment_ids"], d["attention_mask"], next_sentence_label=lab, img_feats=d["img_feats"])
        elif head:
            loss, rel = m(d["input_ids"], d["segment_ids"], d["attention_mask"], next_sentence_label=lab, img_feats=d["img_feats"], head=head)
        else:
            blk = lambda lo, hi: {"input_ids": d["input_ids"][lo:hi], "token_type_ids": d["segment_ids"][lo:hi],
                                  "attention_mask": d["attention_mask"][lo:hi], "img_feats": d["img_feats"][lo:hi]}
            loss, ra, rr = m.qar_forward(blk(0, B0), blk(B0, B), lab[:B0], lab[B0:])
            rel = torch.cat([ra, rr], 0)
        loss.backward()
        assert m._engine().last_train_shape == (B, Lt, Li)
        got = {n: (prm.grad.clone() if prm.grad is not None else None) for n, prm in m.named_parameters()}
        got["loss"], got["scores"] = loss.detach().reshape(1).clone(), rel.detach().clone()
        return got
    t0 = time.time()
    got = step()
    torch.cuda.synchronize()
    t1 = time.time()
    drop = None
    if p > 0:
        drop = {k: v.to(dev) for k, v in _drop_dict(dev, cfg, p, 1, B, Lt + Li).items()}      # first training forward -> step 1
    d64 = dict(d, img_feats=d["img_feats"].double())
    cd = cfg.to_dict()

    def oracle(bf16):
        loss_r, grads, rel_r = O.nsp_step_grads(sd64, cd, d64, lab, drop=drop, bf16=bf16, B0=B0 if kind == "qar" else None,
                                                heads=QAR_HEADS if kind == "qar" else NSP_HEADS)
        grads["loss"], grads["scores"] = loss_r.reshape(1), rel_r
        return grads
    ref = oracle(False)
    emu = oracle(True) if mode == "bf16" else None
    torch.cuda.synchronize()
    t2 = time.time()
    what = "%s %s %s B=%d%s L=%d+%d (%d rows)%s p=%g" % (width, kind if not head else "qar.forward(head=%s)" % head, mode, B,
                                                       "" if B0 is None else " B0=%d" % B0, Lt, Li, B * (Lt + Li), " ragged" if vary else "", p)
    rows = G.compare(mode, got, ref, emu)
    grads = [r for r in rows if r["cls"] not in ("loss", "scores", "key bias")]
    w = max(grads, key=lambda r: G.ratio(r) if emu else r["rel"])
    kb = max((r["rel"] for r in rows if r["cls"] == "key bias"), default=0.0)
    print("\n%s: step %.1f ms, oracle %.2f s; worst gradient %s %.3g (%s); key bias max |g| %.3g" % (
        what, 1e3 * (t1 - t0), t2 - t1, "ratio" if emu else "rel", G.ratio(w) if emu else w["rel"], w["name"], kb))
    print(G.table(rows))
    G.check(mode, got, ref, emu, what)
    if repeat:
        # the same step twice: bit-identical loss and head / pooler gradients (fixed-order sums, no float atomics), as the tiny test promises
        again = step()
        assert torch.equal(again["loss"], got["loss"]), (float(again["loss"]), float(got["loss"]))
        for n in FIXED_ORDER:
            assert torch.equal(again[n], got[n]), n
    return rows


# (B, Lt, Li, p, vary_regions -- alternating from case to case, here and below) -> what it is there for
NSP_BF16 = [
    (8, 165, 100, P, False),    # 2120 rows: the benchmark's VCR step; lean LayerNorm on (>= 2048); Mp = 2176 with 8 real rows in the last K-tile, ragged last
                                # 128-row tile (72 rows); the 257..288 attention kernels; pair launches at 512 and 256 workgroups
    (1, 165, 100, P, True),     # 265: Bp = 64 with one real row for the pooler / relation weight gradients; below the lean threshold
    (8, 96, 32, P, False),      # 1024, L = 128: the backward phase split exactly at 2 B heads = 256; the fused QKV + attention forward with 16 heads
    (9, 96, 32, P, True),       # 1152: the first B with the phase split off
    (16, 97, 32, P, False),     # 2064: just over 2048 rows, L one past a 32-key block edge
    (8, 165, 100, 0.0, True),   # the dropout-free kernels
]


@pytest.mark.parametrize("B,Lt,Li,p,vary", NSP_BF16, ids=["B%d-L%d+%d-p%g" % c[:4] for c in NSP_BF16])
def test_nspcpt_large_bf16(env, B, Lt, Li, p, vary):
    _run(env, "large", "nsp", "bf16", B, Lt, Li, vary, p=p)


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("B,Lt,Li,vary", [(2, 165, 100, False), (8, 96, 32, True)], ids=["B2-L165+100", "B8-L96+32"])
def test_nspcpt_large_parity_modes(env, mode, B, Lt, Li, vary):
    _run(env, "large", "nsp", mode, B, Lt, Li, vary)          # FIXED bounds 2e-4 / 5e-4


@pytest.mark.parametrize("B", [4, 32])
def test_nspcpt_base_bf16(env, B):
    """Oscar-base under the NSP head: B = 4 runs `tail` (the pruned last layer on the [CLS] rows, RowMap{pos = NULL}), B = 32 (3840 rows) the
    triple weight-gradient launch with the deferred Q|K|V partials."""
    _run(env, "base", "nsp", "bf16", B, 70, 50, B == 32)


# (mode, n_q, n_ans, n_rats, Lt, Li, vary_regions): B0 = n_q n_ans, B = n_q (n_ans + n_rats)
QAR = [
    ("bf16", 2, 4, 4, 165, 100, False),     # 8 / 16, 4240 rows
    ("bf16", 1, 4, 16, 96, 32, True),       # 4 / 20, 2560 rows
    ("fp32", 1, 4, 4, 96, 32, False),       # 4 / 8, 1024 rows
]


@pytest.mark.parametrize("mode,n_q,n_ans,n_rats,Lt,Li,vary", QAR, ids=["%s-%dx(%d+%d)-L%d+%d" % c[:6] for c in QAR])
def test_qar_large(env, mode, n_q, n_ans, n_rats, Lt, Li, vary):
    _run(env, "large", "qar", mode, n_q * (n_ans + n_rats), Lt, Li, vary, B0=n_q * n_ans, repeat=mode == "bf16")


@pytest.mark.parametrize("head", ["ans", "rat"])
def test_qar_large_single_head_forward(env, head):
    """forward(head=...) trains through the two-head kernel with B0 = B / B0 = 0: an empty block on one side."""
    _run(env, "large", "qar", "bf16", 4, 96, 32, head == "rat", head=head, repeat=True)
