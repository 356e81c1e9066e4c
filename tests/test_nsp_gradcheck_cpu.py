"""CPU: the NSP-CPT / VCR Q->AR oracle (oracle.cpt_oracle.nsp_step_grads) and the bounds of tests/_gradcheck.py on it.

2-layer Oscar-large width (hidden 1024, 16 heads, intermediate 4096), B = 4 sequences of L = 24 + 8 in float64, two relation heads with the
block boundary at B0 = 2, dropout 0.1 with the masks of oracle.dropout_keep_*.  As in tests/test_gradcheck_cpu.py the "kernel" is the
oracle's bf16 design emulation with one injected fault of the kind a launch of the NSP half of the training step (csrc/train.hip: pooler,
tanh_bwd, rel2_fwd / rel2_bwd, the 128 x 128 weight-gradient tiles and the 128-row data-gradient tiles of this width) can make; the comparator,
with C and FLOOR as the GPU sweep (tests/test_gpu_train_large.py) uses them, must accept the plain emulation and reject every fault on the
tensor it hits.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gradcheck as G
from cpt_amd import config as cfgmod
from cpt_amd import synth
from oracle import cpt_oracle as O

SEED = 0x5EEDC0FFEE123457
P = 0.1
B, B0, LT, LI, LAYERS = 4, 2, 24, 8, 2
L = LT + LI
HEADS = (("cls_ans.weight", "cls_ans.bias"), ("cls_rat.weight", "cls_rat.bias"))
LABELS = [0, -1, 2, 1]          # one ignored row; each block keeps a labelled row, also with the boundary one row off


def _masks(cfg):
    """The multipliers of tests/test_gpu_dropout.py::_drop_dict (first training forward: step 1), from the CPU restatement."""
    H, nh = cfg.hidden_size, cfg.num_attention_heads
    sh = float(np.float32(O.dropout_thresh_scale(P, False)[1]))
    sa = float(np.float32(O.dropout_thresh_scale(P, True)[1]))

    def hid(site):
        return torch.from_numpy(O.dropout_keep_hidden(SEED, 1, site, B * L, H, P)).view(B, L, H).double() * sh
    drop = {"emb": hid(0)}
    for i in range(LAYERS):
        drop[("attn", i)] = torch.from_numpy(O.dropout_keep_attn(SEED, 1, 1 + 3 * i, B * nh, L, P)).view(B, nh, L, L).double() * sa
        drop[("ao", i)] = hid(2 + 3 * i)
        drop[("out", i)] = hid(3 + 3 * i)
    return drop


@pytest.fixture(scope="module")
def case():
    cfg = cfgmod.oscar_large(num_hidden_layers=LAYERS)
    sd = {k: v.double() for k, v in synth.init_state_dict(cfg, 1234, head="qar").items()}
    b = synth.make_batch(B, cfg, seed=5, max_seq_len=LT, img_seq_len=LI, vary_regions=True)
    b["img_feats"] = b["img_feats"].double()
    labels = torch.tensor(LABELS)
    drop = _masks(cfg)
    cd = cfg.to_dict()

    def run(bf16=True, b0=B0, p=P):
        loss, grads, rel = O.nsp_step_grads(sd, cd, b, labels, drop=drop if p > 0 else None, bf16=bf16, B0=b0, heads=HEADS)
        return dict(grads, loss=loss.reshape(1), scores=rel)
    return dict(cfg=cfg, cd=cd, sd=sd, batch=b, labels=labels, run=run, ref=run(bf16=False), emu=run())


def test_two_heads_equal_two_separate_forwards(case):
    """p = 0: one pass with the boundary at B0 is the sum of one nsp_cpt_forward per block (the encoder is batch-invariant in float64)."""
    sd, b, labels = case["sd"], case["batch"], case["labels"]
    got = case["run"](bf16=False, p=0.0)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    loss, rels = 0, []
    for (lo, hi), (wk, bk) in zip(((0, B0), (B0, B)), HEADS):
        lo_, rel = O.nsp_cpt_forward(leaves, case["cd"], b["input_ids"][lo:hi], b["segment_ids"][lo:hi], b["attention_mask"][lo:hi],
                                     b["img_feats"][lo:hi], labels[lo:hi], wk, bk)
        loss = loss + lo_
        rels.append(rel)
    loss.backward()
    assert abs(float(got["loss"]) - float(loss.detach())) <= 1e-12
    assert float((got["scores"] - torch.cat(rels, 0).detach()).abs().max()) <= 1e-12
    for k, v in leaves.items():
        assert v.grad is not None, k
        assert G.rel(got[k], v.grad) <= 1e-12 or float((got[k] - v.grad).abs().max()) <= 1e-15, k      # (key bias: zero on both sides)
    # and the single-head form is nsp_cpt_forward on the whole batch
    one = O.nsp_step_grads(sd, case["cd"], b, labels, heads=(HEADS[0],))
    ref_loss, ref_rel = O.nsp_cpt_forward(sd, case["cd"], b["input_ids"], b["segment_ids"], b["attention_mask"], b["img_feats"], labels, *HEADS[0])
    assert abs(float(one[0]) - float(ref_loss)) <= 1e-12 and float((one[2] - ref_rel).abs().max()) <= 1e-12
    assert one[1]["cls_rat.weight"] is None and one[1]["cls_ans.weight"] is not None       # outside the graph -> None


# ---- the faults: each replaces one function the oracle calls for the duration of one run ---------------------------------------------

class _Linear(torch.autograd.Function):
    """F.linear whose backward leaves rows of the weight gradient unwritten (orows) or drops contraction columns of the data gradient (dcols)."""

    @staticmethod
    def forward(ctx, x, w, b, orows, dcols):
        ctx.save_for_backward(x, w)
        ctx.orows, ctx.dcols = orows, dcols
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g2, x2 = g.reshape(-1, g.size(-1)), x.reshape(-1, x.size(-1))
        gd = g2.clone()
        if ctx.dcols is not None:
            gd[:, ctx.dcols] = 0
        gw = g2.t() @ x2
        if ctx.orows is not None:
            gw[ctx.orows] = 0
        return (gd @ w).view(x.shape), gw, g2.sum(0), None, None


def _fault_linear(key, orows=None, dcols=None):
    def lin(x, sd, k):
        if k != key:
            return F.linear(O._lp(x), O._lp(sd[k + ".weight"]), sd[k + ".bias"])
        return _Linear.apply(O._lp(x), O._lp(sd[k + ".weight"]), sd[k + ".bias"], orows, dcols)
    return O, "_linear", lin


def _fault_count_ignored():
    """The block mean divides by the block's rows, the ignored one included."""
    def loss(rel, labels):
        return F.cross_entropy(rel.view(-1, rel.size(-1)), labels.view(-1), ignore_index=-1, reduction="sum") / labels.numel()
    return O, "relation_loss", loss


class _ShiftGrad(torch.autograd.Function):
    """Identity whose gradient arrives one position later in the sequence."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.roll(1, 1)


def _fault_cls_scatter():
    """The pooler's data gradient (the only gradient of the last layer's output: the [CLS] rows) lands on position 1."""
    orig = O.encoder_layer

    def layer(sd, cfg, x, ext_mask, i, prefix="bert.", drop=None):
        y = orig(sd, cfg, x, ext_mask, i, prefix, drop)
        return _ShiftGrad.apply(y) if i == LAYERS - 1 else y
    return O, "encoder_layer", layer


class _Tanh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = _TANH(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        return g * (1 - ctx.saved_tensors[0])          # 1 - y, not 1 - y^2


_TANH = torch.tanh


def _fault_tanh():
    return torch, "tanh", _Tanh.apply          # (the oracle calls torch.tanh at one place, the pooler)


def _faults(cfg):
    H, I = cfg.hidden_size, cfg.intermediate_size
    p1 = "bert.encoder.layer.1."
    p0 = "bert.encoder.layer.0."
    # what -> (the run's keyword arguments, the patch, the tensor it must be caught on)
    return {
        "block boundary one row off: row B0 through head 0": (dict(b0=B0 + 1), None, "cls_ans.weight"),
        "ignored row counted in the block mean's denominator": ({}, _fault_count_ignored(), "cls_ans.weight"),
        "pooler data gradient scattered to position 1 instead of [CLS]": ({}, _fault_cls_scatter(), p1 + "output.dense.weight"),
        "tanh backward with 1 - y": ({}, _fault_tanh(), "bert.pooler.dense.weight"),
        # (B L = 128 rows are ONE contraction block here; the block that can go missing alone is a row of 128 x 128 output tiles)
        "one 128-row block of output tiles missing from wgrad(ffn down), layer 0": ({}, _fault_linear(p0 + "output.dense", orows=slice(H - 256, H - 128)),
                                                                                    p0 + "output.dense.weight"),
        "last 128 columns missing from dgrad(ffn up), layer 1": ({}, _fault_linear(p1 + "intermediate.dense", dcols=slice(I - 128, I)),
                                                                 p1 + "attention.output.LayerNorm.weight"),
    }


def test_comparator_accepts_the_emulation(case):
    G.check("bf16", case["emu"], case["ref"], case["emu"], "plain emulation")
    rows = G.compare("bf16", case["emu"], case["ref"], case["emu"])
    print("\n" + G.table(rows))
    # the emulation is a real yardstick: bf16 rounding is visible in every weight gradient, the relation heads' and the pooler's included
    mats = [r for r in rows if r["cls"] == "matrix"]
    assert {"cls_ans.weight", "cls_rat.weight", "bert.pooler.dense.weight"} <= {r["name"] for r in mats}
    assert all(r["emu"] > 1e-3 for r in mats), [(r["name"], r["emu"]) for r in mats if r["emu"] <= 1e-3]
    assert G.group("bert.pooler.dense.weight") == "head" and G.group("bert.img_embedding.weight") == "embeddings"


def test_comparator_rejects_every_fault(case, monkeypatch):
    report = []
    faults = _faults(case["cfg"])
    assert len(faults) == 6
    for what, (kw, patch, target) in faults.items():
        with monkeypatch.context() as mp:
            if patch is not None:
                mp.setattr(*patch)
            got = case["run"](**kw)
        rows = {r["name"]: r for r in G.compare("bf16", got, case["ref"], case["emu"])}
        r = rows[target]
        report.append("%-80s %-50s rel %.3e  rel(emu) %.3e  bound %.3e" % (what, target, r["rel"], r["emu"], r["bound"]))
        assert not r["ok"], "not caught: " + report[-1]
        with pytest.raises(AssertionError):
            G.check("bf16", got, case["ref"], case["emu"], what)
    assert torch.tanh is _TANH
    print("\n" + "\n".join(report))
