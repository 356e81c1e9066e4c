"""CPU: the bounds of tests/_gradcheck.py bite.

The "kernel" here is the oracle's bf16 design emulation with one injected fault of the kind a training launch can make, run in float64
on a small Oscar-base shape (2 layers, B = 3, ragged regions, dropout 0.1 with the masks of oracle.dropout_keep_*).  The comparator,
with the C and FLOOR the GPU sweep (tests/test_gpu_train_regimes.py) uses, must accept the plain emulation and reject every fault on the
tensor it hits; at least two of the faults stay inside the 8e-2 band of the old norm-only test.
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
B, LT, LI, LAYERS = 3, 70, 50, 2
L = LT + LI


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


def _case():
    cfg = cfgmod.oscar_base(num_hidden_layers=LAYERS)
    sd = {k: v.double() for k, v in synth.init_state_dict(cfg, 1234, head="cpt").items()}
    sd["cls.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"]
    b = synth.make_batch(B, cfg, seed=5, vary_regions=True)
    b["img_feats"] = b["img_feats"].double()
    assert int(b["attention_mask"][:, LT:].sum(1).min()) < LI          # at least one sequence has padded region rows
    drop = _masks(cfg)
    cd = cfg.to_dict()

    def run(bf16=True):
        return O.train_step_grads(sd, cd, b, drop=drop, bf16=bf16)[1]
    return dict(cfg=cfg, batch=b, run=run, ref=run(bf16=False), emu=run())


@pytest.fixture(scope="module")
def case():
    return _case()


# ---- the faults: each replaces one oracle function for the duration of one run ------------------------------------------------------

class _Mul(torch.autograd.Function):
    """x * m on the way forward, g * m_bwd on the way back (a mask read from the wrong place by the backward only)."""

    @staticmethod
    def forward(ctx, x, m, m_bwd):
        ctx.save_for_backward(m_bwd)
        return x * m

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


class _Linear(torch.autograd.Function):
    """F.linear whose backward drops rows of the weight-gradient contraction (wrows) or contraction columns of the data gradient (dcols)."""

    @staticmethod
    def forward(ctx, x, w, b, wrows, dcols):
        ctx.save_for_backward(x, w)
        ctx.wrows, ctx.dcols = wrows, dcols
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g2, x2 = g.reshape(-1, g.size(-1)), x.reshape(-1, x.size(-1))
        gd = g2.clone()
        if ctx.dcols is not None:
            gd[:, ctx.dcols] = 0
        gw = g2.clone()
        if ctx.wrows is not None:
            gw[ctx.wrows] = 0
        return (gd @ w).view(x.shape), gw.t() @ x2, g2.sum(0), None, None


def _fault_linear(key, wrows=None, dcols=None):
    def lin(x, sd, k):
        if k != key:
            return F.linear(O._lp(x), O._lp(sd[k + ".weight"]), sd[k + ".bias"])
        return _Linear.apply(O._lp(x), O._lp(sd[k + ".weight"]), sd[k + ".bias"], wrows, dcols)
    return "_linear", lin


def _fault_drop_row(target, H):
    def drop_fn(x, drop, key):
        if drop is None or key not in drop:
            return x
        m = drop[key].to(device=x.device, dtype=x.dtype).view(x.shape)
        if key != target:
            return x * m
        return _Mul.apply(x, m, m.reshape(-1, H).roll(1, 0).view(x.shape))      # row r of the gradient takes row r - 1's keep bits
    return "_drop", drop_fn


def _fault_ln_rows(call, rows):
    """The call-th LayerNorm of the forward (0: text embeddings, 1: regions, 2 + 2 i / 3 + 2 i: layer i's attention / FFN side) gives no
    gain / shift gradient for `rows` (one partial-row block of the two-stage column sums missing); its output and data gradient are exact."""
    n = [0]
    orig = O.layer_norm

    def ln(x, w, b, eps):
        i = n[0]
        n[0] += 1
        if i != call:
            return orig(x, w, b, eps)
        sel = torch.zeros(x.shape[:-1] + (1,), dtype=torch.bool)
        sel.view(-1)[rows] = True
        return orig(x, torch.where(sel, w.detach(), w), torch.where(sel, b.detach(), b), eps)
    return "layer_norm", ln


def _fault_unmask_key(layer, seq, key):
    """Layer `layer`'s attention treats padded key `key` of sequence `seq` as real in head 0."""
    orig = O.self_attention

    def attn(sd, cfg, x, ext_mask, p, drop=None, layer_=0):
        if layer_ == layer:
            ext_mask = ext_mask.expand(x.size(0), cfg["num_attention_heads"], 1, x.size(1)).clone()
            ext_mask[seq, 0, 0, key] = 0.0
        return orig(sd, cfg, x, ext_mask, p, drop, layer_)
    return "self_attention", attn


def _faults(case):
    H = case["cfg"].hidden_size
    am = case["batch"]["attention_mask"]
    seq = int(torch.nonzero(am[:, LT:].sum(1) < LI)[0])
    pad_key = LT + int(am[seq, LT:].sum())                         # that sequence's first padded region row
    blk = int(case["batch"]["mask_token_pos"][0]) // 4 * 4         # the 4-row block (one row per wave below 2048 rows) of sequence 0's [MASK] row
    p1 = "bert.encoder.layer.1."
    p0 = "bert.encoder.layer.0."
    # (fault, the tensor it must be caught on)
    return {
        "dropout mask one row off (layer 1, attention-output site)": (_fault_drop_row(("ao", 1), H), p1 + "attention.output.dense.weight"),
        "last 64-row block missing from wgrad(ffn up), layer 0": (_fault_linear(p0 + "intermediate.dense", wrows=slice(B * L - 64, B * L)),
                                                                 p0 + "intermediate.dense.weight"),
        "K-split partial 0 of dgrad(ffn up) without its last 64 columns, layer 1": (_fault_linear(p1 + "intermediate.dense", dcols=slice(1472, 1536)),
                                                                                   p1 + "attention.output.LayerNorm.weight"),
        "ln_bwd partial-row block missing from the FFN-side gain / shift, layer 0": (_fault_ln_rows(3, slice(blk, blk + 4)),
                                                                                    p0 + "output.LayerNorm.weight"),
        # (a padded row that is never a key has no gradient; used as one it sends gradient into the region projection's bias)
        "padded region key unmasked in one attention block, layer 0": (_fault_unmask_key(0, seq, pad_key), "bert.img_embedding.bias"),
    }


def test_comparator_accepts_the_emulation(case):
    G.check("bf16", case["emu"], case["ref"], case["emu"], "plain emulation")
    # and the emulation is a real yardstick: bf16 rounding is visible in every weight gradient
    rows = G.compare("bf16", case["emu"], case["ref"], case["emu"])
    assert all(r["emu"] > 1e-3 for r in rows if r["cls"] == "matrix")


def test_comparator_rejects_every_fault(case, monkeypatch):
    inside_old_band = []
    report = []
    for what, ((attr, fn), target) in _faults(case).items():
        with monkeypatch.context() as mp:
            mp.setattr(O, attr, fn)
            got = case["run"]()
        rows = {r["name"]: r for r in G.compare("bf16", got, case["ref"], case["emu"])}
        r = rows[target]
        report.append("%-90s %-50s rel %.3e  rel(emu) %.3e  bound %.3e" % (what, target, r["rel"], r["emu"], r["bound"]))
        assert not r["ok"], "not caught: " + report[-1]
        with pytest.raises(AssertionError):
            G.check("bf16", got, case["ref"], case["emu"], what)
        if r["rel"] < G.OLD_BAND:
            inside_old_band.append(what)
    print("\n" + "\n".join(report))
    assert len(inside_old_band) >= 2, inside_old_band
