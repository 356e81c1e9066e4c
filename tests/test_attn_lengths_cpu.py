"""CPU: the references tests/test_gpu_attn_lengths.py holds the attention kernels to, checked without a GPU: the written-out backward
equals torch.autograd, and the bf16 emulation stays finite with a non-zero error in every row, at every length and mask of the lists."""
import pytest
import torch

import test_gpu_attn_lengths as T

B, HEADS = 3, 3


def _keep(L, p, seed):
    if p == 0:
        return None
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, HEADS, L, L, generator=g) >= p).float() / (1 - p)


@pytest.mark.parametrize("mask3,L", [(False, L) for L in T.LENGTHS] + [(True, L) for L in T.LENGTHS_3D])
def test_restatements(L, mask3):
    for p in (0.0, 0.1):
        qkv, dctx, _, madd = T.make_case(L, B, HEADS, lp=True, mask3=mask3)
        w = _keep(L, p, L)
        ctx, probs, dqkv = T.reference(qkv, madd, dctx, w, B, L, HEADS)
        ref = {"ctx": ctx, "probs": probs, "dqkv": dqkv}
        exact = T.restate("exact", qkv, madd, dctx, w, B, L, HEADS)
        emu = T.restate("bf16", qkv, madd, dctx, w, B, L, HEADS)
        for name in ("ctx", "probs", "dqkv"):
            r = T.rows_of(name, ref[name], B, L, HEADS)
            top = float(r.norm(dim=-1).max())
            assert float((T.rows_of(name, exact[name], B, L, HEADS) - r).norm(dim=-1).max()) <= 1e-12 * top, (name, p)
            if p > 0 and name == "probs":
                continue                                   # (the forward operator has no dropout: probabilities are compared at p = 0)
            e = T.rows_of(name, emu[name], B, L, HEADS)
            assert torch.isfinite(e).all()
            e2, ee = T.row_errors(e, r)
            live = r.norm(dim=-1) > 0
            # a query with a single visible key has the probability 1: its ctx row is a V row, its dV row a dctx row, both bf16 already
            one = (r == r.bfloat16().double()).all(-1)
            assert (e2[live & ~one] > 0).all() and (ee[live & ~one] > 0).all(), (name, p)
            assert float(e2[live].max()) < 0.1, (name, p)
            assert (e[~live] == 0).all()                   # masked keys: exactly zero gradients in the emulation as in the reference


def test_masks_hold_the_three_kinds():
    for L in T.LENGTHS:
        m = T.key_mask(3, L)
        assert m[0].all() and not m[2].any()
        assert not m[1, 32:64].any() if L >= 64 else m[1, 0] == 0
        assert L < 4 or m[1, -1] == 0
