"""GPU: the attention kernels across the sequence-length regimes of their dispatch tables (csrc/attention.hip att_dispatch,
csrc/bwd.hip attention_bwd / attention_bwd_x3), row by row against float64.

The kernels choose by L: every choice is a template instantiation with its own padded key count LP = 32 NKB, LDS layout and register
budget.  The lengths below sit on every block edge, one past it, and inside every range that leaves whole 32-key blocks of LP empty.

1. cpt_attention (fp32, bf16), with and without saved probabilities (the LEAN = 0 and LEAN = 1 instantiations; ctx bit-identical);
2. cpt_attention_bwd (fp32, bf16, bf16x3), p in {0, 0.1} with the mask cpt_dropout_mask exports, per-key and 3-D masks;
3. the training step (REC_MLM_CPT forward + loss.backward()) on two small models across the same lengths through tests/_gradcheck.py:
   the HAVE backward kernels, the phase split, the forward's dropout and statistics export, the fused QKV + attention launch.

Every case holds three sequences: all keys kept; a ragged tail plus a hole over one aligned 32-key block (key 0 where L < 64); every
key masked (the reference adds -10000 and excludes nothing: the plain softmax of the raw scores).  Outputs carry 64 guard rows of
0xFF bytes (NaN in both number formats: a row the kernel never wrote is as visible as a guard row it did write), inputs 64 rows of NaN.

Rows: every 64-wide (tensor, sequence, head, position) slice of ctx / dqkv and every probability row is compared on its own,
||got - ref||2 / ||ref||2 and max|got - ref| / max|ref|; rows whose reference is exactly zero (K / V gradients of masked keys) are held
absolutely, ||got||2 <= 1e-6 (bf16: 1e-3) x the largest reference row norm of that tensor.

Bounds.  fp32 / bf16x3: the whole-tensor bounds of test_gpu_ops.py / test_gpu_bwd_ops.py (FIXED below), now per row.  bf16:
rel_kernel <= C rel_emulation + FLOOR per row (tests/_gradcheck.py), the emulation being `restate("bf16")`: float64 that rounds to bf16
where the kernels do (attn_core.h, bwd.hip attn_bwd_mfma_kernel; oracle.cpt_oracle `_lp`): the (dropped) probabilities before P V and
P^T dO, dS before dS K and dS^T Q, and the outputs.  tests/test_attn_lengths_cpu.py checks that emulation without a GPU.

One exception to FIXED, in fp32: rows of queries ALL of whose keys are masked (the all-masked sequence; query 0 under a 3-D mask when
key 0 is masked) and the K / V rows of their sequences.  Scores of about -10000 carry the fp32 spacing of that magnitude, 2^-10, so a
CORRECT fp32 kernel (and the reference model in fp32) is off by up to 5e-4 in every score.  Measured per row on the MI355X (the
`degenerate` lines of the log): ctx 4.7e-4, probabilities 3.7e-4, dqkv 4.3e-4 with a per-key mask and 1.06e-3 with a 3-D one (L = 33,
key 0 of the sequence whose query 0 sees nothing), against 2e-5 / 1e-5 / 2e-4 -- and each equal to three digits to the figure of
`restate("f32")`, the same arithmetic in float32 torch on the CPU.  Those rows are held to max(FIXED, 2 x the worst such row of that
restatement), not to anything the kernel produced.  bf16x3 has the same spacing in its scores but stays inside its 1e-3 (worst row
5.1e-4, worst element 8.7e-4): no exception there.

The worst row per (mode, kernel instantiation) of an MI355X run, with its index and bound: profiles/attn_lengths_rows.log (written
when CPT_ATTN_ROWS_LOG names a file).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _gradcheck as G
from cpt_amd import config as cfgmod
from cpt_amd import synth
from oracle import cpt_oracle as O

pytestmark = pytest.mark.gpu

SEED = 0x5EED5EED1234
GUARD = 64
ERR_SHAPE = -1                                          # CPT_ERR_SHAPE (include/cpt_hip.h)
LENGTHS = [1, 2, 31, 32, 33, 64, 65, 96, 97, 127, 128, 129, 160, 161, 192, 193, 224, 225, 256, 257, 287, 288]
LONG = [289, 320]                                       # attention_long_kernel: inference only, no probabilities
# 3-D masks go through the generic backward kernel: ME = 32 up to 128; ME = 44 while its accumulators (44 x 256 elements = 176 keys) and
# 160 KB of LDS hold both tiles -- (195 L + 4224) floats without dropout: L <= 188, (227 L + 4256) with: L <= 161; beyond, V from global
LENGTHS_3D = [31, 33, 128, 129, 161, 162, 176, 177, 188, 189, 224, 288]
FIXED = {("fp32", "ctx"): 2e-5, ("fp32", "probs"): 1e-5, ("fp32", "dqkv"): 2e-4, ("bf16x3", "dqkv"): 1e-3}
ZERO_ABS = {"fp32": 1e-6, "bf16x3": 1e-6, "bf16": 1e-3}
KINDS = {3: (0, 1, 2), 2: (1, 2)}                       # mask kind per sequence: 0 all kept, 1 ragged tail + hole, 2 all masked


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch.device("cuda:0")
    _write_log()


# ---- inputs ------------------------------------------------------------------------------------------------------------------------

def key_mask(B, L):
    m = torch.ones(B, L, dtype=torch.int64)
    for b, kind in enumerate(KINDS[B]):
        if kind == 1:
            if L // 4:
                m[b, L - L // 4:] = 0
            if L >= 64:
                m[b, 32:64] = 0
            else:
                m[b, 0] = 0
        elif kind == 2:
            m[b] = 0
    return m


def make_case(L, B=3, heads=3, lp=False, mask3=False, seed=0):
    """qkv [B L][3 H], dctx [B L][H] (float32 values, already rounded to bf16 when lp), the int64 mask ([B][L] or [B][L][L]) and its
    additive float64 form [B][1][1 | L][L]."""
    g = torch.Generator().manual_seed(1000 * L + 10 * heads + seed)
    H = heads * 64
    qkv = torch.randn(B * L, 3 * H, generator=g)
    dctx = torch.randn(B * L, H, generator=g)
    if lp:
        qkv, dctx = qkv.bfloat16().float(), dctx.bfloat16().float()
    mask = key_mask(B, L)
    if mask3:
        mask = torch.tril(torch.ones(L, L, dtype=torch.int64))[None] * mask[:, None, :]
    madd = (1.0 - mask.double()) * -10000.0
    madd = madd[:, None, :, :] if mask3 else madd[:, None, None, :]
    return qkv, dctx, mask.contiguous(), madd


# ---- float64 reference, and its restatements -----------------------------------------------------------------------------------------

def _split(x, B, L, heads):
    x = x.view(B, L, -1, heads, 64)
    return tuple(x[:, :, i].permute(0, 2, 1, 3) for i in range(x.size(2)))


def _merge(t, B, L, heads):
    return t.permute(0, 2, 1, 3).reshape(B * L, heads * 64)


def reference(qkv, madd, dctx, w, B, L, heads):
    """float64, torch.autograd with qkv as the leaf.  w: the dropout multipliers [B][heads][L][L] (0 or 1 / (1 - p)) or None.
    -> ctx [B L][H], probs [B][heads][L][L], dqkv [B L][3 H] (None without dctx)."""
    leaf = qkv.double().clone().requires_grad_(True)
    q, k, v = _split(leaf, B, L, heads)
    s = q @ k.transpose(-1, -2) / 8.0 + madd
    p = torch.softmax(s, -1)
    ctx = _merge((p if w is None else p * w.double()) @ v, B, L, heads)
    if dctx is not None:
        ctx.backward(dctx.double())
    return ctx.detach(), p.detach(), leaf.grad


def restate(kind, qkv, madd, dctx, w, B, L, heads):
    """The same operation with the backward written out, as
    "exact": float64, nothing rounded (equals `reference`: the check of this function itself);
    "bf16":  float64 with the bf16 design's roundings: the (dropped) probabilities, dS, and the outputs ctx / probs / dqkv;
    "f32":   float32 throughout (the mask added to the scores in float32);
    "x3":    float32 with every product as hi.hi + hi.lo + lo.hi of the operands' bf16 halves."""
    dt = torch.float64 if kind in ("exact", "bf16") else torch.float32
    rnd = (lambda x: x.bfloat16().to(dt)) if kind == "bf16" else (lambda x: x)

    def halves(a):
        hi = a.bfloat16().float()
        return hi, (a - hi).bfloat16().float()

    def mm(a, b):
        if kind != "x3":
            return a @ b
        (ah, al), (bh, bl) = halves(a), halves(b)
        return ah @ bh + ah @ bl + al @ bh
    q, k, v = _split(qkv.to(dt), B, L, heads)
    s = mm(q, k.transpose(-1, -2)) * 0.125 + madd.to(dt)
    p = torch.softmax(s, -1)
    wd = None if w is None else w.to(dt)
    pd = rnd(p if wd is None else p * wd)
    out = {"ctx": _merge(rnd(mm(pd, v)), B, L, heads), "probs": rnd(p)}
    if dctx is not None:
        do, = _split(dctx.to(dt), B, L, heads)
        dv = mm(pd.transpose(-1, -2), do)
        dp = mm(do, v.transpose(-1, -2))
        if wd is not None:
            dp = dp * wd
        ds = rnd(p * (dp - (dp * p).sum(-1, keepdim=True)))
        dq, dk = mm(ds, k) * 0.125, mm(ds.transpose(-1, -2), q) * 0.125
        out["dqkv"] = rnd(torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B * L, 3 * heads * 64))
    return {n: t.double() for n, t in out.items()}


# ---- per-row comparison ----------------------------------------------------------------------------------------------------------

def rows_of(name, x, B, L, heads):
    """-> [T][B][heads][L][n]: T = 1 (ctx, probs) or 3 (dqkv: Q, K, V)."""
    x = x.double()
    if name == "probs":
        return x.reshape(1, B, heads, L, L)
    return x.reshape(B, L, -1, heads, 64).permute(2, 0, 3, 1, 4)


def row_errors(got, ref):
    """Per row: (||got - ref||2 / ||ref||2, max|got - ref| / max|ref|); rows with a zero reference: nan."""
    d = got - ref
    rn, rm = ref.norm(dim=-1), ref.abs().amax(-1)
    nan = torch.full_like(rn, float("nan"))
    return torch.where(rn > 0, d.norm(dim=-1) / rn, nan), torch.where(rm > 0, d.abs().amax(-1) / rm, nan)


def row_flags(name, madd, B, L, heads):
    """[T][B][heads][L] bool: the rows that see a query whose keys are all masked (module docstring)."""
    dq = (madd != 0).all(-1)[:, 0]                                     # [B][1 | L]
    dq = dq.expand(B, L)
    per_row = dq[:, None, :].expand(B, heads, L)
    if name != "dqkv":
        return per_row[None]
    per_seq = dq.any(-1)[:, None, None].expand(B, heads, L)
    return torch.stack([per_row, per_seq, per_seq], 0)


_LOG = {}


def _note(inst, mode, line, ratio):
    key = (mode, inst)
    if key not in _LOG or ratio > _LOG[key][0]:
        _LOG[key] = (ratio, line)


def _write_log():
    path = os.environ.get("CPT_ATTN_ROWS_LOG")
    if not path or not _LOG:
        return
    with open(path, "a") as f:
        for (mode, inst), (ratio, line) in sorted(_LOG.items()):
            f.write("%-7s %-44s error / bound %.3f | %s\n" % (mode, inst, ratio, line))


def check_rows(what, name, mode, inst, got, ref, low, madd, B, L, heads):
    """All rows of one output tensor.  low: the restatement the bound is formed from ("bf16" emulation in bf16; "f32" / "x3" elsewhere)."""
    g, r, e = (rows_of(name, t, B, L, heads) for t in (got, ref, low))
    assert torch.isfinite(g).all(), "%s %s: non-finite output" % (what, name)
    flags = row_flags(name, madd, B, L, heads)
    (k2, ke), (e2, ee) = row_errors(g, r), row_errors(e, r)
    zero = r.norm(dim=-1) == 0
    bad, worst = [], (-1.0, "")
    for T in range(g.size(0)):
        if mode == "bf16":
            b2, be = G.C * e2[T] + G.FLOOR, G.C * ee[T] + G.FLOOR
        else:
            fx = FIXED[(mode, name)]
            deg = flags[T] & ~zero[T] & (mode == "fp32")
            wide2 = max(fx, 2 * float(e2[T][deg].max())) if deg.any() else fx
            widee = max(fx, 2 * float(ee[T][deg].max())) if deg.any() else fx
            b2 = torch.where(flags[T], torch.full_like(e2[T], wide2), torch.full_like(e2[T], fx))
            be = torch.where(flags[T], torch.full_like(e2[T], widee), torch.full_like(e2[T], fx))
        top = float(r.norm(dim=-1).max())                  # (dqkv is one tensor: at L = 1 its Q and K thirds are zero altogether)
        zerr = g[T].norm(dim=-1) / max(top, 1e-300) / ZERO_ABS[mode]                   # <= 1 where the reference row is zero
        ratio = torch.where(zero[T], zerr, torch.maximum(k2[T] / b2, ke[T] / be))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        for sel, tag in ((~flags[T], ""), (flags[T], " degenerate")):
            if not sel.any():
                continue
            rr = torch.where(sel, ratio, torch.full_like(ratio, -1.0))
            i = int(rr.argmax())
            b_, h_, q_ = np.unravel_index(i, rr.shape)
            tname = name if g.size(0) == 1 else "d" + "QKV"[T]
            if zero[T][b_, h_, q_]:
                line = "%s%s L=%d row (seq %d, head %d, pos %d): zero reference, ||got|| / top %.3e, bound %.1e" % (
                    tname, tag, L, b_, h_, q_, float(g[T][b_, h_, q_].norm()) / max(top, 1e-300), ZERO_ABS[mode])
            else:
                line = "%s%s L=%d row (seq %d, head %d, pos %d): rel %.3e (bound %.3e), elem %.3e (bound %.3e), restated %.3e / %.3e" % (
                    tname, tag, L, b_, h_, q_, float(k2[T][b_, h_, q_]), float(b2[b_, h_, q_]), float(ke[T][b_, h_, q_]),
                    float(be[b_, h_, q_]), float(e2[T][b_, h_, q_]), float(ee[T][b_, h_, q_]))
            v = float(rr.flatten()[i])
            _note(inst + tag, mode, line, v)
            if v > worst[0]:
                worst = (v, line)
            if v > 1.0:
                bad.append(line + "  [%d rows of this tensor outside]" % int((rr > 1.0).sum()))
    print("%s [%s] worst: %s" % (what, inst, worst[1]))
    return bad


# ---- the kernels through the C ABI, with guard rows -----------------------------------------------------------------------------------

def _guarded(rows, cols, dtype, dev):
    item = torch.empty((), dtype=dtype).element_size()
    buf = torch.full(((rows + GUARD) * cols * item,), 0xFF, dtype=torch.uint8, device=dev)
    return buf, buf.view(dtype).view(rows + GUARD, cols), rows * cols * item


def _guard_intact(buf, used):
    return bool((buf[used:] == 0xFF).all())


def _with_nan_rows(x, dtype, dev):
    t = torch.full((x.size(0) + GUARD, x.size(1)), float("nan"), dtype=dtype)
    t[:x.size(0)] = x.to(dtype)
    return t.to(dev)


def run_forward(dev, mode, qkv, mask, B, L, heads, want_probs):
    """-> (return code, ctx [B L][H], probs or None); asserts the guard rows."""
    from cpt_amd import _lib as Lb
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    q_d, m_d = _with_nan_rows(qkv, dt, dev), mask.to(dev)
    cbuf, ctx, cused = _guarded(B * L, heads * 64, dt, dev)
    pbuf = probs = None
    if want_probs:
        pbuf, probs, pused = _guarded(B * heads * L, L, dt, dev)
    rc = Lb.lib().cpt_attention(Lb.CPT_BF16 if mode == "bf16" else Lb.CPT_F32, q_d.data_ptr(), m_d.data_ptr(), ctx.data_ptr(),
                                probs.data_ptr() if want_probs else None, B, L, heads, Lb.stream_ptr())
    torch.cuda.synchronize()
    assert _guard_intact(cbuf, cused), "ctx guard rows written"
    if want_probs:
        assert _guard_intact(pbuf, pused), "probs guard rows written"
    return rc, ctx[:B * L].cpu(), probs[:B * heads * L].cpu().view(B, heads, L, L) if want_probs else None


def export_keep(dev, p, step, site, n0, L):
    from cpt_amd import _lib as Lb
    d = Lb.Dropout(p_hidden=p, p_attn=p, seed=SEED, step=step)
    out = torch.empty((n0, L, L), dtype=torch.uint8, device=dev)
    Lb.check(Lb.lib().cpt_dropout_mask(C.byref(d), site, 1, out.data_ptr(), n0, L, L, Lb.stream_ptr()), "cpt_dropout_mask")
    return out.cpu()


def run_backward(dev, mode, qkv, dctx, mask, mask3, B, L, heads, p, step, site):
    """-> (return code, dqkv [B L][3 H], dbias [3 H]); asserts the guard rows."""
    from cpt_amd import _lib as Lb
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    q_d, d_d, m_d = _with_nan_rows(qkv, dt, dev), _with_nan_rows(dctx, dt, dev), mask.to(dev)
    gbuf, dq, used = _guarded(B * L, 3 * heads * 64, dt, dev)
    db = torch.zeros(3 * heads * 64, dtype=torch.float32, device=dev)
    dr = Lb.Dropout(p_hidden=p, p_attn=p, seed=SEED, step=step)
    code = {"fp32": Lb.CPT_F32, "bf16": Lb.CPT_BF16, "bf16x3": Lb.CPT_BF16X3}[mode]
    rc = Lb.lib().cpt_attention_bwd(code, q_d.data_ptr(), m_d.data_ptr(), 1 if mask3 else 0, d_d.data_ptr(), dq.data_ptr(), db.data_ptr(), B, L, heads,
                                    C.byref(dr) if p > 0 else None, site, Lb.stream_ptr())
    torch.cuda.synchronize()
    assert _guard_intact(gbuf, used), "dqkv guard rows written"
    return rc, dq[:B * L].cpu(), db.cpu()


# ---- which instantiation a case runs (the dispatch tables, for the log) -----------------------------------------------------------------

def forward_inst(L, lean):
    if L > 288:
        return "attention_long_kernel"
    nkb = 1 if L <= 32 else 4 if L <= 128 else 7 if L <= 224 else 9
    return "attention_kernel<NKB=%d, LEAN=%d>" % (nkb, lean)


def generic_form(L, drop):
    """attention_bwd's choice among the generic kernel's forms (module comment at LENGTHS_3D)."""
    if L <= 128:
        return "ME=32"
    floats = 2 * L * 65 + 2 * 32 * 65 + (3 if drop else 2) * 32 * (L + 1) + L
    return "ME=44" if floats * 4 <= 160 * 1024 and L <= 176 else "V from global"


def backward_inst(mode, L, drop, mask3):
    if mode == "bf16x3":
        n = next(n for n in (1, 2, 3, 4, 5, 7, 9) if L <= 32 * n)
        return "attn_bwd_x3_%skernel<%d>" % ("long_" if n > 4 else "", n)
    if mode == "bf16" and not mask3:
        n = next(n for n in (1, 2, 4, 5, 7, 9) if L <= 32 * n)
        return "attn_bwd_mfma_kernel<%d%s>" % (n, ", TR" if L > 64 else "")
    return "attn_bwd_kernel<%s, %s>%s" % (mode, generic_form(L, drop), " 3-D mask" if mask3 else "")


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------------

_FWD_CASES = [(L, 3, 3) for L in LENGTHS + LONG] + [(129, 2, 8), (257, 2, 8)]       # heads = 8, B = 2: B heads a multiple of 8 (no padded groups)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("L,B,heads", _FWD_CASES, ids=["L%d-B%d-h%d" % c for c in _FWD_CASES])
def test_forward_rows(dev, L, B, heads, mode):
    """ctx (and the probabilities up to L = 288) row by row; the lean and the full instantiation give the same ctx bits.  B heads = 9 pads
    the remapped grid of L >= 129 to 16 groups."""
    qkv, _, mask, madd = make_case(L, B, heads, lp=mode == "bf16")
    ref_ctx, ref_p, _ = reference(qkv, madd, None, None, B, L, heads)
    low = restate("bf16" if mode == "bf16" else "f32", qkv, madd, None, None, B, L, heads)
    what = "forward %s L=%d B=%d heads=%d" % (mode, L, B, heads)
    rc, ctx_lean, _ = run_forward(dev, mode, qkv, mask, B, L, heads, False)
    assert rc == 0, rc
    bad = check_rows(what, "ctx", mode, forward_inst(L, 1), ctx_lean, ref_ctx, low["ctx"], madd, B, L, heads)
    if L <= 288:
        rc, ctx_full, probs = run_forward(dev, mode, qkv, mask, B, L, heads, True)
        assert rc == 0, rc
        assert torch.equal(ctx_full.view(torch.uint8), ctx_lean.view(torch.uint8)), "ctx differs between want_probs on and off"
        bad += check_rows(what, "ctx", mode, forward_inst(L, 0), ctx_full, ref_ctx, low["ctx"], madd, B, L, heads)
        bad += check_rows(what, "probs", mode, forward_inst(L, 0), probs, ref_p, low["probs"], madd, B, L, heads)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_forward_refuses_probabilities_beyond_288(dev, mode):
    qkv, _, mask, _ = make_case(289, lp=mode == "bf16")
    rc, _, _ = run_forward(dev, mode, qkv, mask, 3, 289, 3, True)
    assert rc == ERR_SHAPE


# ---- 2. backward -----------------------------------------------------------------------------------------------------------------------

_REF = {}


def _backward_case(dev, L, lp, mask3, p, B=3, heads=3):
    """Inputs, exported dropout multipliers and the float64 reference of one (L, input rounding, mask form, p): shared by the modes."""
    key = (L, lp, mask3, p)
    if key not in _REF:
        _REF.clear()                                                   # (parametrised with `mode` innermost: one entry is all that is reused)
        qkv, dctx, mask, madd = make_case(L, B, heads, lp=lp, mask3=mask3)
        step, site = 3, 13
        w = None
        if p > 0:
            _, sa = O.dropout_thresh_scale(p, True)
            w = export_keep(dev, p, step, site, B * heads, L).view(B, heads, L, L).float() * float(np.float32(sa))
        _, _, ref = reference(qkv, madd, dctx, w, B, L, heads)
        _REF[key] = (qkv, dctx, mask, madd, w, step, site, ref)
    return _REF[key]


def _check_backward(dev, mode, L, p, mask3):
    B, heads = 3, 3
    H = heads * 64
    qkv, dctx, mask, madd, w, step, site, ref = _backward_case(dev, L, mode == "bf16", mask3, p)
    low = restate({"fp32": "f32", "bf16": "bf16", "bf16x3": "x3"}[mode], qkv, madd, dctx, w, B, L, heads)["dqkv"]
    rc, dqkv, dbias = run_backward(dev, mode, qkv, dctx, mask, mask3, B, L, heads, p, step, site)
    assert rc == 0, rc
    what = "backward %s L=%d p=%g%s" % (mode, L, p, " 3-D" if mask3 else "")
    inst = backward_inst(mode, L, p > 0, mask3)
    bad = check_rows(what, "dqkv", mode, inst, dqkv, ref, low, madd, B, L, heads)
    # dbias_qkv = column sums.  The K third is zero in exact arithmetic (rows of dS sum to zero): it is held against the column sums of
    # |dK|, the size of what cancels.
    assert torch.isfinite(dbias).all()
    rs, ls, gs = ref.sum(0), low.sum(0), dbias.double()
    for t, nm in enumerate("QKV"):
        sl = slice(t * H, (t + 1) * H)
        scale = float(ref[:, sl].abs().sum(0).norm()) if nm == "K" else float(rs[sl].norm())
        if scale == 0:                                     # L = 1: dS = 0, the Q and K thirds are exactly zero -> the absolute rule, against the V third
            err = float(gs[sl].norm()) / float(rs[2 * H:].norm())
            print("%s dbias %s: zero reference, ||got|| / ||dV sums|| %.3e (bound %.1e)" % (what, nm, err, ZERO_ABS[mode]))
            if not err <= ZERO_ABS[mode]:
                bad.append("dbias %s: zero reference, %.3e > %.1e" % (nm, err, ZERO_ABS[mode]))
            continue
        err, emu = float((gs[sl] - rs[sl]).norm()) / scale, float((ls[sl] - rs[sl]).norm()) / scale
        deg = bool((madd != 0).all(-1).any())
        bound = G.C * emu + G.FLOOR if mode == "bf16" else (max(FIXED[(mode, "dqkv")], 2 * emu) if deg and mode == "fp32" else FIXED[(mode, "dqkv")])
        print("%s dbias %s: rel %.3e (bound %.3e, restated %.3e)" % (what, nm, err, bound, emu))
        if not err <= bound:
            bad.append("dbias %s: rel %.3e > %.3e" % (nm, err, bound))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("L", LENGTHS)
def test_backward_rows(dev, L, p, mode):
    _check_backward(dev, mode, L, p, False)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("L", LENGTHS_3D)
def test_backward_rows_3d_mask(dev, L, p, mode):
    """A lower-triangular [B][L][L] mask times the per-key mask: the generic kernel's ME = 32, ME = 44 and V-from-global forms, on each side
    of each switch (LDS with dropout 161 | 162; the ME = 44 accumulators 176 | 177; LDS without dropout 188 | 189)."""
    _check_backward(dev, mode, L, p, True)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
def test_backward_refuses_289(dev, mode):
    qkv, dctx, mask, _ = make_case(289, lp=mode == "bf16")
    for p in (0.0, 0.1):
        rc, _, _ = run_backward(dev, mode, qkv, dctx, mask, False, 3, 289, 3, p, 3, 13)
        assert rc == ERR_SHAPE, (p, rc)


def test_backward_x3_refuses_3d_mask(dev):
    qkv, dctx, mask, _ = make_case(33, mask3=True)
    rc, _, _ = run_backward(dev, "bf16x3", qkv, dctx, mask, True, 3, 33, 3, 0.0, 3, 13)
    assert rc == ERR_SHAPE


# ---- 3. the training step ----------------------------------------------------------------------------------------------------------

TRAIN_LENGTHS = [32, 33, 64, 65, 128, 129, 160, 161, 224, 225, 288]
P = 0.1


@pytest.fixture(scope="module")
def models(dev):
    cfgs = {"tiny": lambda: cfgmod.tiny(max_position_embeddings=192), "base": lambda: cfgmod.oscar_base(num_hidden_layers=2)}
    cache = {}

    def get(name, mode):
        from cpt_amd.modeling_rec import REC_MLM_CPT
        if name not in cache:
            sd = synth.init_state_dict(cfgs[name](), 1234, head="cpt")
            sd64 = {k: v.to(dev, torch.float64) for k, v in sd.items()}
            sd64["cls.decoder.weight"] = sd64["bert.embeddings.word_embeddings.weight"]
            cache[name] = (sd, sd64, {})
        sd, sd64, ms = cache[name]
        if mode not in ms:
            m = REC_MLM_CPT(cfgs[name]())
            m.load_state_dict(sd)
            m.tie_weights()
            m.to(dev).train()
            m.set_compute_dtype(mode)
            ms[mode] = m
        return ms[mode], sd64
    return get


def _train(dev, models, name, mode, L, B, mask3=False):
    from cpt_amd.train import set_dropout_seed
    from test_gpu_dropout import SEED as STEP_SEED, _drop_dict
    m, sd64 = models(name, mode)
    cfg = m.config
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = P
    set_dropout_seed(m, STEP_SEED, step=0)
    for prm in m.parameters():
        prm.grad = None
    Li = max(4, L // 3)
    Lt = L - Li
    b = synth.make_batch(B, cfg, seed=2000 + L + B, max_seq_len=Lt, img_seq_len=Li, vary_regions=True)
    d = {k: v.to(dev) for k, v in b.items()}
    lab = None
    if mask3:
        d["attention_mask"] = torch.tril(torch.ones(L, L, dtype=torch.long, device=dev))[None] * d["attention_mask"][:, None, :]
        lab = torch.full((B, L), -1, dtype=torch.long, device=dev)
        lab[torch.arange(B), d["mask_token_pos"]] = d["colors"]
        loss, scores = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], masked_lm_labels=lab)
    else:
        loss, scores = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], masked_lm_labels=d["colors"],
                         mask_token_pos=d["mask_token_pos"])
    loss.backward()
    torch.cuda.synchronize()
    got = {n: prm.grad for n, prm in m.named_parameters()}
    got["loss"], got["scores"] = loss.detach().reshape(1), scores.detach()
    drop = {k: v.to(dev) for k, v in _drop_dict(dev, cfg, P, 1, B, L).items()}       # first training forward -> step 1
    d64 = dict(d, img_feats=d["img_feats"].double())

    def oracle(bf16):
        loss_r, grads, sc = O.train_step_grads(sd64, cfg.to_dict(), d64, drop=drop, labels=lab, bf16=bf16, with_scores=True)
        grads["loss"], grads["scores"] = loss_r.reshape(1), sc
        return grads
    ref = oracle(False)
    emu = oracle(True) if mode == "bf16" else None
    what = "step %s %s L=%d+%d B=%d%s" % (name, mode, Lt, Li, B, " 3-D mask" if mask3 else "")
    rows = G.check(mode, got, ref, emu, what)
    w = max((r for r in rows if r["cls"] != "key bias"), key=lambda r: r["rel"] / r["bound"])
    line = "L=%d B=%d worst %s: rel %.3e (bound %.3e, emulation %.3e)" % (L, B, w["name"], w["rel"], w["bound"], w["emu"])
    print(what, line)
    _note("training step, %s%s" % (name, " 3-D mask" if mask3 else ""), mode, line, w["rel"] / w["bound"])


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("L", TRAIN_LENGTHS)
def test_step_tiny(dev, models, L, mode):
    """Two heads, two layers: the fused forward's one-workgroup-per-head form; every compute mode at every length."""
    _train(dev, models, "tiny", mode, L, 3)


_BASE = [("bf16", L, 2) for L in TRAIN_LENGTHS] + [("bf16", 128, 11), ("bf16", 129, 11)] + \
        [(m, L, 2) for m in ("fp32", "bf16x3") for L in (65, 161, 288)]


@pytest.mark.parametrize("mode,L,B", _BASE, ids=["%s-L%d-B%d" % c for c in _BASE])
def test_step_base_width(dev, models, mode, L, B):
    """Oscar-base width, two layers: three heads per workgroup in the fused forward; the backward's phase split holds at B = 2
    (2 B heads = 48 <= 256) and not at B = 11 (264)."""
    _train(dev, models, "base", mode, L, B)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("L", [33, 129, 225])
def test_step_tiny_3d_mask(dev, models, L, mode):
    _train(dev, models, "tiny", mode, L, 3, mask3=True)
