"""float64 reference of the LayerNorm-folded GEMMs (gemm_ln_prod, gemm_ln_prod3, gemm_ln_cons, fold_ln_weights), an error bound
computed from the inputs alone, an fp32 emulation that shows the bound is achievable, and planted defects that show it is tight
enough.  Host-only helper of tests/test_ln_gemm_ref_cpu.py and tests/test_gpu_ln_gemm_parity.py; every function takes the
operands the kernels take (bf16 operands as their exact values) as torch tensors on any device and computes in float64.

The bound (per output element, U = 2^-24), never fitted to a kernel's output:
  accumulation      K * U * (|A| . |W|^T)                       worst-case fp32 chain over K
  added terms       4 * U * (|bias| + |R|)                       R = the residual as added (LayerNorm'ed or plain); consumer: |cold|, |pre|
  statistics        one-pass variance sq/H - mu^2: relative error C_VAR * U * (1 + mu^2 / var); the table's own fp32 summation H * U
                    (on var, and H * U * rms on mu; rms >= mean |x|); through rstd at half the relative error, through mu as is
  output format     half an ulp of the format at the reference value: bf16 keeps 8 significant bits, the 3-byte code 16.  Half an ulp is
                    2^-9 (2^-17) of the TOP of the value's binade, i.e. between 2^-9 and 2^-8 (2^-17 and 2^-16) of the value itself:
                    _half_ulp computes it exactly instead of taking either end
  GELU              |gelu'| <= 1.13 on the pre-activation's bound + 1e-6, the documented absolute error of the kernels' erf
                    approximation (csrc/common.h gelu_fast2)

C_VAR = 8.  It is calibrated on the fp32 emulation below (emulate_producer / emulate_consumer: per-block sums in index order,
ln_mean_rstd / ln_fold / ln_apply with their fma structure, accumulation over K in fp32), not on a kernel: the smallest power of two
for which the emulation stays within a quarter of the bound on every input family and shape class of tests/test_ln_gemm_ref_cpu.py
(1, 2, 4 give 0.82, 0.61, 0.41 on the |mean|/std = 64 family: the reader adds up to 12 slots and rounds sq/H and the difference, each
amplified by 1 + mu^2 / var = 4097).  "Within a quarter" is asked of the ESTIMATED terms: the format's half ulp is exact, a correctly
rounded result reaches it, so the figure is (error - half ulp)+ / (the other terms) (_ratio).  Worst figure per family with C_VAR = 8
(python tests/_lnref.py prints them):
  |mean|/std = 0        0.0973   (partial sums of a 96-column block against 96 * U * sum |x|)
  |mean|/std = 4        0.0919   (same)
  |mean|/std = 64       0.2433   (fp32 output of the LayerNorm-residual producer, N = 200, K = 64: the statistics term)
  four outliers at 30   0.1251   (partial sums)

A constant non-zero row is ill-conditioned for ANY fp32 LayerNorm (var = 0 up to rounding, rstd = 1 / sqrt(eps) amplifies the
rounding of the mean a million times): no bound from the inputs can hold there, and the families leave it out on purpose.  The
all-zero row is exact (mu = 0, every product 0) and is in every matrix.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
BLK = 96
C_VAR = 8.0
GELU_ABS = 1e-6
GELU_SLOPE = 1.13
FAIL = float("inf")


def parts(n):
    return (n + BLK - 1) // BLK


def slots(n):
    return (parts(n) + 1) & ~1


# ---- the 3-byte residual code (csrc/common.h r3_encode / r3_decode) --------------------------------------------------------------
def _r3_encode_np(x):
    """CPU restatement of the 3-byte residual code (csrc/common.h r3_encode): T = fp32 pattern rounded half away to 24 bits,
    hi = (T + 0x80) >> 8 (a bf16 pattern), lo = int8(T - (hi << 8))."""
    b = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    hi = (((b + 0x8080) >> 16) & 0xffff).astype(np.uint16)
    lo = (((b + 0x80) >> 8) & 0xff).astype(np.uint8).view(np.int8)
    return hi, lo


def _r3_decode_np(hi, lo):
    v = ((hi.astype(np.int64) << 16) + (lo.astype(np.int64) << 8)) & 0xffffffff
    return v.astype(np.uint32).view(np.float32)


def bf16_bits(t):
    """uint16 bit patterns (numpy) of a bf16 tensor."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def r3_encode_t(x):
    """fp32 tensor -> (hi bf16 tensor, lo int8 tensor) on x's device, through _r3_encode_np."""
    hi, lo = _r3_encode_np(x.detach().float().cpu().numpy())
    return (torch.from_numpy(hi.view(np.int16).copy()).view(torch.bfloat16).to(x.device), torch.from_numpy(lo.copy()).to(x.device))


def r3_decode_t(hi, lo, lo_unsigned=False):
    l = lo.cpu().numpy()
    if lo_unsigned:
        l = l.view(np.uint8)
    return torch.from_numpy(_r3_decode_np(bf16_bits(hi), l).copy()).to(hi.device)


# ---- reference --------------------------------------------------------------------------------------------------------------
def gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def fold(W, gamma, beta, bias):
    """cpt_fold_ln_weights: Wf = bf16(gamma * W) (the fp32 product rounded to nearest even), colc = sum_k Wf, cold = W . beta + bias."""
    Wf = (gamma.float()[None, :] * W.float()).to(torch.bfloat16)
    colc = Wf.double().sum(1)
    cold = W.double() @ beta.double()
    if bias is not None:
        cold = cold + bias.double()
    return Wf, colc, cold


def stats(x, N=None, mut=None):
    """[M][slots][2] table of (sum, sum of squares) per 96-column block of x[M][N]; pad slots 0."""
    x = x.double()
    M = x.size(0)
    N = N or x.size(1)
    P = parts(N)
    st = torch.zeros((M, slots(N), 2), dtype=torch.float64, device=x.device)
    for p in range(P):
        blk = x[:, p * BLK:min(p * BLK + BLK, N)]
        st[:, p, 0] = blk.sum(1)
        st[:, p, 1] = (blk * blk).sum(1)
    if mut == "last_block_dropped":
        st[:, P - 1, :] = 0
    if mut == "sum_sq_swapped":
        st = st.flip(2)
    return st


def mean_rstd(st, hidden, eps, mut=None):
    """(mu [M,1], rstd [M,1], var [M,1]) from a table: the first `parts` slots, one-pass variance clamped at 0."""
    P, S = parts(hidden), slots(hidden)
    st = st.double()
    M = st.size(0)
    tot = st[:, :P, :].sum(1)
    if mut == "pad_slot_added":          # one slot too many: the pad slot, or (no pad slot) the next row's first
        flat = st.reshape(-1, 2)
        tot = tot + flat[(torch.arange(M, device=st.device) * S + P) % flat.size(0)]
    if mut == "stats_row_plus_1":
        tot = tot.roll(-1, 0)
    inv_h = 1.0 / (S * BLK) if mut == "inv_h_padded" else 1.0 / hidden
    mu = tot[:, 0] * inv_h
    var = (tot[:, 1] * inv_h - mu * mu).clamp_min(0.0)
    rs = 1.0 / torch.sqrt(var + eps)
    return mu[:, None], rs[:, None], var[:, None]


def _gemm(a, w, mut):
    a, w = a.double(), w.double()
    if mut == "k_tile_dropped":
        a, w = a[:, :-64], w[:, :-64]
    return a @ w.T


def _residual(resid, st_in, g_in, b_in, eps, hidden, mut=None):
    r = resid.double()
    if g_in is None:
        return r
    mu, rs, _ = mean_rstd(st_in, hidden, eps, mut)
    r = (r - mu) * rs * g_in.double()
    return r if mut == "ln_shift_dropped" else r + b_in.double()


def producer(a, w, bias, resid, st_in, g_in, b_in, eps, hidden, mut=None):
    """out = a . w^T + bias + R, R = resid or LayerNorm(resid; st_in, g_in, b_in); returns (out, table of out), float64."""
    b = bias.double()
    if mut == "bias_col_plus_4":
        b = b.roll(-4)
    out = _gemm(a, w, mut) + b + _residual(resid, st_in, g_in, b_in, eps, hidden, mut)
    return out, stats(out, mut=mut)


def consumer(a, wf, st_in, colc, cold, eps, hidden, gelu_on, mut=None):
    """The folded form: [gelu]( rstd * (a . wf^T - mean * colc) + cold )."""
    mu, rs, _ = mean_rstd(st_in, hidden, eps, mut)
    c = colc.double()
    if mut == "mean_colc_kept":
        c = c * 0
    pre = rs * (_gemm(a, wf, mut) - mu * c) + cold.double()
    return gelu(pre) if gelu_on else pre


def consumer_unfolded(x, W, gamma, beta, bias, eps, gelu_on):
    """[gelu]( LayerNorm(x) . W^T + bias ) with torch's LayerNorm in float64."""
    K = x.size(1)
    ln = torch.nn.functional.layer_norm(x.double(), (K,), None if gamma is None else gamma.double(), None if beta is None else beta.double(), eps)
    pre = ln @ W.double().T + bias.double()
    return gelu(pre) if gelu_on else pre


# ---- bound ---------------------------------------------------------------------------------------------------------------------
def _half_ulp(v, bits):
    """Half an ulp of a format with `bits` significant bits at |v| (float64 tensor): 2^(floor(log2 |v|) - bits); 0 at 0."""
    v = v.abs()
    e = torch.floor(torch.log2(v.clamp_min(1e-300)))
    return torch.where(v > 0, torch.exp2(e - bits), torch.zeros_like(v))


FMT_BITS = {"f32": 24, "bf16": 8, "r3": 16}


def _fmt(core, ref, fmt):
    # (estimated terms, the format's half ulp).  The format rounds the COMPUTED value, which lies within `core` of ref: half an ulp at
    # the far end of that interval.  The two stay apart because the half ulp is exact -- a correctly rounded result does reach it -- so
    # "the emulation within a quarter of the bound" can only be asked of the estimated terms: see _ratio
    return core, _half_ulp(ref.abs() + core, FMT_BITS[fmt])


def _stat_err(st_in, hidden, eps):
    """(mu, rs, |error of mu|, relative error of rstd) of an fp32 reader of the table."""
    mu, rs, var = mean_rstd(st_in, hidden, eps)
    ve = var + eps
    rel_var = C_VAR * U * (1.0 + mu * mu / ve) + hidden * U
    e_rs = 0.5 * rel_var + 4 * U                       # + the rsqrt itself and the rounding of var + eps
    e_mu = hidden * U * torch.sqrt(var + mu * mu) + U * mu.abs()
    return mu, rs, e_mu, e_rs


def producer_bound(a, w, bias, resid, st_in, g_in, b_in, eps, hidden, fmt):
    K = a.size(1)
    core = K * U * (a.double().abs() @ w.double().abs().T)
    R = _residual(resid, st_in, g_in, b_in, eps, hidden)
    core = core + 4 * U * (bias.double().abs() + R.abs())
    if g_in is not None:
        mu, rs, e_mu, e_rs = _stat_err(st_in, hidden, eps)
        core = core + g_in.double().abs() * rs * (e_mu + (resid.double() - mu).abs() * (e_rs + 3 * U))
    ref, _ = producer(a, w, bias, resid, st_in, g_in, b_in, eps, hidden)
    return _fmt(core, ref, fmt)


def consumer_bound(a, wf, st_in, colc, cold, eps, hidden, gelu_on, a_err=None, mu_err=None, rs_err=None, colc_err=None, cold_err=None):
    """Bound of the bf16 output.  a_err [M,K] / mu_err [M,1] / rs_err [M,1] (relative) / colc_err [N] / cold_err [N]: how far the
    kernel's operands may lie from the ones given here (the chain: the producer's bf16 rounding through |wf|, its table's error)."""
    K = a.size(1)
    aa, ww = a.double().abs(), wf.double().abs()
    if a_err is not None:
        aa = aa + a_err
    mu, rs, e_mu, e_rs = _stat_err(st_in, hidden, eps)
    if mu_err is not None:
        e_mu = e_mu + mu_err
    if rs_err is not None:
        e_rs = e_rs + rs_err
    c, d = colc.double(), cold.double()
    acc = a.double() @ wf.double().T
    inner = acc - mu * c
    e_inner = K * U * (aa @ ww.T) + e_mu * c.abs() + 2 * U * (mu * c).abs() + U * inner.abs()
    if a_err is not None:
        e_inner = e_inner + a_err @ ww.T
    if colc_err is not None:
        e_inner = e_inner + (mu.abs() + e_mu) * colc_err
    pre = rs * inner + d
    core = rs * (1 + e_rs) * e_inner + (rs * inner).abs() * (e_rs + 2 * U) + 4 * U * (d.abs() + pre.abs())
    if cold_err is not None:
        core = core + cold_err
    ref = pre
    if gelu_on:
        ref = gelu(pre)
        core = GELU_SLOPE * core + GELU_ABS + U * ref.abs()
    return _fmt(core, ref, "bf16")


def chain_errs(x_ref, e_f32, eps):
    """Operand errors of a consumer that reads a producer's outputs: the table summarises fp32 values within e_f32 [M,H] of x_ref."""
    x = x_ref.double()
    mu = x.mean(1, keepdim=True)
    var = x.var(1, unbiased=False, keepdim=True)
    ee = e_f32 + e_f32.mean(1, keepdim=True)
    d_var = 2 * ((x - mu).abs() * ee).mean(1, keepdim=True) + (ee * ee).mean(1, keepdim=True)
    return e_f32.mean(1, keepdim=True), 0.5 * d_var / (var + eps)


# ---- checks (shared by the CPU file, which runs them on the emulation and the planted defects, and the GPU file) --------------------
def _ratio(err, bound):
    """bound = (estimated terms, exact format term): max over the elements of (err - format term)+ / estimated terms, so that
    err <= bound  <=>  ratio <= 1, and ratio <= 1/4 says the estimated terms are met four times over.  0 / 0 = 0; inf when a value is
    not finite."""
    core, exact = bound
    if not bool(torch.isfinite(err).all()):
        return FAIL
    ex = (err - exact).clamp_min(0.0)
    r = torch.where(ex > 0, ex / core.clamp_min(1e-300), torch.zeros_like(ex))
    return float(r.max())


def check_stats(st_out, src_f32, N):
    """Every slot p < parts of st_out against the float64 (sum, sum of squares) of columns [96 p, min(96 p + 96, N)) of the fp32 tensor
    it summarises, within 96 * U * (sum |x|, sum x^2); pad slots must be ZERO: the wave that owns a pad slot's column block lies outside
    the matrix, sums zeros and stores them (gemm.hip, the st_out float2 store of the slab epilogue)."""
    ref = stats(src_f32, N)
    x = src_f32.double()
    P = parts(N)
    bound = torch.zeros_like(ref)
    for p in range(P):
        blk = x[:, p * BLK:min(p * BLK + BLK, N)]
        bound[:, p, 0] = BLK * U * blk.abs().sum(1)
        bound[:, p, 1] = BLK * U * (blk * blk).sum(1)
    out = {"st_out": _ratio((st_out.double() - ref)[:, :P].abs(), (bound[:, :P], 0.0))}
    pad = st_out[:, P:, :]
    out["st_pad_zero"] = 0.0 if (pad.numel() == 0 or bool((pad == 0).all())) else FAIL
    return out


def check_producer(inp, res):
    """inp: the operands (a, w, bias, resid, st_in, g_in, b_in, eps, hidden; resid = the fp32 values the kernel adds, for the 3-byte form
    the decoded pair).  res: out_f32 + out_bf16 (fp32 form) or hi + lo + src_f32 (3-byte form; src_f32 = the fp32 values before
    encoding), and st_out.  Returns {check: worst error / bound}; a check passes at <= 1."""
    args = (inp["a"], inp["w"], inp["bias"], inp["resid"], inp["st_in"], inp["g_in"], inp["b_in"], inp["eps"], inp["hidden"])
    ref, _ = producer(*args)
    N = ref.size(1)
    out = {}
    if "hi" in res:
        dec = r3_decode_t(res["hi"], res["lo"])
        out["decode"] = _ratio((dec.double() - ref).abs(), producer_bound(*args, "r3"))
        src = res["src_f32"]
        hi_e, lo_e = _r3_encode_np(src.cpu().numpy())
        fin = np.isfinite(src.cpu().numpy())
        same = np.array_equal(bf16_bits(res["hi"])[fin], hi_e[fin]) and np.array_equal(res["lo"].cpu().numpy()[fin], lo_e[fin])
        out["encode_bits"] = 0.0 if same else FAIL
    else:
        src = res["out_f32"]
        out["out_f32"] = _ratio((src.double() - ref).abs(), producer_bound(*args, "f32"))
        out["out_bf16_bits"] = 0.0 if np.array_equal(bf16_bits(res["out_bf16"]), bf16_bits(src.to(torch.bfloat16))) else FAIL
    out.update(check_stats(res["st_out"], src, N))
    return out


def check_consumer(inp, out_bf16, ref=None, **errs):
    args = (inp["a"], inp["wf"], inp["st_in"], inp["colc"], inp["cold"], inp["eps"], inp["hidden"], inp["gelu"])
    if ref is None:
        ref = consumer(*args)
    return {"cons": _ratio((out_bf16.double() - ref).abs(), consumer_bound(*args, **errs))}


# ---- planted defects: the float64 reference with ONE defect, rounded to the output formats as a perfect kernel would -------------
MUTATIONS = [
    "last_block_dropped",    # the last 96-column block left out of the row sums
    "sum_sq_swapped",        # sum and sum of squares swapped
    "inv_h_padded",          # inv_h from N padded to slots * 96
    "stats_row_plus_1",      # the statistics of row m + 1 used for row m
    "bias_col_plus_4",       # bias taken from column n + 4
    "k_tile_dropped",        # the last 64-wide K-tile dropped
    "mean_colc_kept",        # mean * colc not subtracted
    "bf16_truncated",        # bf16 output truncated instead of rounded
    "lo_unsigned",           # the lo byte of the 3-byte code read unsigned
    "ln_shift_dropped",      # the residual LayerNorm applied without its shift
    "pad_slot_added",        # the pad slot added in
]
STAT_MUTATIONS = ("last_block_dropped", "sum_sq_swapped")      # these touch the table a producer WRITES: the statistics check finds them


def _trunc_bf16(x_f32):
    b = x_f32.contiguous().view(torch.int32) & ~0xffff
    return b.view(torch.float32).to(torch.bfloat16)


def ideal_producer(inp, mut=None, r3=False):
    """What a perfect kernel (float64 arithmetic, outputs rounded once) returns for check_producer -- with `mut`, one defect planted.
    r3: inp carries resid_hi / resid_lo; the caller's inp["resid"] stays the correct decode."""
    resid = r3_decode_t(inp["resid_hi"], inp["resid_lo"], lo_unsigned=(mut == "lo_unsigned")) if r3 else inp["resid"]
    out, st = producer(inp["a"], inp["w"], inp["bias"], resid, inp["st_in"], inp["g_in"], inp["b_in"], inp["eps"], inp["hidden"], mut)
    f32 = out.float()
    st = stats(f32, mut=mut).float()
    if r3:
        hi, lo = r3_encode_t(f32)
        return {"hi": hi, "lo": lo, "src_f32": f32, "st_out": st}
    return {"out_f32": f32, "out_bf16": _trunc_bf16(f32) if mut == "bf16_truncated" else f32.to(torch.bfloat16), "st_out": st}


def ideal_consumer(inp, mut=None):
    y = consumer(inp["a"], inp["wf"], inp["st_in"], inp["colc"], inp["cold"], inp["eps"], inp["hidden"], inp["gelu"], mut)
    return y.float().to(torch.bfloat16)


# ---- fp32 emulation of the documented arithmetic (numpy; shows that a correct fp32 implementation meets the bound) ------------------
F = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def emulate_stats(x, N=None):
    x = np.asarray(x, F)
    M = x.shape[0]
    N = N or x.shape[1]
    st = np.zeros((M, slots(N), 2), F)
    for p in range(parts(N)):
        s, q = np.zeros(M, F), np.zeros(M, F)
        for k in range(p * BLK, min(p * BLK + BLK, N)):
            s = (s + x[:, k]).astype(F)
            q = _fma(x[:, k], x[:, k], q)
        st[:, p, 0], st[:, p, 1] = s, q
    return st


def emulate_mean_rstd(st, hidden, eps):
    st = np.asarray(st, F)
    s, q = np.zeros(st.shape[0], F), np.zeros(st.shape[0], F)
    for p in range(parts(hidden)):
        s = (s + st[:, p, 0]).astype(F)
        q = (q + st[:, p, 1]).astype(F)
    inv_h = F(1.0) / F(hidden)
    mu = (s * inv_h).astype(F)
    v = np.maximum(_fma(-mu, mu, (q * inv_h).astype(F)), F(0))
    v = (v + F(eps)).astype(F)
    rs = (1.0 / np.sqrt(v.astype(np.float64))).astype(F)
    return mu[:, None], rs[:, None]


def emulate_gemm(a, w):
    a, w = np.asarray(a, F), np.asarray(w, F)
    acc = np.zeros((a.shape[0], w.shape[0]), F)
    for k in range(a.shape[1]):
        acc = _fma(a[:, k:k + 1], w[None, :, k], acc)
    return acc


def _np(t):
    return None if t is None else t.detach().float().cpu().numpy()


def emulate_producer(inp, r3=False, acc=None):
    a, w, bias, resid, g, b = (_np(inp[k]) for k in ("a", "w", "bias", "resid", "g_in", "b_in"))
    x = ((emulate_gemm(a, w) if acc is None else acc) + bias[None, :]).astype(F)
    if g is not None:
        mu, rs = emulate_mean_rstd(_np(inp["st_in"]), inp["hidden"], inp["eps"])
        resid = _fma(((resid - mu).astype(F) * rs).astype(F), g[None, :], b[None, :])       # ln_apply
    x = (x + resid).astype(F)
    f32 = torch.from_numpy(x)
    st = torch.from_numpy(emulate_stats(x))
    if r3:
        hi, lo = r3_encode_t(f32)
        return {"hi": hi, "lo": lo, "src_f32": f32, "st_out": st}
    return {"out_f32": f32, "out_bf16": f32.to(torch.bfloat16), "st_out": st}


def emulate_consumer(inp, acc=None):
    a, wf, c, d = (_np(inp[k]) for k in ("a", "wf", "colc", "cold"))
    mu, rs = emulate_mean_rstd(_np(inp["st_in"]), inp["hidden"], inp["eps"])
    pre = _fma(rs, _fma(-mu, c[None, :], emulate_gemm(a, wf) if acc is None else acc), d[None, :])                   # ln_fold
    y = torch.from_numpy(pre)
    if inp["gelu"]:
        y = gelu(y.double()).float()
    return y.to(torch.bfloat16)


# ---- input families ----------------------------------------------------------------------------------------------------------------
FAMILIES = {"ratio0": 0.0, "ratio4": 4.0, "ratio64": 64.0, "outliers": 0.3}


def family_rows(gen, family, M, H, zero_row):
    """fp32 rows [M][H] with |row mean| / row std = FAMILIES[family] (signs alternate by row, the std varies by row); `outliers`: four
    columns at 30 std.  Row `zero_row` (None: no row) is all zero."""
    sd = 0.8 + 0.8 * torch.rand((M, 1), generator=gen, dtype=torch.float64)
    x = torch.randn((M, H), generator=gen, dtype=torch.float64) * sd
    sign = torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0).double()[:, None]
    x = x + FAMILIES[family] * sd * sign
    if family == "outliers":
        for j, c in enumerate((3, H // 3 + 1, H // 2 + 5, H - 2)):
            x[:, c] = 30.0 * sd[:, 0] * (1.0 if j % 2 == 0 else -1.0)
    if zero_row is not None:
        x[zero_row] = 0
    return x.float()


def table_with_nan_pads(x_f32):
    """The fp32 table of x (float64 sums rounded once) with NaN in its pad slots: a reader must skip them."""
    st = stats(x_f32).float()
    st[:, parts(x_f32.size(1)):, :] = float("nan")
    return st


def make_case(seed, family, M, H, Kp, I, zero_row, device="cpu"):
    """One half-layer's operands: producer a[M,Kp] . w[H,Kp]^T + bias + LayerNorm(x0; g_in, b_in); consumer (I not None) on the same rows:
    a = bf16(x0), table of x0, folded W2[I,H]."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=gen, dtype=torch.float32)      # noqa: E731
    x0 = family_rows(gen, family, M, H, zero_row)
    c = {"x0": x0, "st0": table_with_nan_pads(x0), "eps": 1e-12, "H": H,
         "a": rn(M, Kp).to(torch.bfloat16), "w": (rn(H, Kp) * (0.03 * math.sqrt(768.0 / max(Kp, 768)))).to(torch.bfloat16),
         "bias": rn(H) * 0.1, "g_in": 1.0 + rn(H) * 0.1, "b_in": rn(H) * 0.1}
    c["r_hi"], c["r_lo"] = r3_encode_t(x0)
    if I is not None:
        c.update(W2=rn(I, H) * 0.03, gamma2=1.0 + rn(H) * 0.1, beta2=rn(H) * 0.1, bias2=rn(I) * 0.1)
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in c.items()}


def producer_inputs(c, fold_resid, r3=False):
    inp = {"a": c["a"], "w": c["w"], "bias": c["bias"], "eps": c["eps"], "hidden": c["H"],
           "resid": r3_decode_t(c["r_hi"], c["r_lo"]) if r3 else c["x0"],
           "st_in": c["st0"] if fold_resid else None, "g_in": c["g_in"] if fold_resid else None, "b_in": c["b_in"] if fold_resid else None}
    if r3:
        inp["resid_hi"], inp["resid_lo"] = c["r_hi"], c["r_lo"]
    return inp


def consumer_inputs(c, gelu_on):
    wf, colc, cold = fold(c["W2"], c["gamma2"], c["beta2"], c["bias2"])
    return {"a": c["x0"].to(torch.bfloat16), "wf": wf, "st_in": c["st0"], "colc": colc.float(), "cold": cold.float(), "eps": c["eps"],
            "hidden": c["H"], "gelu": gelu_on}


# shape classes (H = producer N = consumer K, producer K, consumer N) of tests/test_gpu_ln_gemm_parity.py; H = 200 is no legal consumer K
SHAPES = [(768, 64, 256), (768, 128, 256), (768, 768, 192), (768, 3072, 256), (768, 2048, 192),
          (1024, 64, 256), (1024, 128, 192), (1024, 768, 256), (200, 64, None), (200, 128, None), (200, 768, None)]


def emulation_ratios(c):
    """Every check on the fp32 emulation of every operator form of case c."""
    out = {}
    acc = emulate_gemm(_np(c["a"]), _np(c["w"]))
    for r3 in (False, True):
        for fr in (True, False):
            inp = producer_inputs(c, fr, r3)
            for k, v in check_producer(inp, emulate_producer(inp, r3, acc)).items():
                out["prod%s%s.%s" % ("3" if r3 else "", "_ln" if fr else "", k)] = v
    if "W2" in c:
        acc = None
        for g in (True, False):
            inp = consumer_inputs(c, g)
            acc = emulate_gemm(_np(inp["a"]), _np(inp["wf"])) if acc is None else acc
            out["cons%s" % ("_gelu" if g else "")] = check_consumer(inp, emulate_consumer(inp, acc))["cons"]
    return out


if __name__ == "__main__":
    import sys
    if len(sys.argv) > 1:
        C_VAR = float(sys.argv[1])
    for fam in FAMILIES:
        worst = ("", 0.0)
        for i, (H, Kp, I) in enumerate(SHAPES):
            r = emulation_ratios(make_case(100 + i, fam, 5, H, Kp, I, 2))
            k = max(r, key=r.get)
            if r[k] > worst[1]:
                worst = ("%s H=%d K=%d" % (k, H, Kp), r[k])
        print("%-9s worst emulation error / bound %.4f (%s)" % (fam, worst[1], worst[0]))
