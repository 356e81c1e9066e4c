"""GPU: the LayerNorm-folded GEMMs against the float64 reference of tests/_lnref.py at every tile shape the producers run.

The reference, the bound and the checks are those of tests/_lnref.py; tests/test_ln_gemm_ref_cpu.py shows on the CPU that an fp32
implementation meets the bound four times over and that every planted epilogue defect breaks it.  Here the same checks run on the kernels:
  producers   cpt_gemm_ln_prod_tile / cpt_gemm_ln_prod3_tile at tiles 13 (128x192), 18 (64x192), 11 (192x192), 10 (128x384) and, for the
              3-byte form, 15 (128x192 two workgroups per CU, K = 2048), N in {768, 1024, 200}, K from one K-tile to 3072, plain and
              LayerNorm'ed residual, M in {1, 77, bm, bm + 1, 2 bm + 33}: fp32 / decoded output within the bound, an exact-copy probe,
              out_bf16 and (out_hi, out_lo) bit-equal to the codes of the fp32 value, st_out against the tensor it summarises, sentinels
              around every buffer, NaN around every operand, determinism
  fold        cpt_fold_ln_weights against _lnref.fold
  chain       producer -> fold -> consumer on the producer's own out_bf16 / out_hi and st_out
  regimes     rows with |mean| / std in {0, 4, 64}, outlier columns, an all-zero row
Every case is a handful of small launches; the reference is computed in float64 on the device from the same tensors."""
import functools

import pytest
import torch

import _lnref as R

pytestmark = pytest.mark.gpu

BM = {13: 128, 18: 64, 11: 192, 10: 128, 15: 128}      # rows of the tile an id forces (gemm.hip launch_fast)
EPS = 1e-12
SENT32, SENT16, SENT8 = 0x4b5a5a5a, 0x4b5a, 0x5a       # finite sentinels (fp32 14309978.0, bf16 14286848.0, int8 90): far from every result
PROBES = (5, 100, -3)                                    # output columns of the exact-copy probe


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cpt_amd import _lib
    _lib.check(_lib.lib().cpt_check_device(0), "cpt_check_device")
    return torch.device("cuda:0")


def _rows(bm):
    return sorted({1, 77, bm, bm + 1, 2 * bm + 33})


class _Padded:
    """An [M][N] output inside an [M + 8][N + 8] buffer filled with a sentinel bit pattern (row stride N + 8)."""

    def __init__(self, M, N, dtype, dev):
        it, pat = {torch.float32: (torch.int32, SENT32), torch.bfloat16: (torch.int16, SENT16), torch.int8: (torch.int8, SENT8)}[dtype]
        self.raw = torch.full((M + 8, N + 8), pat, dtype=it, device=dev)
        self.pat, self.M, self.N = pat, M, N
        self.view = self.raw.view(dtype)[:M, :N]

    def intact(self):
        keep = torch.ones_like(self.raw, dtype=torch.bool)
        keep[:self.M, :self.N] = False
        return bool((self.raw[keep] == self.pat).all())


def _inside_nan(t, fill=float("nan")):
    """t[M][C] as a view of a wider [M][C + 8] tensor whose extra columns hold NaN (int8: the sentinel): row stride C + 8."""
    big = torch.full((t.size(0), t.size(1) + 8), SENT8 if t.dtype == torch.int8 else fill, dtype=t.dtype, device=t.device)
    big[:, :t.size(1)] = t
    return big[:, :t.size(1)]


def _nan_table(M, N, dev):
    st = torch.full((M + 8, R.slots(N), 2), float("nan"), device=dev)
    return st, st[:M]


@functools.lru_cache(maxsize=None)
def _operands(N, K, M, fold):
    """Producer operands with the exact-copy probe planted: W row n = one 1.0 at column k(n), bias[n] = b_in[n] = 0; plain residual: column n
    zero in every row; LayerNorm'ed residual: the all-zero row (row M // 2) alone has a zero residual.  Shared by every tile; never modified."""
    c = R.make_case(7 * N + K + M, "outliers", M, N, K, None, M // 2, device="cuda:0")
    w, bias, b_in, x0 = c["w"].clone(), c["bias"].clone(), c["b_in"].clone(), c["x0"].clone()
    probes = [(n % N, (17 * (i + 1)) % K) for i, n in enumerate(PROBES)]
    for n, k in probes:
        w[n] = 0
        w[n, k] = 1.0
        bias[n] = 0
        b_in[n] = 0
        if not fold:
            x0[:, n] = 0
    hi, lo = R.r3_encode_t(x0)
    c.update(w=w, bias=bias, b_in=b_in, x0=x0, r_hi=hi, r_lo=lo, st0=R.table_with_nan_pads(x0), probes=probes)
    return c


def _launch_pair(ops, c, tile, fold, M, N, dev):
    """gemm_ln_prod on the decoded residual (the fp32 values prod3 encodes from) and gemm_ln_prod3 on the pair, every buffer padded."""
    xq = R.r3_decode_t(c["r_hi"], c["r_lo"])
    a = _inside_nan(c["a"])
    st_in, g, b = (c["st0"], c["g_in"], c["b_in"]) if fold else (None, None, None)
    bufs = {"f32": _Padded(M, N, torch.float32, dev), "bf16": _Padded(M, N, torch.bfloat16, dev), "hi": _Padded(M, N, torch.bfloat16, dev),
            "lo": _Padded(M, N, torch.int8, dev)}
    st_raw, st = _nan_table(M, N, dev)
    st3_raw, st3 = _nan_table(M, N, dev)
    ops.gemm_ln_prod(a, c["w"], c["bias"], _inside_nan(xq), st_in, g, b, EPS, N, tile=tile, out=bufs["f32"].view, out_lp=bufs["bf16"].view, st_out=st)
    ops.gemm_ln_prod3(a, c["w"], c["bias"], _inside_nan(c["r_hi"]), _inside_nan(c["r_lo"]), st_in, g, b, EPS, N, tile=tile,
                      out_hi=bufs["hi"].view, out_lo=bufs["lo"].view, st_out=st3)
    return xq, bufs, st_raw, st3_raw


def _check_producers(dev, tile, N, K, fold):
    from cpt_amd import ops
    for M in _rows(BM[tile]):
        c = _operands(N, K, M, fold)
        xq, bufs, st_raw, st3_raw = _launch_pair(ops, c, tile, fold, M, N, dev)
        _, bufs2, st_raw2, st3_raw2 = _launch_pair(ops, c, tile, fold, M, N, dev)
        tag = "tile %d N=%d K=%d M=%d fold=%d" % (tile, N, K, M, fold)
        # sentinels, finiteness, determinism
        for k, b in bufs.items():
            assert b.intact(), "%s: %s wrote outside its matrix" % (tag, k)
            assert torch.equal(b.raw, bufs2[k].raw), "%s: %s differs on a second launch" % (tag, k)
        for s, s2 in ((st_raw, st_raw2), (st3_raw, st3_raw2)):
            assert bool(torch.isnan(s[M:]).all()), "%s: st_out rows beyond M written" % tag
            assert bool(torch.isfinite(s[:M]).all()), "%s: st_out not finite" % tag
            assert torch.equal(s[:M], s2[:M]), "%s: st_out differs on a second launch" % tag
        out_f32, out_bf16 = bufs["f32"].view, bufs["bf16"].view
        assert bool(torch.isfinite(out_f32).all())
        # reference, bound, codes, statistics
        inp = {"a": c["a"], "w": c["w"], "bias": c["bias"], "resid": xq, "st_in": c["st0"] if fold else None, "g_in": c["g_in"] if fold else None,
               "b_in": c["b_in"] if fold else None, "eps": EPS, "hidden": N}
        r = R.check_producer(inp, {"out_f32": out_f32, "out_bf16": out_bf16, "st_out": st_raw[:M]})
        r3 = R.check_producer(inp, {"hi": bufs["hi"].view, "lo": bufs["lo"].view, "src_f32": out_f32.contiguous(), "st_out": st3_raw[:M]})
        print("%s: prod %s | prod3 %s" % (tag, " ".join("%s=%.3g" % kv for kv in r.items()), " ".join("%s=%.3g" % kv for kv in r3.items())))
        assert all(v <= 1.0 for v in r.values()), (tag, r)
        assert all(v <= 1.0 for v in r3.values()), (tag, r3)
        # exact-copy probe: a row or column permutation of the fragment layout would move these
        dec = R.r3_decode_t(bufs["hi"].view, bufs["lo"].view)
        rows = slice(None) if not fold else slice(M // 2, M // 2 + 1)
        for n, k in c["probes"]:
            want = c["a"][rows, k].float()
            assert torch.equal(out_f32[rows, n], want), "%s: probe column %d is no copy of A[:, %d]" % (tag, n, k)
            assert torch.equal(dec[rows, n], want), "%s: 3-byte probe column %d is no copy of A[:, %d]" % (tag, n, k)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("K", [64, 128, 768])
@pytest.mark.parametrize("N", [768, 1024, 200])
@pytest.mark.parametrize("tile", [13, 18, 11, 10])
def test_producers_match_float64(dev, tile, N, K, fold):
    """K = 64 is one K-tile, K = 128 fewer K-tiles than ring stages.  N = 1024: 11 blocks, the last 64 wide, one pad slot, and with 192-column
    tiles a wave that owns no valid column; N = 200: a ragged last block, guarded epilogue everywhere."""
    _check_producers(dev, tile, N, K, fold)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("tile", [13, 18, 11, 10])
def test_producers_match_float64_long_k(dev, tile, fold):
    _check_producers(dev, tile, 768, 3072, fold)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("N", [768, 1024, 200])
def test_producers_match_float64_two_per_cu(dev, N, fold):
    """Tile 15 exists for the 3-byte producer only (the fp32 producer runs its 128x192 kernel, same K order: the fp32 values the codes are
    compared with come from there)."""
    _check_producers(dev, 15, N, 2048, fold)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("N", [192, 400])
def test_forced_128x384_tile_stays_inside_the_table(dev, N, fold):
    """N mod 384 in 1..192: the table has 2 ceil(N / 192) slots per row, the last 384-column tile would own 4 ceil(N / 384) -- its waves beyond N
    would store their zero sums into the next row's first slots and, for the last row, behind the table.  gemm.hip ln_prod_variant runs the
    128x192 tile there; the statistics check and the NaN rows behind the table see any such store."""
    _check_producers(dev, 10, N, 128, fold)


def _fold_call(W, gamma, beta, bias, N, K, rows):
    from cpt_amd import _lib as L
    dev = W.device
    wf = torch.full((rows, K), SENT16, dtype=torch.int16, device=dev)
    colc = torch.full((rows,), SENT32, dtype=torch.int32, device=dev)
    cold = torch.full((rows,), SENT32, dtype=torch.int32, device=dev)
    L.check(L.lib().cpt_fold_ln_weights(W.data_ptr(), gamma.data_ptr(), beta.data_ptr(), L.ptr(bias), wf.data_ptr(), colc.data_ptr(), cold.data_ptr(),
                                        N, K, L.stream_ptr()), "cpt_fold_ln_weights")
    return wf, colc, cold


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("K", [4, 768, 1024])
@pytest.mark.parametrize("N", [1, 7, 768])
def test_fold_ln_weights(dev, N, K, bias):
    gen = torch.Generator().manual_seed(N * 31 + K)
    W = (torch.randn((N, K), generator=gen) * 0.03).to(dev)
    gamma, beta = (1 + torch.randn(K, generator=gen) * 0.1).to(dev), (torch.randn(K, generator=gen) * 0.1).to(dev)
    bs = torch.randn(N, generator=gen).to(dev) if bias else None
    wf, colc, cold = _fold_call(W, gamma, beta, bs, N, K, N + 3)
    wf_ref, colc_ref, cold_ref = R.fold(W, gamma, beta, bs)
    assert torch.equal(wf[:N], wf_ref.view(torch.int16))
    assert bool((wf[N:] == SENT16).all()) and bool((colc[N:] == SENT32).all()) and bool((cold[N:] == SENT32).all())      # rows at and beyond N untouched
    e_c = (colc[:N].view(torch.float32).double() - colc_ref).abs()
    e_d = (cold[:N].view(torch.float32).double() - cold_ref).abs()
    b_c = K * R.U * wf_ref.double().abs().sum(1)
    b_d = K * R.U * ((beta.double()[None, :] * W.double()).abs().sum(1) + (bs.double().abs() if bias else 0))
    print("fold N=%d K=%d: colc %.3g of its bound, cold %.3g" % (N, K, float((e_c / b_c).max()), float((e_d / b_d).max())))
    assert bool((e_c <= b_c).all()) and bool((e_d <= b_d).all())


@pytest.mark.parametrize("tile,H,r3", [(13, 768, False), (18, 768, False), (11, 768, False), (10, 768, False), (13, 1024, False), (18, 1024, False),
                                       (11, 1024, False), (10, 1024, False), (13, 768, True), (10, 1024, True)])
def test_chain_producer_fold_consumer(dev, tile, H, r3):
    """One encoder half-layer at operator level: x1 = A.W1^T + b1 + LayerNorm(x0) (producer at `tile`, pad slots of its table NaN before it
    runs), cpt_fold_ln_weights, y = gelu(LayerNorm(x1).W2^T + b2) by the consumer on the producer's OWN out_bf16 (3-byte form: out_hi) and
    st_out.  Reference: the float64 unfolded composition on the producer's float64 output, with the folded weight the fold test holds bit-equal
    to _lnref.fold; the bound carries x1's error and bf16 rounding through |W2| and through the statistics (_lnref.chain_errs)."""
    from cpt_amd import ops
    I, Kp = 256, 256
    for M in (77, 2 * BM[tile] + 33):
        c = R.make_case(H + M + tile, "outliers", M, H, Kp, I, M // 2, device="cuda:0")
        pin = R.producer_inputs(c, True, r3)
        a = _inside_nan(c["a"])
        st_raw, st = _nan_table(M, H, dev)
        if r3:
            hi, lo = _Padded(M, H, torch.bfloat16, dev), _Padded(M, H, torch.int8, dev)
            ops.gemm_ln_prod3(a, c["w"], c["bias"], _inside_nan(c["r_hi"]), _inside_nan(c["r_lo"]), c["st0"], c["g_in"], c["b_in"], EPS, H, tile=tile,
                              out_hi=hi.view, out_lo=lo.view, st_out=st)
            x1_lp = hi.view
        else:
            f32, lp = _Padded(M, H, torch.float32, dev), _Padded(M, H, torch.bfloat16, dev)
            ops.gemm_ln_prod(a, c["w"], c["bias"], _inside_nan(c["x0"]), c["st0"], c["g_in"], c["b_in"], EPS, H, tile=tile, out=f32.view, out_lp=lp.view, st_out=st)
            x1_lp = lp.view
        wf_k, colc_k, cold_k = _fold_call(c["W2"], c["gamma2"], c["beta2"], c["bias2"], I, H, I)
        wf_ref, colc_ref, cold_ref = R.fold(c["W2"], c["gamma2"], c["beta2"], c["bias2"])
        assert torch.equal(wf_k, wf_ref.view(torch.int16))
        y = ops.gemm_ln_cons(x1_lp, wf_k.view(torch.bfloat16), st, colc_k.view(torch.float32), cold_k.view(torch.float32), EPS, H, True)
        assert bool(torch.isfinite(y).all())
        args = (pin["a"], pin["w"], pin["bias"], pin["resid"], pin["st_in"], pin["g_in"], pin["b_in"], EPS, H)
        x1_ref, _ = R.producer(*args)
        y_ref = R.consumer_unfolded(x1_ref, wf_ref, None, None, cold_ref, EPS, True)
        e32 = sum(R.producer_bound(*args, "r3" if r3 else "f32"))
        elp = sum(R.producer_bound(*args, "bf16")) + (R.producer_bound(*args, "r3")[1] if r3 else 0)     # out_hi: the 24-bit value rounded once more
        mu_err, rs_err = R.chain_errs(x1_ref, e32, EPS)
        cin = {"a": x1_ref, "wf": wf_ref, "st_in": R.stats(x1_ref), "colc": colc_ref, "cold": cold_ref, "eps": EPS, "hidden": H, "gelu": True}
        r = R.check_consumer(cin, y, ref=y_ref, a_err=elp, mu_err=mu_err, rs_err=rs_err, colc_err=H * R.U * wf_ref.double().abs().sum(1),
                             cold_err=H * R.U * ((c["beta2"].double()[None, :] * c["W2"].double()).abs().sum(1) + c["bias2"].double().abs()))
        print("chain tile %d H=%d M=%d r3=%d: %.3g of the bound" % (tile, H, M, r3, r["cons"]))
        assert r["cons"] <= 1.0, r


@pytest.mark.parametrize("H", [768, 1024])
@pytest.mark.parametrize("family", list(R.FAMILIES))
def test_statistics_regimes(dev, family, H):
    """The one-pass variance sq/H - mu^2 of ln_mean_rstd (csrc/common.h) where its cancellation term counts: |mean| / std up to 64, outlier
    columns, an all-zero row.  Tables carry NaN in their pad slots."""
    from cpt_amd import ops
    M, N, z = 77, 192, 38
    # consumer: rows of width K = H
    c = R.make_case(H + len(family), family, M, H, 64, N, z, device="cuda:0")
    for g in (True, False):
        cin = R.consumer_inputs(c, g)
        y = ops.gemm_ln_cons(_inside_nan(cin["a"]), cin["wf"], cin["st_in"], cin["colc"], cin["cold"], EPS, H, g)
        r = R.check_consumer(cin, y)
        print("regime %s H=%d consumer gelu=%d: %.3g of the bound" % (family, H, g, r["cons"]))
        assert r["cons"] <= 1.0, r
        if g:       # the all-zero row: gelu(cold) up to the kernels' erf approximation (1e-6 absolute) and the bf16 half ulp
            want = R.gelu(cin["cold"].double())
            assert bool(((y[z].double() - want).abs() <= R.GELU_ABS + R._half_ulp(want.abs() + R.GELU_ABS, 8)).all())
        else:       # ... exactly cold
            assert torch.equal(y[z], cin["cold"].to(torch.bfloat16))
    # LayerNorm-residual producer: residual rows of width N = hidden = 192, K = H
    p = R.make_case(H + 7 + len(family), family, M, N, H, None, z, device="cuda:0")
    pin = R.producer_inputs(p, True)
    out, out_lp, st = ops.gemm_ln_prod(_inside_nan(p["a"]), p["w"], p["bias"], _inside_nan(p["x0"]), p["st0"], p["g_in"], p["b_in"], EPS, N)
    r = R.check_producer(pin, {"out_f32": out, "out_bf16": out_lp, "st_out": st})
    print("regime %s H=%d producer: %s" % (family, H, " ".join("%s=%.3g" % kv for kv in r.items())))
    assert all(v <= 1.0 for v in r.values()), r
    acc = p["a"][z].double() @ p["w"].double().T
    want = acc + p["bias"].double() + p["b_in"].double()
    assert bool(((out[z].double() - want).abs() <= H * R.U * (p["a"][z].double().abs() @ p["w"].double().abs().T)).all())
    assert bool(torch.isfinite(out).all())
