"""CPU: the float64 reference, the bound and the planted defects of tests/_lnref.py, on every input family and shape class that
tests/test_gpu_ln_gemm_parity.py runs on the kernels.  What this file shows, without a GPU:
  * the reference is the operation: the folded consumer equals LayerNorm -> Linear -> erf GELU, the producer equals
    Linear + bias + LayerNorm(residual), both in float64 to 1e-11; fold matches its definition;
  * the bound is achievable: the fp32 emulation of the documented arithmetic stays within a quarter of it;
  * the bound is tight enough: every planted single defect breaks it (or, for a defect in the table a producer writes, the statistics check).

Input families: rows with |mean| / std in {0, 4, 64}, rows with four outlier columns at 30 std, and one all-zero row in every matrix.
A constant NON-zero row is left out on purpose: var = 0 up to rounding and rstd = 1 / sqrt(eps) multiplies the rounding error of the mean
by 10^6 -- ill-conditioned for any fp32 LayerNorm, one-pass or two-pass, so no bound from the inputs can hold on it."""
import pytest
import torch

import _lnref as R

M, ZERO_ROW = 5, 2
CASES = [(i, fam) for i in range(len(R.SHAPES)) for fam in R.FAMILIES]
# the ONE mutation that cannot apply at a width (at most one per case):
#   H = 768: 8 blocks = 8 slots, N padded to slots * 96 is N itself;  H = 200 is no legal consumer K (K % 64), so no consumer runs there
NOT_APPLICABLE = {768: {"inv_h_padded"}, 1024: set(), 200: {"mean_colc_kept"}}


def _case(i, fam):
    H, Kp, I = R.SHAPES[i]
    return R.make_case(100 + i, fam, M, H, Kp, I, ZERO_ROW)


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("i,fam", CASES)
def test_reference_is_the_operation(i, fam):
    c = _case(i, fam)
    H, eps = c["H"], c["eps"]
    # producer = Linear + bias + LayerNorm(residual) (torch's LayerNorm, float64)
    ref, st = R.producer(c["a"], c["w"], c["bias"], c["x0"], R.stats(c["x0"]), c["g_in"], c["b_in"], eps, H)
    ln = torch.nn.functional.layer_norm(c["x0"].double(), (H,), c["g_in"].double(), c["b_in"].double(), eps)
    comp = c["a"].double() @ c["w"].double().T + c["bias"].double() + ln
    assert _rel(ref, comp) <= 1e-11
    assert torch.equal(st, R.stats(ref)) and st.shape == (M, R.slots(H), 2)
    # the all-zero residual row: its LayerNorm is exactly b_in, everything finite
    lnz = R._residual(c["x0"], c["st0"], c["g_in"], c["b_in"], eps, H)
    assert torch.equal(lnz[ZERO_ROW], c["b_in"].double()) and bool(torch.isfinite(ref).all())
    if "W2" not in c:
        return
    # consumer, folded with UNROUNDED float64 weights on the statistics of its own A = LayerNorm -> Linear -> GELU
    a = c["x0"].to(torch.bfloat16)
    wf = c["gamma2"].double()[None, :] * c["W2"].double()
    colc, cold = wf.sum(1), c["W2"].double() @ c["beta2"].double() + c["bias2"].double()
    for g in (True, False):
        y = R.consumer(a, wf, R.stats(a), colc, cold, eps, H, g)
        yu = R.consumer_unfolded(a, c["W2"], c["gamma2"], c["beta2"], c["bias2"], eps, g)
        assert _rel(y, yu) <= 1e-11, (g, _rel(y, yu))
        assert bool(torch.isfinite(y).all())


@pytest.mark.parametrize("N,K,bias", [(1, 4, True), (7, 768, False), (768, 1024, True)])
def test_fold_matches_its_definition(N, K, bias):
    gen = torch.Generator().manual_seed(N + K)
    W, g, b = torch.randn((N, K), generator=gen) * 0.03, 1 + torch.randn(K, generator=gen) * 0.1, torch.randn(K, generator=gen) * 0.1
    bs = torch.randn(N, generator=gen) if bias else None
    wf, colc, cold = R.fold(W, g, b, bs)
    assert wf.dtype == torch.bfloat16 and colc.dtype == torch.float64
    prod = g[None, :] * W                                   # fp32 product, one rounding
    assert bool(((prod.double() - wf.double()).abs() <= R._half_ulp(prod.double(), 8)).all())      # nearest ...
    ties = (prod.double() - wf.double()).abs() == R._half_ulp(prod.double(), 8)
    assert bool(((R.bf16_bits(wf)[ties.numpy()] & 1) == 0).all())                                   # ... even
    assert torch.equal(colc, wf.double().sum(1))
    want = (W.double() * b.double()[None, :]).sum(1) + (bs.double() if bias else 0)
    assert float((cold - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("i,fam", CASES)
def test_emulation_within_a_quarter_of_the_bound(i, fam):
    r = R.emulation_ratios(_case(i, fam))
    worst = max(r, key=r.get)
    print("emulation %s %s: worst %.4f (%s)" % (R.SHAPES[i], fam, r[worst], worst))
    assert r[worst] <= 0.25, (worst, r[worst])


def _mutant_ratios(c, mut):
    out = {}
    for r3 in (False, True):
        for fr in (True, False):
            inp = R.producer_inputs(c, fr, r3)
            for k, v in R.check_producer(inp, R.ideal_producer(inp, mut, r3)).items():
                out["prod%s%s.%s" % ("3" if r3 else "", "_ln" if fr else "", k)] = v
    if "W2" in c:
        for g in (True, False):
            inp = R.consumer_inputs(c, g)
            out["cons%s" % ("_gelu" if g else "")] = R.check_consumer(inp, R.ideal_consumer(inp, mut))["cons"]
    return out


@pytest.mark.parametrize("i,fam", CASES)
def test_every_planted_defect_is_caught(i, fam):
    c = _case(i, fam)
    clean = _mutant_ratios(c, None)
    assert max(clean.values()) <= 1.0, clean               # the perfect kernel passes every check
    for mut in R.MUTATIONS:
        if mut in NOT_APPLICABLE[c["H"]]:
            continue
        r = _mutant_ratios(c, mut)
        broke = sorted(k for k, v in r.items() if not v <= 1.0)
        assert broke, "%s not caught at %s %s" % (mut, R.SHAPES[i], fam)
        if mut in R.STAT_MUTATIONS:
            assert any(k.endswith(".st_out") for k in broke), (mut, broke)


def test_not_applicable_list_is_minimal():
    assert all(len(v) <= 1 for v in NOT_APPLICABLE.values())
    for mut in R.MUTATIONS:
        assert sum(mut not in NOT_APPLICABLE[R.SHAPES[i][0]] for i, _ in CASES) >= 2, mut
    assert {H for H, _, _ in R.SHAPES} == set(NOT_APPLICABLE)
    assert len(R.MUTATIONS) == 11 and len(set(R.MUTATIONS)) == 11
