"""CPU: what keeps tests/test_gpu_fwd_regimes.py honest.

1. The case table.  ``plan()`` below restates the shape conditions by which cpt_model_fwd picks its launches (cpt_amd/csrc/cpt_abi.hip make_plan,
   panel_modes, pad_rows and the helpers they call, product build: every switch of csrc/switches.h at its default).  Every case of the GPU
   file's table names the plan fields it exists for; here each claim is checked against the restatement, and every value of every plan
   field must be reached by some case.  When a threshold moves in the library, the restatement is updated with it, the claims fail here, and
   the table is derived again.
2. The comparator (tests/_fwdcheck.py) on the tiny configuration in float64: the emulation as "kernel" passes, the reference passes with
   zero error, and four planted faults of the kind a launch can have are each caught by a wide margin.
"""
import math

import pytest
import torch

import _fwdcheck as FC
import test_gpu_fwd_regimes as R
from cpt_amd import config as cfgmod
from cpt_amd import synth
from oracle import cpt_oracle as O

TAIL_NONE, TAIL_BF16, TAIL_X3, TAIL_F32 = "NONE", "BF16", "X3", "F32"


# ---- restatement of the plan (product build) -------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return (a + b - 1) // b


def ffn_up_2pass_legal(M, N, K):            # csrc/gemm_ffn.hip: TM = 384, TN = 256
    return K in (768, 1024) and N % 256 == 0 and M >= 384


def ffn_up_2pass_preferred(M, N, K):        # csrc/gemm_ffn.hip; switch 16 (g_ffn_2pass_min_tiles) = 192
    return ffn_up_2pass_legal(M, N, K) and _cdiv(M, 384) * (N // 256) >= 192


def panel_eligible(M, N, K):                # csrc/gemm_prod.hip: TM = 128, TN = 192
    return M > 0 and M % 128 == 0 and N > 0 and N % 192 == 0 and K >= 512 and K % 256 == 0 and M * K * 2 <= 0x7fffffff


def qkv_attn3_eligible(L, heads, K):        # csrc/qkv_attn3.hip
    return 0 < L <= 128 and heads > 0 and heads % 3 == 0 and 96 <= K <= 768 and K % 32 == 0


def head_transform_splits(K):               # csrc/gemm.hip
    nt = K // 64
    return nt // 2 if nt >= 4 else 1


def rows_gemm_splits(K):                    # csrc/gemm.hip
    nt = K // 64
    if nt < 4:
        return 1
    S = nt // 2
    while S > 24 or nt % S:
        S -= 1
    return S


def panel_modes(attn_form, two_kernel, H, I, Me, fold):
    """cpt_abi.hip panel_modes with g_panel = g_panel_ffn_multi = g_rpanel = 1, g_lncons4 = 1 -> (panel, panel_ffn, rpanel)."""
    panel = bool(fold and (attn_form == 3 or two_kernel) and ffn_up_2pass_preferred(Me, I, H) and panel_eligible(Me, H, H)
                 and panel_eligible(Me, H, I))
    panel_ffn = panel          # (Me / 128 * (H / 192) <= 256 || g_panel_ffn_multi), the switch being 1
    rpanel = panel and panel_ffn and attn_form == 3
    return panel, panel_ffn, rpanel


def pad_rows(lp, attn_form, two_kernel, H, I, M):
    """cpt_abi.hip pad_rows."""
    if not lp or panel_modes(attn_form, two_kernel, H, I, M, True)[2]:
        return M
    Mp = _cdiv(M, 128) * 128
    while Mp <= M + M // 2:
        if panel_modes(attn_form, two_kernel, H, I, Mp, True)[2]:
            tp, tf = Mp // 128 * (H // 192), _cdiv(Mp, 384) * (I // 256)
            for t in (tp, tf):
                rounds = _cdiv(t, 256)
                if rounds >= 2 and t - 256 * (rounds - 1) < 128:
                    return M
            return Mp
        Mp += 128
    return M


def ln_cons_kernel(M, N, K, gelu, out_panel):
    """csrc/gemm.hip gemm_ln_cons, GEMM variant 3 (by shape), g_lncons4 = 1, g_qkv_2pass = 1: which kernel runs a LayerNorm-consumer GEMM
    (FFN up: gelu; the stand-alone QKV projection of the two-kernel form: not)."""
    if out_panel:
        return "2pass"
    t4 = _cdiv(M, 192) * (N // 256)
    r4 = _cdiv(t4, 256)
    t2 = _cdiv(M, 384) * (N // 256)
    r2 = _cdiv(t2, 256)
    fills_better = t4 * r2 * 10 >= t2 * r4 * 11
    pref = ffn_up_2pass_preferred(M, N, K)
    if pref and (gelu or t4 * 5 >= r4 * 256 * 4) and fills_better:
        return "lncons4"
    if gelu and pref:
        return "2pass"
    t128 = _cdiv(M, 128) * _cdiv(N, 192)
    if not gelu and t128 >= 1024:
        return "pipe128x192"
    if not gelu and pref and t2 * 5 >= r2 * 256 * 4:
        return "2pass"
    return "by tile"


def plan(case, output):
    """make_plan for one output of one case -> dict of the plan fields (and, below the plan, the kernels that depend on tile fill)."""
    cfg = R.config_of(case)
    H, I, heads = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads
    B, Lt, Li = case.B, case.Lt, case.Li
    L, M = Lt + Li, B * (Lt + Li)
    x3 = case.mode == "bf16x3"
    lp = case.mode == "bf16"
    f32 = case.mode == "fp32"
    fold = lp and case.fold
    mask3 = case.mask3
    all_logits = output == "all"
    all_rows = output in ("all", "bert")
    want_mask = output == "mask"
    want_cls = output in ("nsp", "bert")              # CPT_OUT_REL, or CPT_OUT_POOLED beside CPT_OUT_SEQ
    img_dim_pad = _cdiv(cfg.img_feature_dim, 64) * 64
    p = {}
    fuse_attn = lp and L <= 128 and H % 64 == 0 and not mask3
    p["attn_form"] = 0 if not fuse_attn else (3 if qkv_attn3_eligible(L, heads, H) else 1)
    p["two_kernel"] = bool(lp and not fuse_attn and not mask3 and L <= 288)
    Mw = pad_rows(lp, p["attn_form"], p["two_kernel"], H, I, M)
    p["Me"] = Mw if fold else M
    p["pad_rows"] = p["Me"] > M
    p["panel"], p["panel_ffn"], p["rpanel"] = panel_modes(p["attn_form"], p["two_kernel"], H, I, p["Me"], fold)
    p["x3a"] = bool(x3 and not mask3 and 0 < L <= 288 and H % 8 == 0)
    p["x3f"] = bool(x3 and I % 8 == 0 and I * 4 >= 3 * H * 2)
    p["pre_ln"] = bool(fold and not all_rows)
    p["img_split2"] = bool(lp and img_dim_pad >= 128 and img_dim_pad % 64 == 0 and 2 * B * Li <= M)
    hs = head_transform_splits(H)
    p["head_splits"] = hs if (lp and not all_logits and H % 64 == 0 and hs > 1 and hs * B <= M) else 0
    tail_ok = cfg.num_hidden_layers >= 2 and not all_rows and want_mask != want_cls
    p["tail"], p["tail_s1"], p["tail_s2"] = TAIL_NONE, 0, 0
    HI = max(H, I)
    if tail_ok and fold:
        s1, s2 = rows_gemm_splits(H), rows_gemm_splits(I)
        if H % 64 == 0 and I % 64 == 0 and max(s1 * B * HI, s2 * B * H) * 4 <= M * I * 2 and B * I * 2 <= M * H * 4:
            p["tail"], p["tail_s1"], p["tail_s2"] = TAIL_BF16, s1, s2
    elif tail_ok and p["x3a"] and p["x3f"]:
        s1, s2 = rows_gemm_splits(3 * H), rows_gemm_splits(3 * I)
        if (H % 64 == 0 and I % 64 == 0 and s1 <= 24 and s2 <= 24 and max(s1 * B * HI, s2 * B * H) * 4 <= M * I * 4
                and B * I * 6 <= M * 3 * H * 4 and B * 3 * H * 2 <= M * H * 4):
            p["tail"], p["tail_s1"], p["tail_s2"] = TAIL_X3, s1, s2
    elif tail_ok and f32:
        p["tail"] = TAIL_F32
    # below the plan (folded bf16 encoder only)
    if fold:
        p["ffn_up"] = ln_cons_kernel(p["Me"], I, H, True, p["panel"])
        p["qkv"] = ln_cons_kernel(p["Me"], 3 * H, H, False, False) if p["attn_form"] == 0 else "fused"
        if p["panel"]:
            p["producer_waves"] = 4 if p["Me"] // 128 * (H // 192) > 256 else 8       # csrc/gemm_prod.hip, g_prod_waves = 0: by tile count
    return p


ALL_CASES = [(c, o) for c in R.CASES for o in c.outputs]


def test_case_ids_are_unique_and_outputs_known():
    ids = [c.id for c in R.CASES]
    assert len(set(ids)) == len(ids)
    for c in R.CASES:
        assert c.outputs and set(c.outputs) <= {"mask", "all", "bert", "nsp"}, c.id
        assert "all" not in c.outputs or c.B <= 2, "%s: all-row logits at B <= 2 only (V = 30522)" % c.id


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_case_runs_the_plan_its_comment_claims(case):
    """``case.expect``: plan fields by name; a value is either the field's value for every output of the case, or a dict
    {output: value} for the fields that depend on the output flags (pre_ln, head_splits, tail, tail_s1, tail_s2)."""
    assert case.expect, "%s claims nothing" % case.id
    for o in case.outputs:
        p = plan(case, o)
        for k, v in case.expect.items():
            want = v.get(o, None) if isinstance(v, dict) else v
            if isinstance(v, dict) and o not in v:
                continue
            assert k in p, "%s: %s is not a field of this plan" % (case.id, k)
            assert p[k] == want, "%s, output %s: %s is %r, the table claims %r" % (case.id, o, k, p[k], want)


def test_every_plan_value_is_reached():
    reached = {}
    for c, o in ALL_CASES:
        for k, v in plan(c, o).items():
            reached.setdefault(k, set()).add(v)
    want = {
        "attn_form": {0, 1, 3},
        "two_kernel": {False, True},
        "pad_rows": {False, True},
        "panel": {False, True}, "panel_ffn": {False, True}, "rpanel": {False, True},
        "pre_ln": {False, True},
        "img_split2": {False, True},
        "head_splits": {0, head_transform_splits(768), head_transform_splits(1024)},
        "tail": {TAIL_NONE, TAIL_BF16, TAIL_X3, TAIL_F32},
        "tail_s1": {0, rows_gemm_splits(768), rows_gemm_splits(1024), rows_gemm_splits(3 * 768)},
        "tail_s2": {0, rows_gemm_splits(3072), rows_gemm_splits(4096), rows_gemm_splits(3 * 3072)},
        "x3a": {False, True},
        # x3f is off only outside the bf16x3 mode: inside it, it needs an intermediate size below 1.5 x hidden, which no Oscar model has
        "x3f": {False, True},
        # below the plan: the LayerNorm-consumer kernels by tile fill, the panel producers' wave shape by tile count
        "ffn_up": {"by tile", "2pass", "lncons4"},
        "qkv": {"fused", "by tile", "2pass", "lncons4", "pipe128x192"},
        "producer_waves": {4, 8},
    }
    for k, vals in want.items():
        assert vals <= reached.get(k, set()), "%s: no case reaches %s" % (k, sorted(vals - reached.get(k, set()), key=str))
    # x3a off INSIDE the bf16x3 mode, with x3f on (3-D mask; L > 288), and the tail off there
    x3_off = [(c.id, o) for c, o in ALL_CASES if c.mode == "bf16x3" and not plan(c, o)["x3a"] and plan(c, o)["x3f"]]
    assert any(c.mask3 for c in R.CASES if (c.id, "mask") in x3_off) and any(c.Lt + c.Li > 288 for c in R.CASES if (c.id, "mask") in x3_off)
    # both sides of pad_rows's "a further round is at least half full" rule: refused, and taken with a second round
    refused = [c.id for c, o in ALL_CASES if c.mode == "bf16" and c.fold and not plan(c, o)["pad_rows"] and not plan(c, o)["panel"]
               and c.B * (c.Lt + c.Li) > 7680 and c.Lt + c.Li <= 128 and not c.mask3 and R.config_of(c).hidden_size == 768]
    taken2 = [c.id for c, o in ALL_CASES if plan(c, o)["pad_rows"] and plan(c, o)["Me"] // 128 * 4 > 256]
    assert refused and taken2, (refused, taken2)
    # every mode runs every output
    for mode in ("bf16", "fp32", "bf16x3"):
        assert {o for c, o in ALL_CASES if c.mode == mode} == {"mask", "all", "bert", "nsp"}, mode


def test_boundaries_are_visited_from_both_sides():
    """The smallest batch on each side of every row-count boundary of the RefCOCO shape (L = 70 + 50), by the restatement itself."""
    def p(B, Lt=70, Li=50, **kw):
        return plan(R.Case("probe", "bf16", "base3", B, Lt, Li, ("mask",), kw.get("mask3", False), True, {}), "mask")
    first_pad = min(B for B in range(1, 64) if p(B)["pad_rows"])
    first_direct = min(B for B in range(1, 200) if p(B)["rpanel"] and not p(B)["pad_rows"])
    first_refused = min(B for B in range(first_direct + 1, 200) if not p(B)["panel"])
    have = {c.B for c in R.CASES if c.mode == "bf16" and c.fold and (c.Lt, c.Li) == (70, 50) and not c.mask3 and c.cfg == "base3"}
    assert (first_pad, first_direct, first_refused) == (33, 64, 68)
    assert {first_pad - 1, first_pad, first_direct - 1, first_direct, first_refused - 1, first_refused} <= have
    assert p(51)["Me"] == 6144 and p(52)["Me"] == 6272 and {51, 52} <= have
    # L: 128 | 129 and 288 | 289
    Ls = {c.Lt + c.Li for c in R.CASES if c.mode == "bf16" and c.fold}
    assert {128, 129, 288, 289} <= Ls


# ---- comparator self-test: tiny configuration, float64 ---------------------------------------------------------------------------------
B_TINY, LT_TINY, LI_TINY = 10, 20, 6          # 260 rows: the rows of the second 128-row tile are rows 128..255


def _forward(sd, cd, b, fault=None):
    """The oracle's forward (O.bert_img_forward + O.lm_head + the relation head) written out layer by layer, so that a fault can be planted
    where a launch could have it.  fault None reproduces the oracle bit for bit (asserted below)."""
    nl = cd["num_hidden_layers"]
    eps = cd["layer_norm_eps"]
    ext = O.extended_mask(b["attention_mask"])
    x = O.text_embeddings(sd, cd, b["input_ids"], b["segment_ids"])
    x = torch.cat((x, O.image_embeddings(sd, cd, b["img_feats"])), 1)
    Bn, L, H = x.shape

    def resid(t):
        # the 3-byte residual stream (csrc/common.h r3_encode) without its low byte is a bf16 tensor
        return t.to(torch.bfloat16).to(t.dtype) if fault == "residual low byte" else t
    hiddens = [x]
    for i in range(nl):
        p = "bert.encoder.layer.%d." % i
        ctx = O.self_attention(sd, cd, x, ext, p + "attention.self.", None, i)
        a = O._linear(ctx, sd, p + "attention.output.dense")
        a = O.layer_norm(a + resid(x), sd[p + "attention.output.LayerNorm.weight"], sd[p + "attention.output.LayerNorm.bias"], eps)
        h = O.gelu_erf(O._linear(a, sd, p + "intermediate.dense"))
        o = O._linear(h, sd, p + "output.dense")
        if fault == "k slice" and i == nl - 1:
            # one 64-wide K-slice of the FFN-down product missing for the rows of the second 128-row tile
            hs, ws = O._lp(h).reshape(Bn * L, -1)[128:256, 64:128], O._lp(sd[p + "output.dense.weight"])[:, 64:128]
            o = o.reshape(Bn * L, H).clone()
            o[128:256] -= hs @ ws.t()
            o = o.reshape(Bn, L, H)
        x = O.layer_norm(o + resid(a), sd[p + "output.LayerNorm.weight"], sd[p + "output.LayerNorm.bias"], eps)
        hiddens.append(x)
    ar = torch.arange(Bn)
    rows = x[ar, b["mask_token_pos"]]
    cls_rows = x[:, 0]
    if fault == "tail row":
        # the last layer on the head's rows only: one row never replaced by the last layer's result
        rows, cls_rows = rows.clone(), cls_rows.clone()
        rows[3] = hiddens[-2][3, b["mask_token_pos"][3]]
        cls_rows[3] = hiddens[-2][3, 0]
    pooled = torch.tanh(O._linear(cls_rows, sd, "bert.pooler.dense"))
    out = dict(mask_logits=O.lm_head(sd, cd, rows), seq=x, pooled=pooled, rel=O.relation_head(sd, pooled))
    if fault == "swapped sequences":
        perm = list(range(Bn))
        perm[2], perm[7] = 7, 2
        out = {k: v[perm] for k, v in out.items()}
    return out


@pytest.fixture(scope="module")
def tiny():
    cfg = cfgmod.tiny()
    sd = {k: v.double() for k, v in synth.init_state_dict(cfg, 77, head="pretrain").items()}
    sd["cls.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"]
    for k in ("bias", "transform.dense.weight", "transform.dense.bias", "transform.LayerNorm.weight", "transform.LayerNorm.bias"):
        sd["cls." + k] = sd["cls.predictions." + k]
    b = synth.make_batch(B_TINY, cfg, seed=6, max_seq_len=LT_TINY, img_seq_len=LI_TINY, vary_regions=True)
    b["img_feats"] = b["img_feats"].double()
    cd = cfg.to_dict()
    with torch.no_grad():
        ref = _forward(sd, cd, b)
        with O.emulate_bf16():
            emu = _forward(sd, cd, b)
    return sd, cd, b, ref, emu


def test_written_out_forward_is_the_oracle(tiny):
    """... and the shared encoder pass of the GPU file (R.oracle_outputs) equals the three oracle entry points it stands for."""
    sd, cd, b, ref, emu = tiny
    with torch.no_grad():
        for on, mine in ((False, ref), (True, emu)):
            with O.emulate_bf16(on):
                seq, pooled = O.bert_img_forward(sd, cd, b["input_ids"], b["segment_ids"], b["attention_mask"], img_feats=b["img_feats"])
                logits = O.rec_mlm_cpt_forward(sd, cd, b["input_ids"], b["segment_ids"], b["attention_mask"], img_feats=b["img_feats"],
                                               mask_rows_only=b["mask_token_pos"])[0]
                allr = O.rec_mlm_cpt_forward(sd, cd, b["input_ids"], b["segment_ids"], b["attention_mask"], img_feats=b["img_feats"])[0]
                rel = O.nsp_cpt_scores(sd, cd, b["input_ids"], b["segment_ids"], b["attention_mask"], b["img_feats"])
                shared = R.oracle_outputs(sd, sd, cd, b, ("mask", "all", "bert", "nsp"), on)
            assert torch.equal(seq, mine["seq"]) and torch.equal(pooled, mine["pooled"])
            assert torch.equal(logits, mine["mask_logits"]) and torch.equal(rel, mine["rel"])
            assert torch.equal(shared["seq"], seq) and torch.equal(shared["pooled"], pooled) and torch.equal(shared["rel"], rel)
            assert torch.equal(shared["mask_logits"], logits) and torch.equal(shared["all_logits"], allr)
    assert not torch.equal(ref["seq"], emu["seq"])


def test_reference_and_emulation_pass(tiny):
    sd, cd, b, ref, emu = tiny
    rows = FC.check("bf16", ref, ref, emu, "reference as kernel")
    assert all(r["ok"] and r["rel"] == 0.0 and r["row_rel"] == 0.0 for r in rows) and len(rows) == len(ref)
    rows = FC.check("bf16", emu, ref, emu, "emulation as kernel")
    assert all(r["ok"] for r in rows) and len(rows) == len(ref)
    assert all(abs(FC.ratio(r) - 1.0) < 1e-12 and abs(FC.ratio(r, True) - 1.0) < 1e-12 for r in rows)
    for mode in ("fp32", "bf16x3"):
        assert all(r["ok"] for r in FC.check(mode, ref, ref, None, "reference as kernel"))


# fault -> the outputs on which it must be caught by a wide margin under the stand-in constants, and whether the MEASURED constants of
# _fwdcheck catch it too.  The residual stream without its low byte is a design of lower accuracy, not a misplaced sum: its error is of the
# size of the bf16 design's own (kernel-to-emulation ratio 3.3 on the sequence output here, about 1.5 at Oscar-base width with three
# layers), so a constant that leaves room for summation order (C_FWD) cannot be relied on to tell the two apart; the stand-ins can.
STAND_IN = dict(C_FWD=1.5, FLOOR_FWD=0.0)
FAULTS = [
    ("swapped sequences", ("mask_logits", "seq"), True),
    ("k slice", ("mask_logits", "seq", "pooled", "rel"), True),
    ("tail row", ("mask_logits", "pooled", "rel"), True),
    ("residual low byte", ("seq",), False),
]
MARGIN = 2.0          # "by a wide margin": the figure that catches the fault is at least twice its bound


@pytest.mark.parametrize("fault,outputs,measured_too", FAULTS, ids=[f[0].replace(" ", "_") for f in FAULTS])
def test_planted_fault_is_caught(tiny, monkeypatch, fault, outputs, measured_too):
    sd, cd, b, ref, emu = tiny
    with torch.no_grad(), O.emulate_bf16():
        got = _forward(sd, cd, b, fault)
    if measured_too:
        rows = {r["name"]: r for r in FC.compare("bf16", got, ref, emu)}
        print("\nmeasured constants\n" + FC.table(list(rows.values()), fault))
        with pytest.raises(AssertionError):
            FC.check("bf16", got, ref, emu, fault)
        assert all(not rows[name]["ok"] for name in outputs), fault
    for k, v in STAND_IN.items():
        monkeypatch.setattr(FC, k, v)
    assert all(r["ok"] for r in FC.check("bf16", emu, ref, emu, "emulation as kernel"))
    rows = {r["name"]: r for r in FC.compare("bf16", got, ref, emu)}
    print("\nstand-in constants\n" + FC.table(list(rows.values()), fault))
    with pytest.raises(AssertionError):
        FC.check("bf16", got, ref, emu, fault)
    for name in outputs:
        r = rows[name]
        assert not r["ok"], (fault, name)
        assert max(r["rel"] / r["bound"], r["row_rel"] / r["row_bound"]) >= MARGIN, (fault, name, r)
    if fault == "tail row":
        # one row of ten: the row figure sees it far better than the whole-tensor figure
        r = rows["mask_logits"]
        assert r["row"] == 3 and r["row_rel"] / r["row_bound"] > 2 * r["rel"] / r["bound"]


def test_one_bad_row_is_caught_by_the_row_figure_alone(tiny):
    """One wrong row among thousands: the whole-tensor figure stays inside its bound, the worst-row figure does not."""
    sd, cd, b, ref, emu = tiny
    n = 8000
    g = torch.Generator().manual_seed(1)
    r = torch.randn(n, 64, generator=g, dtype=torch.float64)
    e = r + 1e-3 * torch.randn(n, 64, generator=g, dtype=torch.float64)
    k = r + 1e-3 * torch.randn(n, 64, generator=g, dtype=torch.float64)
    k[4321] = 1.2 * r[4321]
    row = FC.compare("bf16", {"seq": k}, {"seq": r}, {"seq": e})[0]
    assert row["rel"] <= row["bound"] and row["row"] == 4321 and row["row_rel"] > MARGIN * row["row_bound"] and not row["ok"]


def test_nan_missing_and_extra_outputs_fail(tiny):
    sd, cd, b, ref, emu = tiny
    got = {k: v.clone() for k, v in emu.items()}
    got["seq"][1, 2, 3] = float("nan")
    row = [r for r in FC.compare("bf16", got, ref, emu) if r["name"] == "seq"][0]
    assert not row["ok"] and row["row"] == 1 * (LT_TINY + LI_TINY) + 2 and math.isinf(row["row_rel"])
    got = {k: v for k, v in emu.items() if k != "pooled"}
    assert [r["name"] for r in FC.compare("bf16", got, ref, emu) if not r["ok"]] == ["pooled"]
    with pytest.raises(ValueError):
        FC.compare("bf16", dict(emu, other=emu["seq"]), ref, emu)
    with pytest.raises(ValueError):
        FC.compare("bf16", emu, ref, None)
    # the absolute band of the logits holds on its own
    got = {k: v.clone() for k, v in ref.items()}
    got["mask_logits"][0, 0] += 0.05
    assert [r["name"] for r in FC.compare("fp32", got, ref) if not r["ok"]] == ["mask_logits"]
