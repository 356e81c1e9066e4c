"""GPU: the inference forward (cpt_model_fwd through REC_MLM_CPT, its BertImgModel and NSPCPT) against the float64 oracle on the device, at
the shapes where the forward's plan (cpt_amd/csrc/cpt_abi.hip make_plan) and the kernels below it change.

Each case runs the outputs it lists -- every output asks for a different plan:
  mask   [MASK]-row logits      tail on the [MASK] rows, pre_ln, head_splits
  bert   sequence output + pooled, every row, final LayerNorm applied, no tail
  nsp    relation scores alone (NSPCPT)   tail on the [CLS] rows
  all    all-row logits (B <= 2: V = 30522)   head_splits 0
and checks each with tests/_fwdcheck.py: whole tensor and worst row, fixed bounds in fp32 / bf16x3,
``rel_kernel <= C_FWD * rel_emulation + FLOOR_FWD`` in bf16 against the oracle's bf16 design emulation.  The reference is ONE float64 encoder
pass per case (O.bert_img_forward) with the heads of O.rec_mlm_cpt_forward and O.nsp_cpt_scores behind it; tests/test_fwd_regimes_cpu.py
asserts that this equals the three entry points bit for bit, and checks every ``expect`` below against a restatement of make_plan.

Before every measured bf16 run the engine's forward workspace is filled with 0xFF (NaN in every format): a read of a padding row, or of
anything a launch should have written first, shows up against the reference.
"""
import collections
import time

import pytest
import torch

import _fwdcheck as FC
from cpt_amd import config as cfgmod
from cpt_amd import synth
from oracle import cpt_oracle as O

pytestmark = pytest.mark.gpu
SEED = 4321

# id, compute mode, model ("base3": Oscar-base width, 3 layers; "large2": Oscar-large width, 2 layers), B, Lt, Li (0: text only), outputs,
# 3-D attention mask, LayerNorm fold (bf16), expect = the plan fields the case is there for (checked by tests/test_fwd_regimes_cpu.py).
Case = collections.namedtuple("Case", "id mode cfg B Lt Li outputs mask3 fold expect")


def _c(id, mode, cfg, B, Lt, Li, outputs, expect, mask3=False, fold=True):
    return Case(id, mode, cfg, B, Lt, Li, tuple(outputs.split()), mask3, fold, expect)


T_BF16 = {"mask": "BF16", "nsp": "BF16", "bert": "NONE", "all": "NONE"}
T_X3 = {"mask": "X3", "nsp": "X3", "bert": "NONE", "all": "NONE"}
T_F32 = {"mask": "F32", "nsp": "F32", "bert": "NONE", "all": "NONE"}
PRE = {"mask": True, "nsp": True, "bert": False, "all": False}
HS6 = {"mask": 6, "nsp": 6, "bert": 6, "all": 0}

CASES = [
    # ---- bf16, LayerNorm folded, the RefCOCO shape L = 70 + 50 (M = 120 B rows) ----
    # 120 rows, below one 128-row tile: fused (sequence, three heads) attention, row-major 3-byte stream, FFN-up by tile; every output, all-row logits too
    _c("b1", "bf16", "base3", 1, 70, 50, "mask bert nsp all", dict(attn_form=3, two_kernel=False, Me=120, panel=False, rpanel=False, pre_ln=PRE,
                                                                  head_splits=HS6, tail=T_BF16, tail_s1={"mask": 6, "nsp": 6}, tail_s2={"mask": 24, "nsp": 24},
                                                                  img_split2=True, ffn_up="by tile")),
    # 240 rows: all-row logits over two row tiles (head_splits 0, the plain transform GEMM + LayerNorm on 240 head rows)
    _c("b2", "bf16", "base3", 2, 70, 50, "all", dict(Me=240, panel=False, head_splits=0, pre_ln=False, tail="NONE")),
    # 480 rows: configs[2]'s per-GPU share
    _c("b4", "bf16", "base3", 4, 70, 50, "mask bert nsp", dict(Me=480, panel=False, tail=T_BF16, pre_ln=PRE)),
    # 3840 rows: the largest row count that is NOT padded (5760 = 1.5 x 3840 rows would make 15 x 12 = 180 FFN-up tiles < 192)
    _c("b32", "bf16", "base3", 32, 70, 50, "mask bert nsp", dict(Me=3840, pad_rows=False, panel=False, rpanel=False, ffn_up="by tile")),
    # 3960 rows: the first padded batch, -> 5888 rows = 46 row tiles, 16 x 12 = 192 FFN-up tiles; the full panel mode on padded rows
    _c("b33", "bf16", "base3", 33, 70, 50, "mask bert nsp", dict(Me=5888, pad_rows=True, panel=True, panel_ffn=True, rpanel=True, ffn_up="2pass",
                                                                producer_waves=8, tail=T_BF16)),
    # 6120 -> 6144 rows = 16 FFN-up tiles of 384 exactly; 6240 -> 6272 rows: the 17th FFN-up row tile hangs over the padded matrix
    _c("b51", "bf16", "base3", 51, 70, 50, "mask bert", dict(Me=6144, pad_rows=True, rpanel=True)),
    _c("b52", "bf16", "base3", 52, 70, 50, "mask nsp", dict(Me=6272, pad_rows=True, rpanel=True)),
    # 7560 -> 7680 rows: the bench shape's row count reached by padding one sequence's worth
    _c("b63", "bf16", "base3", 63, 70, 50, "mask bert nsp", dict(Me=7680, pad_rows=True, rpanel=True, producer_waves=8)),
    # 7680 rows: the bench shape, rpanel direct (no padding): 240 producer tiles and 240 FFN-up tiles, one round
    _c("b64", "bf16", "base3", 64, 70, 50, "mask bert nsp", dict(Me=7680, pad_rows=False, panel=True, panel_ffn=True, rpanel=True, ffn_up="2pass",
                                                                producer_waves=8, tail=T_BF16, pre_ln=PRE)),
    # 8040 -> 8064 rows: the last padded batch of the first round (252 tiles of either shape, the round all but full)
    _c("b67", "bf16", "base3", 67, 70, 50, "mask", dict(Me=8064, pad_rows=True, rpanel=True, producer_waves=8)),
    # 8160 rows: padding REFUSED (8192 rows = 256 producer tiles but 22 x 12 = 264 FFN-up tiles: a second round for 8 of them) -> row-major kernels; the FFN-up's
    # 384 x 256 tiles fill their rounds worse than the 4-wave kernel's 192 x 256 ones (264 = 52 % of two rounds against 516 = 67 % of three) -> lncons4
    _c("b68", "bf16", "base3", 68, 70, 50, "mask bert", dict(Me=8160, pad_rows=False, panel=False, rpanel=False, ffn_up="lncons4")),
    # 12360 -> 12416 rows: padding TAKEN with a second round (388 producer tiles, 396 FFN-up tiles: the second round is more than half full);
    # 4-wave producer on padded rows.  [MASK] logits only
    _c("b103", "bf16", "base3", 103, 70, 50, "mask", dict(Me=12416, pad_rows=True, rpanel=True, producer_waves=4)),
    # 19200 rows: 600 producer tiles = three rounds (4-wave producer), panel_ffn over several rounds.  [MASK] logits only
    _c("b160", "bf16", "base3", 160, 70, 50, "mask", dict(Me=19200, pad_rows=False, rpanel=True, panel_ffn=True, producer_waves=4)),
    # ---- L = 128 exactly (78 + 50): 8320 rows = 65 row tiles but 21.67 FFN-up tiles of 384: the last one hangs over the matrix ----
    _c("L128_b65", "bf16", "base3", 65, 78, 50, "mask bert nsp", dict(attn_form=3, two_kernel=False, Me=8320, pad_rows=False, rpanel=True)),
    # ---- L = 129 (79 + 50): the two-kernel form.  16512 rows = 129 row tiles: the stand-alone attention kernel writes the ctx panel; the residual
    # stream stays row-major (rpanel needs attention form 3), so nothing is ever padded beyond L = 128; QKV projection through the 128 x 192 tiles
    # at two workgroups per CU (129 x 16 = 2064 tiles) ----
    _c("L129_b128", "bf16", "base3", 128, 79, 50, "mask bert", dict(attn_form=0, two_kernel=True, Me=16512, pad_rows=False, panel=True, panel_ffn=True,
                                                                   rpanel=False, qkv="pipe128x192", producer_waves=4)),
    _c("L129_b3", "bf16", "base3", 3, 79, 50, "mask nsp", dict(attn_form=0, two_kernel=True, Me=387, panel=False, qkv="by tile")),
    # ---- L = 210 (165 + 45), the GQA shape: the stand-alone QKV projection and the FFN-up walk through their kernels as the rows grow.  pad_rows pads
    # towards rpanel only, which needs attention form 3: beyond L = 128 nothing is padded, and the panel mode needs 210 B to be a multiple of 128 ----
    # 6720 rows: QKV by tile (18 x 9 = 162 two-pass tiles < 192), FFN-up on the two-pass kernel (216 tiles)
    _c("L210_b32", "bf16", "base3", 32, 165, 45, "mask", dict(two_kernel=True, Me=6720, panel=False, qkv="by tile", ffn_up="2pass")),
    # 8610 rows: QKV on the GELU-less two-pass kernel (23 x 9 = 207 tiles, 81 % of a round), FFN-up on the 4-wave kernel
    _c("L210_b41", "bf16", "base3", 41, 165, 45, "mask", dict(two_kernel=True, Me=8610, panel=False, qkv="2pass", ffn_up="lncons4")),
    # 10920 rows: QKV on the 128 x 192 tiles at two workgroups per CU (86 x 12 = 1032 tiles >= 1024)
    _c("L210_b52", "bf16", "base3", 52, 165, 45, "mask", dict(two_kernel=True, Me=10920, panel=False, qkv="pipe128x192", ffn_up="lncons4")),
    # 13230 rows: no multiple of 128, not padded -> row-major; QKV on the 4-wave kernel.  13440 rows = 105 row tiles: ctx / FFN panels on, rpanel off
    _c("L210_b63", "bf16", "base3", 63, 165, 45, "mask nsp", dict(two_kernel=True, Me=13230, pad_rows=False, panel=False, qkv="lncons4", ffn_up="2pass")),
    _c("L210_b64", "bf16", "base3", 64, 165, 45, "mask bert", dict(two_kernel=True, Me=13440, pad_rows=False, panel=True, panel_ffn=True, rpanel=False,
                                                                  qkv="lncons4", ffn_up="2pass", producer_waves=4)),
    # ---- L = 288 | 289 at small B: the last length of the two-kernel form (MFMA attention kernel), and the first beyond it (row-major ctx, generic attention) ----
    _c("L288_b3", "bf16", "base3", 3, 238, 50, "mask bert nsp", dict(attn_form=0, two_kernel=True, Me=864, panel=False)),
    _c("L289_b3", "bf16", "base3", 3, 239, 50, "mask bert nsp", dict(attn_form=0, two_kernel=False, Me=867, panel=False, tail=T_BF16)),
    # ---- more regions than text, 28 + 50: the region projection without its K split (2 B Li > B L) ----
    _c("Li_gt_Lt_b5", "bf16", "base3", 5, 28, 50, "mask bert", dict(img_split2=False, attn_form=3, Me=390)),
    # ---- text only (img_feats None): no region launches; at 64 x 120 the text embedding launch alone writes the panel-layout residual stream ----
    _c("text_b4", "bf16", "base3", 4, 70, 0, "mask bert nsp", dict(img_split2=True, attn_form=3, Me=280, panel=False)),
    _c("text_b64", "bf16", "base3", 64, 120, 0, "mask", dict(Me=7680, rpanel=True)),
    # ---- 3-D attention mask: the generic attention kernel, no fused form, no panel -- also at the bench shape's row count ----
    _c("mask3_b4", "bf16", "base3", 4, 70, 50, "mask bert nsp", dict(attn_form=0, two_kernel=False, Me=480, panel=False), mask3=True),
    _c("mask3_b64", "bf16", "base3", 64, 70, 50, "mask", dict(attn_form=0, two_kernel=False, Me=7680, pad_rows=False, panel=False, rpanel=False,
                                                             ffn_up="2pass", qkv="by tile"), mask3=True),
    # ---- Oscar-large width (H = 1024, 16 heads, I = 4096): attention form 1 (heads % 3 != 0), 11 statistics parts in 12 slots, no panel (1024 % 192 != 0),
    # head_splits 8, tail splits 8 / 16.  B = 36: 4320 rows = 12 x 16 = 192 FFN-up tiles, the first shape of the two-pass kernel (75 % of a round; the 4-wave
    # kernel's 368 tiles fill 72 % of two); B = 52: 6240 rows = 17 x 16 = 272 tiles (53 % of two rounds) against 33 x 16 = 528 (69 % of three) -> lncons4 ----
    _c("large_b3", "bf16", "large2", 3, 70, 50, "mask bert nsp", dict(attn_form=1, two_kernel=False, Me=360, panel=False, head_splits={"mask": 8},
                                                                     tail=T_BF16, tail_s1={"mask": 8, "nsp": 8}, tail_s2={"mask": 16, "nsp": 16}, ffn_up="by tile")),
    _c("large_b36", "bf16", "large2", 36, 70, 50, "mask", dict(attn_form=1, Me=4320, panel=False, ffn_up="2pass")),
    _c("large_b52", "bf16", "large2", 52, 70, 50, "mask nsp", dict(attn_form=1, Me=6240, pad_rows=False, panel=False, ffn_up="lncons4")),
    # ---- bf16 with the fold off (engine.fold_ln = False): the unfolded bf16 encoder -- no tail, no pre_ln, no panel, never padded ----
    _c("nofold_b4", "bf16", "base3", 4, 70, 50, "mask bert nsp", dict(Me=480, pre_ln=False, tail="NONE", panel=False, attn_form=3), fold=False),
    _c("nofold_b64", "bf16", "base3", 64, 70, 50, "mask bert nsp", dict(Me=7680, pre_ln=False, tail="NONE", panel=False, rpanel=False, attn_form=3), fold=False),
    _c("nofold_b33", "bf16", "base3", 33, 70, 50, "mask", dict(Me=3960, pad_rows=False, panel=False), fold=False),
    # ---- fp32: TAIL_F32 on [MASK] and on [CLS] rows; no fused attention, no region K split, head_splits 0 ----
    _c("fp32_b1", "fp32", "base3", 1, 70, 50, "mask all", dict(attn_form=0, two_kernel=False, tail={"mask": "F32", "all": "NONE"}, head_splits=0, img_split2=False)),
    _c("fp32_b4", "fp32", "base3", 4, 70, 50, "mask bert nsp", dict(tail=T_F32, Me=480, x3a=False, x3f=False)),
    _c("fp32_b33", "fp32", "base3", 33, 70, 50, "mask bert nsp", dict(tail=T_F32, Me=3960, pad_rows=False)),
    _c("fp32_b64", "fp32", "base3", 64, 70, 50, "mask bert nsp", dict(tail=T_F32, Me=7680, panel=False)),
    _c("fp32_L210_b3", "fp32", "base3", 3, 165, 45, "mask bert nsp", dict(tail=T_F32, Me=630)),
    # ---- bf16x3: TAIL_X3 (K-split row GEMMs on split operands, 18 / 24 splits), x3a + x3f; x3a off (and with it the tail) beyond L = 288 and under a 3-D mask ----
    _c("x3_b1", "bf16x3", "base3", 1, 70, 50, "mask all", dict(x3a=True, x3f=True, tail={"mask": "X3", "all": "NONE"}, head_splits=0)),
    _c("x3_b4", "bf16x3", "base3", 4, 70, 50, "mask bert nsp", dict(x3a=True, x3f=True, tail=T_X3, tail_s1={"mask": 18, "nsp": 18}, tail_s2={"mask": 24, "nsp": 24})),
    _c("x3_b33", "bf16x3", "base3", 33, 70, 50, "mask bert nsp", dict(x3a=True, x3f=True, tail=T_X3, Me=3960, pad_rows=False)),
    _c("x3_b64", "bf16x3", "base3", 64, 70, 50, "mask bert nsp", dict(x3a=True, x3f=True, tail=T_X3, Me=7680, panel=False)),
    _c("x3_L210_b3", "bf16x3", "base3", 3, 165, 45, "mask bert nsp", dict(x3a=True, x3f=True, tail=T_X3)),
    _c("x3_L289_b3", "bf16x3", "base3", 3, 239, 50, "mask bert nsp", dict(x3a=False, x3f=True, tail="NONE")),
    _c("x3_mask3_b4", "bf16x3", "base3", 4, 70, 50, "mask bert nsp", dict(x3a=False, x3f=True, tail="NONE"), mask3=True),
]


def config_of(case):
    if case.cfg == "base3":
        return cfgmod.oscar_base(num_hidden_layers=3)
    return cfgmod.oscar_large(num_hidden_layers=2)


def make_inputs(case, cfg):
    """CPU batch of the case: synth.make_batch with ragged region counts; Li = 0 drops the regions; mask3 builds a [B, L, L] mask that differs
    from row to row (odd query rows do not see the first region)."""
    b = synth.make_batch(case.B, cfg, seed=1000 + case.B, max_seq_len=case.Lt, img_seq_len=max(case.Li, 1), vary_regions=True)
    if case.Li == 0:
        b["attention_mask"] = b["attention_mask"][:, :case.Lt].contiguous()
        b["img_feats"] = None
    if case.mask3:
        L = case.Lt + case.Li
        m3 = b["attention_mask"][:, None, :].repeat(1, L, 1)
        m3[:, 1::2, case.Lt] = 0
        b["attention_mask"] = m3.contiguous()
    return b


def oracle_outputs(sd_cpt, sd_nsp, cd, b, outputs, emulate):
    """One encoder pass (O.bert_img_forward) and the heads of O.rec_mlm_cpt_forward / O.nsp_cpt_scores on it, in the dtype and on the device of the
    state dicts; under O.emulate_bf16() when ``emulate``."""
    with torch.no_grad(), O.emulate_bf16(emulate):
        seq, pooled = O.bert_img_forward(sd_cpt, cd, b["input_ids"], b["segment_ids"], b["attention_mask"], img_feats=b["img_feats"])
        out = {}
        if "mask" in outputs:
            out["mask_logits"] = O.lm_head(sd_cpt, cd, seq[torch.arange(seq.size(0), device=seq.device), b["mask_token_pos"]])
        if "all" in outputs:
            out["all_logits"] = O.lm_head(sd_cpt, cd, seq)
        if "bert" in outputs:
            out["seq"], out["pooled"] = seq, pooled
        if "nsp" in outputs:
            out["rel"] = O.relation_head(sd_nsp, pooled)
    return out


def build_env(dev):
    built = {}

    def get(name):
        """(REC_MLM_CPT, NSPCPT, float64 state of the first, float64 state of the second): one set per model width, built once.  The two models
        hold the same encoder weights (same seed, same draw order), so one oracle pass serves both."""
        if name not in built:
            from cpt_amd.modeling_bert import BertImgForPreTraining
            from cpt_amd.modeling_rec import REC_MLM_CPT
            from cpt_amd.modeling_vcr import NSPCPT
            cfg = cfgmod.oscar_base(num_hidden_layers=3) if name == "base3" else cfgmod.oscar_large(num_hidden_layers=2)
            sd = synth.init_state_dict(cfg, SEED, head="cpt")
            sdp = synth.init_state_dict(cfg, SEED, head="pretrain")
            assert all(torch.equal(sd[k], sdp[k]) for k in sd if k.startswith("bert."))
            m = REC_MLM_CPT(cfg)
            m.load_state_dict(sd)
            m.tie_weights()
            m.to(dev).eval()
            pre = BertImgForPreTraining(cfg)
            pre.load_state_dict(sdp)
            pre.tie_weights()
            nsp = NSPCPT(cfg)
            nsp.copy_from_pretraining_model(pre)
            nsp.to(dev).eval()
            sd64 = {k: v.to(dev, torch.float64) for k, v in sd.items()}
            sd64["cls.decoder.weight"] = sd64["bert.embeddings.word_embeddings.weight"]
            nsp64 = {k: sdp[k].to(dev, torch.float64) for k in ("cls.seq_relationship.weight", "cls.seq_relationship.bias")}
            built[name] = (m, nsp, sd64, nsp64)
        return built[name]
    return dev, get


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return build_env(torch.device("cuda:0"))


def _poison(engines):
    n = 0
    for eng in engines:
        ws = eng._ws.get("fwd")
        if ws is not None:
            ws.fill_(0xFF)
            n += 1
    return n


def kernel_outputs(case, m, nsp, d):
    """The case's outputs through the public forward of the models.  bf16: every measured run is preceded by a run that makes the engine's
    workspace exist at this size, and by filling that workspace with 0xFF."""
    a = (d["input_ids"], d["segment_ids"], d["attention_mask"])
    kw = dict(img_feats=d["img_feats"])
    runs = {"mask": (m, lambda: m(*a, mask_token_pos=d["mask_token_pos"], **kw)),
            "all": (m, lambda: m(*a, **kw)),
            "bert": (m.bert, lambda: m.bert(*a, **kw)),
            "nsp": (nsp, lambda: nsp(*a, **kw))}
    engines = [m._engine(), m.bert._engine(), nsp._engine()]
    out = {}
    for model in (m, m.bert, nsp):
        model.set_compute_dtype(case.mode)
    for eng in engines:
        eng.fold_ln = case.fold
    try:
        with torch.no_grad():
            for o in case.outputs:
                model, run = runs[o]
                if case.mode == "bf16":
                    run()
                    assert _poison([model._engine()]) == 1
                res = run()
                if o == "mask":
                    out["mask_logits"] = res[0]
                elif o == "all":
                    out["all_logits"] = res[0]
                elif o == "bert":
                    out["seq"], out["pooled"] = res[0], res[1]
                else:
                    out["rel"] = res[0]
        torch.cuda.synchronize()
    finally:
        for eng in engines:
            eng.fold_ln = True
    return out


def run_case(env, case):
    dev, get = env
    m, nsp, sd64, nsp64 = get(case.cfg)
    cfg = m.config
    b = make_inputs(case, cfg)
    d = {k: (v.to(dev) if v is not None else None) for k, v in b.items()}
    t0 = time.time()
    got = kernel_outputs(case, m, nsp, d)
    t1 = time.time()
    d64 = dict(d, img_feats=d["img_feats"].double() if d["img_feats"] is not None else None)
    cd = cfg.to_dict()
    ref = oracle_outputs(sd64, nsp64, cd, d64, case.outputs, False)
    emu = oracle_outputs(sd64, nsp64, cd, d64, case.outputs, True) if case.mode == "bf16" else None
    torch.cuda.synchronize()
    t2 = time.time()
    rows = FC.compare(case.mode, got, ref, emu)
    print("\n%s (%s, B=%d, L=%d+%d): forward %.2f s, oracle %.2f s" % (case.id, case.mode, case.B, case.Lt, case.Li, t1 - t0, t2 - t1))
    print(FC.table(rows, case.id))
    FC.check(case.mode, got, ref, emu, case.id)
    return rows


@pytest.mark.parametrize("case", [c for c in CASES if c.mode == "bf16"], ids=[c.id for c in CASES if c.mode == "bf16"])
def test_bf16_forward_matches_emulation(env, case):
    run_case(env, case)


@pytest.mark.parametrize("case", [c for c in CASES if c.mode != "bf16"], ids=[c.id for c in CASES if c.mode != "bf16"])
def test_parity_modes_match_float64(env, case):
    run_case(env, case)
