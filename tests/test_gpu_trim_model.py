"""GPU: the inference forward with trim=True (PackedModel.forward / the models' ``trim_padding``) against the float64 oracle of the UNTRIMMED
padded batch, through tests/_fwdcheck.py with the bounds of the forward-regime tests (FIXED, FIXED_ROW, C_FWD, FLOOR_FWD, ABS_BAND).

Shapes are chosen where the plan changes under trimming (cpt_amd/csrc/cpt_abi.hip make_plan), on Oscar-base width with 2 layers and on the tiny
golden config:
  short     padded 165 + 45, real text <= 23, regions <= 30: the two-kernel attention of L = 210 becomes the fused form of L <= 128
  long      padded 165 + 45, real text 100: stays above 128
  noregion  padded 70 + 50, no region attended: a text-only batch (Li' = 0, img_feats dropped)
  full      attended to the last text slot and the last region: nothing is cut, the output is bit-identical to trim=False
Outputs: [MASK]-row logits, column-list scores, pooled output, relation scores -- the head-row outputs trimming is defined for.
The reference is computed once per case and shared by the three compute modes."""
import collections

import numpy as np
import pytest
import torch

import _fwdcheck as FC
import test_gpu_fwd_regimes as R
from cpt_amd import _lib as L
from cpt_amd import batching as BT
from cpt_amd import config as cfgmod
from cpt_amd import synth

pytestmark = pytest.mark.gpu
SEED = 4321

Case = collections.namedtuple("Case", "id cfg B Lt Li text regions grow")
CASES = [
    Case("base_short", "base2", 5, 165, 45, 23, 30, 0),
    Case("base_long", "base2", 5, 165, 45, 70, 45, 100),
    Case("base_noregion", "base2", 4, 70, 50, 40, 0, 0),
    Case("base_full", "base2", 3, 70, 50, 70, 50, 70),
    Case("tiny_short", "tiny", 5, 28, 12, 20, 6, 0),
    Case("tiny_noregion", "tiny", 4, 28, 12, 20, 0, 0),
    Case("tiny_full", "tiny", 3, 28, 12, 28, 12, 28),
]
MODES = ("fp32", "bf16x3", "bf16")


def make_inputs(case, cfg):
    """A ragged batch of real size text x regions (synth.make_batch) inside the padded shape Lt + Li; ``grow``: sequence 0's text is
    extended to that many attended tokens."""
    b = synth.make_batch(case.B, cfg, seed=700 + case.B + case.Lt, max_seq_len=case.text, img_seq_len=max(case.regions, 1),
                         vary_regions=case.regions < case.Li)
    B, D = case.B, cfg.img_feature_dim
    ids = torch.zeros((B, case.Lt), dtype=torch.int64)
    seg = torch.zeros((B, case.Lt), dtype=torch.int64)
    mask = torch.zeros((B, case.Lt + case.Li), dtype=torch.int64)
    img = torch.zeros((B, case.Li, D), dtype=torch.float32)
    ids[:, :case.text], seg[:, :case.text], mask[:, :case.text] = b["input_ids"], b["segment_ids"], b["attention_mask"][:, :case.text]
    if case.regions:
        img[:, :case.regions] = b["img_feats"]
        mask[:, case.Lt:case.Lt + case.regions] = b["attention_mask"][:, case.text:]
    if case.grow:
        rng = np.random.Generator(np.random.PCG64(case.grow))
        n = int(mask[0, :case.Lt].sum())
        ids[0, n:case.grow] = torch.from_numpy(rng.integers(10, min(cfg.vocab_size, 30000), case.grow - n))
        seg[0, n:case.grow] = 1
        mask[0, :case.grow] = 1
    return dict(input_ids=ids, segment_ids=seg, attention_mask=mask, img_feats=img, mask_token_pos=b["mask_token_pos"])


def colour_columns(cfg):
    cols = [c for c in synth.COLOR_IDS + (synth.NONE_ID,) if c < cfg.vocab_size] or [5, 6, 7, 8, 9, 10]
    return torch.tensor(cols, dtype=torch.int64)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    built, refs = {}, {}

    def models(name):
        if name not in built:
            from cpt_amd.modeling_bert import BertImgForPreTraining
            from cpt_amd.modeling_rec import REC_MLM_CPT
            from cpt_amd.modeling_vcr import NSPCPT
            cfg = cfgmod.oscar_base(num_hidden_layers=2) if name == "base2" else cfgmod.tiny()
            sd = synth.init_state_dict(cfg, SEED, head="cpt")
            sdp = synth.init_state_dict(cfg, SEED, head="pretrain")
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

    def reference(case, emulate):
        """The float64 oracle (or its bf16 emulation) of the PADDED batch, once per case."""
        key = (case.id, emulate)
        if key not in refs:
            m, _, sd64, nsp64 = models(case.cfg)
            b = make_inputs(case, m.config)
            d64 = {k: v.to(dev) for k, v in b.items()}
            d64["img_feats"] = d64["img_feats"].double()
            o = R.oracle_outputs(sd64, nsp64, m.config.to_dict(), d64, ("mask", "bert", "nsp"), emulate)
            cols = colour_columns(m.config).to(dev)
            refs[key] = {"mask_logits": o["mask_logits"], "cols_logits": o["mask_logits"][:, cols], "pooled": o["pooled"], "rel": o["rel"]}
        return refs[key]
    return dev, models, reference


def run_outputs(m, nsp, d, cols, trim, shapes=None):
    """The four head-row outputs; ``shapes`` collects engine.last_shape after each forward."""
    a = (d["input_ids"], d["segment_ids"], d["attention_mask"])
    out = {}
    note = (lambda eng: shapes.append(eng.last_shape)) if shapes is not None else (lambda eng: None)
    m.trim_padding = nsp.trim_padding = trim
    try:
        with torch.no_grad():
            out["mask_logits"] = m(*a, img_feats=d["img_feats"], mask_token_pos=d["mask_token_pos"])[0]
            note(m._engine())
            out["cols_logits"] = m(*a, img_feats=d["img_feats"], mask_token_pos=d["mask_token_pos"], vocab_columns=cols)[0]
            note(m._engine())
            out["pooled"] = m.bert._engine().forward(*a, None, d["img_feats"], flags=L.OUT_POOLED, trim=trim)["pooled"]
            note(m.bert._engine())
            out["rel"] = nsp(*a, img_feats=d["img_feats"])[0]
            note(nsp._engine())
        torch.cuda.synchronize()
    finally:
        m.trim_padding = nsp.trim_padding = False
    return out


def expected_shape(case, b):
    want = BT.batch_extent(b["attention_mask"], case.Lt, b["mask_token_pos"])
    assert want == BT.batch_extent(b["attention_mask"], case.Lt)          # the [MASK] slot lies inside the attended text
    kind = case.id.split("_")[1]
    if kind == "short":
        assert want[0] <= case.text and 0 < want[1] <= case.regions and sum(want) <= 128
        assert case.cfg == "tiny" or case.Lt + case.Li > 128            # Oscar-base: from the two-kernel attention to the fused form
    elif kind == "long":
        assert want[0] == 100 and sum(want) > 128 and want != (case.Lt, case.Li)
    elif kind == "noregion":
        assert want[1] == 0 and want[0] < case.Lt
    else:
        assert want == (case.Lt, case.Li)
    return (case.B,) + want


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_trimmed_forward_matches_padded_oracle(env, case, mode):
    dev, models, reference = env
    m, nsp, _, _ = models(case.cfg)
    b = make_inputs(case, m.config)
    d = {k: v.to(dev) for k, v in b.items()}
    cols = colour_columns(m.config).to(dev)
    want_shape = expected_shape(case, b)
    for model in (m, m.bert, nsp):
        model.set_compute_dtype(mode)
    if mode == "bf16":                                  # every read of something a launch should have written first shows up
        run_outputs(m, nsp, d, cols, True)
        assert R._poison([m._engine(), m.bert._engine(), nsp._engine()]) == 3
    shapes = []
    got = run_outputs(m, nsp, d, cols, True, shapes)
    assert shapes == [want_shape] * 4, (shapes, want_shape)
    ref = reference(case, False)
    emu = reference(case, True) if mode == "bf16" else None
    rows = FC.compare(mode, got, ref, emu)
    print("\n%s %s: ran %s of padded %s" % (case.id, mode, want_shape, (case.B, case.Lt, case.Li)))
    print(FC.table(rows, case.id))
    FC.check(mode, got, ref, emu, case.id)
    plain_shapes = []
    plain = run_outputs(m, nsp, d, cols, False, plain_shapes)
    assert plain_shapes == [(case.B, case.Lt, case.Li)] * 4             # trim off: the padded shape, as before
    if want_shape == (case.B, case.Lt, case.Li):
        for k in got:
            assert torch.equal(got[k], plain[k]), k                      # nothing to cut: the same launches on the same buffers
    if mode == "fp32":
        assert got["cols_logits"].argmax(1).tolist() == plain["cols_logits"].argmax(1).tolist()
        assert got["mask_logits"][:, cols].argmax(1).tolist() == plain["mask_logits"][:, cols].argmax(1).tolist()


@pytest.mark.parametrize("cfg_name", ["base2", "tiny"])
def test_trim_is_skipped_where_a_dropped_row_would_show(env, cfg_name):
    dev, models, _ = env
    case = next(c for c in CASES if c.cfg == cfg_name and c.id.endswith("short"))
    m, nsp, _, _ = models(cfg_name)
    b = make_inputs(case, m.config)
    d = {k: v.to(dev) for k, v in b.items()}
    padded = (case.B, case.Lt, case.Li)
    Lw = case.Lt + case.Li
    for model in (m, m.bert):
        model.set_compute_dtype("fp32")
    m.trim_padding = m.bert.trim_padding = True
    try:
        with torch.no_grad():
            seq, pooled = m.bert(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"])       # OUT_SEQ
            assert m.bert._engine().last_shape == padded and tuple(seq.shape) == (case.B, Lw, m.config.hidden_size)
            mask3 = d["attention_mask"][:, None, :].repeat(1, Lw, 1).contiguous()
            m(d["input_ids"], d["segment_ids"], mask3, img_feats=d["img_feats"], mask_token_pos=d["mask_token_pos"])     # 3-D mask
            assert m._engine().last_shape == padded
            m(d["input_ids"], d["segment_ids"], None, img_feats=d["img_feats"], mask_token_pos=d["mask_token_pos"])      # no mask
            assert m._engine().last_shape == padded
            if cfg_name == "tiny":
                full = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"])[0]            # OUT_ALL_LOGITS
                assert m._engine().last_shape == padded and tuple(full.shape) == (case.B, Lw, m.config.vocab_size)
                grid = torch.full((case.B, Lw), -1, dtype=torch.int64, device=dev)
                grid[torch.arange(case.B, device=dev), d["mask_token_pos"]] = 7
                m(d["input_ids"], d["segment_ids"], d["attention_mask"], masked_lm_labels=grid, img_feats=d["img_feats"],
                  mask_token_pos=d["mask_token_pos"])                                                                     # a loss
                assert m._engine().last_shape == padded
            # and the row forms: (sequence, position) head rows and log_softmax are trimmed, to the same extent
            pairs = torch.stack([torch.arange(case.B, device=dev), d["mask_token_pos"]], 1)
            rows = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], mask_token_pos=pairs, log_softmax=True)[0]
            assert m._engine().last_shape == (case.B,) + BT.batch_extent(b["attention_mask"], case.Lt, b["mask_token_pos"])
            m.trim_padding = False
            want = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], mask_token_pos=pairs, log_softmax=True)[0]
            assert m._engine().last_shape == padded
            assert (rows - want).abs().max().item() <= FC.ABS_BAND["fp32"]
    finally:
        m.trim_padding = m.bert.trim_padding = False


def test_head_row_beyond_the_attended_text_is_kept(env):
    """A [MASK] slot past the last attended text index widens Lt' (the row must exist to be read)."""
    dev, models, _ = env
    case = next(c for c in CASES if c.id == "tiny_short")
    m, _, _, _ = models("tiny")
    m.set_compute_dtype("fp32")
    b = make_inputs(case, m.config)
    far = int(BT.batch_extent(b["attention_mask"], case.Lt)[0]) + 3
    assert far < case.Lt
    b["mask_token_pos"][1] = far
    d = {k: v.to(dev) for k, v in b.items()}
    a = (d["input_ids"], d["segment_ids"], d["attention_mask"])
    with torch.no_grad():
        want = m(*a, img_feats=d["img_feats"], mask_token_pos=d["mask_token_pos"])[0]
        m.trim_padding = True
        try:
            got = m(*a, img_feats=d["img_feats"], mask_token_pos=d["mask_token_pos"])[0]
        finally:
            m.trim_padding = False
    assert m._engine().last_shape[1] == far + 1
    assert (got - want).abs().max().item() <= FC.ABS_BAND["fp32"]
