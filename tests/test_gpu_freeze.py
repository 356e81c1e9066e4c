"""GPU: layer freezing -- the training step with a frozen prefix of stages (cpt_train_bwd_from / cpt_train_zero_grads_from through
train.freeze_layers / freeze_embeddings / train_head_only), the optimizer over the trainable range and the data-parallel bucket subset.

The reference is the FULL step of the same build (existing code, held to the float64 oracle by tests/test_gpu_train_regimes.py) on the same
batch with the same dropout seed and step.  Rules (``_check_against_full``):
  * loss and head scores: the same bits (the training forward adds the row losses up in row order in the cross-entropy launch's last
    workgroup, csrc/rowops.hip ce_finish_rows, so the loss is a function of the inputs alone);
  * a frozen parameter has ``.grad is None``;
  * every trainable Linear weight gradient (two-dimensional, not an embedding table) ABOVE the boundary layer, the head's among them (head
    transform, pooler, the relation heads' weights): ``torch.equal``.  At the boundary layer bit equality holds for
    every Linear weight too and is asserted: attention output, FFN up and FFN down come from the full walk's own launches, and the Q|K|V
    weight gradient's K-split partial matrices are added in split order by either carrier (the flush launch here, the next layer's spare
    workgroups in the full walk);
  * the vectors the backward sums with atomics (bias / LayerNorm gain and shift, the head's among them) and the boundary layer's column
    sums, whose summing launch changed: the bound tests/test_gpu_train_trim.py::_same_bits applies between two runs of one step,
    ``_gradcheck.rel <= _gradcheck.FIXED["fp32"]``, attention.self.key.bias (rounding noise on both sides) excepted as there.

Shapes: ``oscar_base(num_hidden_layers=4)`` at L = 70 + 50 (hidden 768 keeps the real tile choices), bf16, B = 4 (480 rows: fp32 K-split
partials, narrow tiles), 18 (2160 rows: bf16 partial pair, lean LayerNorm) and 32 (3840 rows: triple launch with deferred Q|K|V partial sums);
stages 1 (embedding side only), 2 (a mid boundary), 4 (the pruned tail layer alone) and 5 (the head only).
"""
import os
import tempfile
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _gradcheck as G
import _softcheck as S
from cpt_amd import config as cfgmod
from cpt_amd import engine, soft_prompt, synth, train
from oracle import cpt_oracle as O
from test_gpu_dropout import SEED, _drop_dict
from test_gpu_train_trim import _free_port, _param_diff_ok

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NL = 4
LT, LI = 70, 50
STAGES = (1, 2, 4, 5)
SAME_RUN_BOUND = G.FIXED["fp32"]        # tests/test_gpu_train_trim.py::_same_bits, its last branch


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---- shared ----------------------------------------------------------------------------------------------------------------------------------
def _grads(m, loss, scores):
    got = {n: (p.grad.clone() if p.grad is not None else None) for n, p in m.named_parameters()}
    got["loss"], got["scores"] = loss.detach().reshape(1).clone(), scores.detach().clone()
    return got


def _mlm_step(m, d, p=0.0, lab=None):
    cfg = m.config
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = p
    train.set_dropout_seed(m, SEED, step=0)
    for prm in m.parameters():
        prm.grad = None
    if lab is not None:
        loss, scores = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d.get("img_feats"), masked_lm_labels=lab)
    else:
        loss, scores = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d.get("img_feats"), masked_lm_labels=d["colors"],
                         mask_token_pos=d["mask_token_pos"])
    loss.backward()
    return _grads(m, loss, scores)


def _is_linear_weight(n, t):
    """A Linear weight gradient -- two-dimensional, not an embedding table (no LayerNorm is): GEMMs (or the relation heads' fixed-order sums)
    write it whole with no atomics upstream, the rule of tests/test_gpu_train.py::test_backward_needs_no_whole_buffer_fill.  The encoder's
    matrices, and the head's: head transform, pooler, relation heads."""
    return t.dim() == 2 and "embeddings" not in n


def _check_against_full(full, got, stage, n_layers, what):
    """The rules of the module docstring; prints the worst bounded tensor and which boundary tensors came out with the same bits."""
    print("%s: loss %r, full step %r" % (what, float(got["loss"]), float(full["loss"])))
    assert torch.equal(full["loss"], got["loss"]), (what, float(full["loss"]), float(got["loss"]))
    assert torch.equal(full["scores"], got["scores"]), what
    worst, same_at_boundary = (0.0, ""), []
    for n, ref in full.items():
        if n in ("loss", "scores") or n == soft_prompt.KEY:
            continue
        k = engine.bucket_of(n, n_layers)
        if k < stage or ref is None:
            assert got[n] is None, "%s: %s (stage %d) has a gradient under first stage %d" % (what, n, k, stage)
            continue
        assert got[n] is not None, "%s: trainable %s has no gradient" % (what, n)
        if G.is_key_bias(n):
            continue
        boundary = k == stage and k <= n_layers
        if _is_linear_weight(n, ref):
            assert torch.equal(ref, got[n]), "%s: %s differs from the full step's bits (rel %.3g)" % (what, n, G.rel(got[n], ref))
            continue
        r = G.rel(got[n], ref)
        print("%s: %-60s rel %.3e%s" % (what, n, r, "  (boundary)" if boundary else ""))
        assert r <= SAME_RUN_BOUND, (what, n, r)
        worst = max(worst, (r, n))
        if boundary and torch.equal(ref, got[n]):
            same_at_boundary.append(n)
    print("%s: worst bounded tensor %s rel %.3e; boundary tensors with the full step's bits: %s" % (what, worst[1], worst[0], same_at_boundary))
    return same_at_boundary


# ---- 4-layer Oscar-base --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base(dev):
    cfg0 = cfgmod.oscar_base(num_hidden_layers=NL)
    sd = synth.init_state_dict(cfg0, 1234, head="cpt")
    models, fulls, batches = {}, {}, {}

    def model(mode):
        from cpt_amd.modeling_rec import REC_MLM_CPT
        if mode not in models:
            m = REC_MLM_CPT(cfgmod.oscar_base(num_hidden_layers=NL))
            m.load_state_dict(sd)
            m.tie_weights()
            m.to(dev).train()
            m.set_compute_dtype(mode)
            models[mode] = m
        return models[mode]

    def batch(B, kind="plain"):
        """(device batch, label grid or None); kind: plain | text (Li = 0) | grid (several labelled rows per sequence: row_seq)."""
        if (B, kind) not in batches:
            b = synth.make_batch(B, cfg0, seed=3000 + B, vary_regions=True)
            lab = None
            if kind == "text":
                b = dict(b, attention_mask=b["attention_mask"][:, :b["input_ids"].size(1)].contiguous())
                del b["img_feats"]
            if kind == "grid":
                lab = torch.full(b["attention_mask"].shape, -1, dtype=torch.long)
                for i in range(B):
                    mp_ = int(b["mask_token_pos"][i])
                    lab[i, mp_] = int(b["colors"][i])
                    if i % 2 == 0:
                        lab[i, 1] = int(synth.COLOR_IDS[i % 5])
                        lab[i, mp_ + 1] = int(synth.COLOR_IDS[(i + 2) % 5])
                lab = lab.to(dev)
            batches[(B, kind)] = ({k: v.to(dev) for k, v in b.items()}, lab)
        return batches[(B, kind)]

    def full(mode, B, p, kind="plain"):
        """The full step (no stage set) on this batch, computed once and left unchanged."""
        key = (mode, B, p, kind)
        if key not in fulls:
            m = model(mode)
            train.unfreeze(m)
            d, lab = batch(B, kind)
            fulls[key] = _mlm_step(m, d, p, lab)
        return fulls[key]
    return cfg0, sd, model, batch, full


def _staged(base, mode, B, p, stage, kind="plain"):
    cfg0, sd, model, batch, full = base
    ref = full(mode, B, p, kind)
    m = model(mode)
    d, lab = batch(B, kind)
    train._set_stage(m, stage)
    try:
        got = _mlm_step(m, d, p, lab)
    finally:
        train.unfreeze(m)
    what = "%s B=%d p=%g %s stage %d" % (mode, B, p, kind, stage)
    return _check_against_full(ref, got, stage, NL, what), got


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("B", [4, 18, 32])
def test_bf16_stages_match_the_full_step(dev, base, B, stage):
    _staged(base, "bf16", B, 0.1, stage)


@pytest.mark.parametrize("B", [4, 32])
def test_bf16_without_dropout(dev, base, B):
    for stage in STAGES:
        _staged(base, "bf16", B, 0.0, stage)


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_unfused_branch_at_few_rows(dev, base, mode):
    for stage in STAGES:
        _staged(base, mode, 4, 0.1, stage)


def test_text_only_batch(dev, base):
    for stage in STAGES:
        _staged(base, "bf16", 4, 0.1, stage, kind="text")


def test_label_grid_batch(dev, base):
    for stage in STAGES:          # (a label grid: the last layer runs on all rows -- no pruned tail at stage 4)
        _staged(base, "bf16", 4, 0.1, stage, kind="grid")


def test_two_full_steps_give_the_same_loss_bits(dev, base):
    """What the loss rule rests on: the full step itself reproduces its loss bit for bit (mask rows, a label grid, 32 sequences)."""
    cfg0, sd, model, batch, full = base
    m = model("bf16")
    train.unfreeze(m)
    for B, kind in ((4, "plain"), (4, "grid"), (32, "plain")):
        d, lab = batch(B, kind)
        ref = full("bf16", B, 0.1, kind)
        for _ in range(3):
            again = _mlm_step(m, d, 0.1, lab)
            assert torch.equal(ref["loss"], again["loss"]) and torch.equal(ref["scores"], again["scores"]), (B, kind)


def test_stage_zero_is_the_full_step(dev, base):
    """unfreeze() after a stage: the plain entry points again, the same bits wherever the step reproduces its own."""
    cfg0, sd, model, batch, full = base
    m = model("bf16")
    ref = full("bf16", 4, 0.1)
    train.freeze_layers(m, 2)
    train.unfreeze(m)
    d, lab = batch(4)
    _check_against_full(ref, _mlm_step(m, d, 0.1), 0, NL, "bf16 B=4 unfrozen")


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_trainable_gradients_match_float64(dev, base, mode):
    """B = 4, stage 2: the trainable gradients through tests/_gradcheck.py against oracle.cpt_oracle.train_step_grads, as
    tests/test_gpu_train_regimes.py checks the full step (dropout 0.1, the masks the library exports)."""
    cfg0, sd, model, batch, full = base
    B, p, stage = 4, 0.1, 2
    _, got = _staged(base, mode, B, p, stage)
    m = model(mode)
    d, _ = batch(B)
    sd64 = {k: v.to(dev, torch.float64) for k, v in sd.items()}
    sd64["cls.decoder.weight"] = sd64["bert.embeddings.word_embeddings.weight"]
    drop = {k: v.to(dev) for k, v in _drop_dict(dev, m.config, p, 1, B, LT + LI).items()}
    d64 = dict(d, img_feats=d["img_feats"].double())

    def oracle(bf16):
        loss_r, grads, sc = O.train_step_grads(sd64, m.config.to_dict(), d64, drop=drop, bf16=bf16, with_scores=True)
        out = {n: g for n, g in grads.items() if n in got and got[n] is not None}          # the trainable stages' tensors
        out["loss"], out["scores"] = loss_r.reshape(1), sc
        return out
    ref = oracle(False)
    assert any(n.startswith("bert.encoder.layer.1.") for n in ref) and not any(n.startswith(("bert.encoder.layer.0.", "bert.embeddings.")) for n in ref)
    emu = oracle(True) if mode == "bf16" else None
    what = "%s B=%d stage %d against float64" % (mode, B, stage)
    print("\n%s\n%s" % (what, G.table(G.compare(mode, got, ref, emu))))
    G.check(mode, got, ref, emu, what)


# ---- the relation heads on the tiny shape -------------------------------------------------------------------------------------------------------
def _tiny_cfg():
    cfg = cfgmod.tiny(num_hidden_layers=NL)
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
    return cfg


def _pretrained(cfg, seed=4321):
    from cpt_amd.modeling_bert import BertImgForPreTraining
    pre = BertImgForPreTraining(cfg)
    pre.load_state_dict(synth.init_state_dict(cfg, seed, head="pretrain"))
    pre.tie_weights()
    return pre


def _head_step(m, run, p):
    cfg = m.config
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = p
    train.set_dropout_seed(m, SEED, step=0)
    for prm in m.parameters():
        prm.grad = None
    loss, scores = run()
    loss.backward()
    return _grads(m, loss, scores)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("head", ["nsp", "qar"])
def test_relation_heads(dev, mode, head):
    from cpt_amd.modeling_vcr import NSPCPT, VCRQAR_NSPCPT
    cfg = _tiny_cfg()
    m = (NSPCPT if head == "nsp" else VCRQAR_NSPCPT)(cfg)
    m.copy_from_pretraining_model(_pretrained(cfg))
    if head == "qar":
        g = torch.Generator().manual_seed(4322)
        with torch.no_grad():
            m.cls_rat.weight.add_(torch.randn(m.cls_rat.weight.shape, generator=g) * 0.05)
    m.to(dev).train().set_compute_dtype(mode)
    b = {k: v.to(dev) for k, v in synth.make_batch(8, cfg, seed=11, max_seq_len=20, img_seq_len=6, vary_regions=True).items()}
    labels = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1], device=dev)
    if head == "nsp":
        run = lambda: m(b["input_ids"], b["segment_ids"], b["attention_mask"], next_sentence_label=labels, img_feats=b["img_feats"])
    else:
        part = lambda lo, hi: {"input_ids": b["input_ids"][lo:hi], "token_type_ids": b["segment_ids"][lo:hi],
                               "attention_mask": b["attention_mask"][lo:hi], "img_feats": b["img_feats"][lo:hi]}

        def run():
            loss, ra, rr = m.qar_forward(part(0, 5), part(5, 8), labels[:5], labels[5:])
            return loss, torch.cat([ra, rr], 0)
    for p in (0.0, 0.1):
        full = _head_step(m, run, p)
        assert full["bert.embeddings.word_embeddings.weight"] is not None and full["bert.pooler.dense.weight"] is not None
        for stage in (1, 3, 5):
            train._set_stage(m, stage)
            try:
                got = _head_step(m, run, p)
            finally:
                train.unfreeze(m)
            _check_against_full(full, got, stage, NL, "%s %s p=%g stage %d" % (head, mode, p, stage))


# ---- a trainable template under trainable top layers ------------------------------------------------------------------------------------------
def _template_case(dev, cfg, sd, mode, b, p, scale):
    """stage 3 (layers 2, 3 and the head train; the template trains under the frozen layers 0, 1).  The full step refuses an attached
    template, so the layer gradients are held to the float64 oracle construction of tests/_softcheck.py through tests/_gradcheck.py -- the
    rule the full step itself is held to -- and the template's gradient is compared the way tests/test_gpu_soft_prompt.py does."""
    from cpt_amd.modeling_rec import REC_MLM_CPT
    stage = 3
    m = REC_MLM_CPT(cfg)
    m.load_state_dict(sd)
    m.tie_weights()
    m.to(dev).train()
    m.set_compute_dtype(mode)
    w = soft_prompt.attach(m, n_slots=S.N_SLOTS, freeze_backbone=False)
    tmpl = S.make_template(sd[S.WORD], scale=scale)
    with torch.no_grad():
        w.copy_(tmpl.to(dev))
    d = {k: v.to(dev) for k, v in b.items()}
    B, L = d["attention_mask"].shape
    # stage 0 with a trainable template still raises
    with pytest.raises(NotImplementedError, match="trainable soft template"):
        m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], masked_lm_labels=d["colors"], mask_token_pos=d["mask_token_pos"])
    train.freeze_layers(m, stage - 1)
    got = _mlm_step(m, d, p)
    first = got[soft_prompt.KEY].clone()
    again = _mlm_step(m, d, p)
    assert torch.equal(first, again[soft_prompt.KEY]) and torch.equal(got["scores"], again["scores"]), "two backward runs: the same template bits"
    for n in got:
        if n not in ("loss", "scores", soft_prompt.KEY):
            assert (got[n] is None) == (engine.bucket_of(n, cfg.num_hidden_layers) < stage or n.startswith(train.NO_GRAD_PREFIXES)), n
    sd64 = {k: v.to(dev, torch.float64) for k, v in sd.items()}
    sd64["cls.decoder.weight"] = sd64[S.WORD]
    t64 = tmpl.to(dev, torch.float64)
    drop = {k: v.to(dev) for k, v in _drop_dict(dev, cfg, p, 1, B, L).items()} if p > 0 else None
    d64 = dict(d, img_feats=d["img_feats"].double())

    def oracle(bf16):
        loss_r, grads, sc = O.train_step_grads(S.oracle_state(sd64, t64), cfg.to_dict(), d64, drop=drop, bf16=bf16, with_scores=True)
        out = {n: g for n, g in grads.items() if n in got and got[n] is not None and n != soft_prompt.KEY}
        tg = grads[S.WORD][:S.N_SLOTS].detach().clone()
        tg[0] = 0
        out.update({"template": tg, "loss": loss_r.reshape(1), "scores": sc})
        return out
    ref = oracle(False)
    emu = oracle(True) if mode == "bf16" else None
    mine = dict(got, template=first)
    what = "template + top layers, %s B=%d p=%g" % (mode, B, p)
    print("\n%s\n%s" % (what, G.table(G.compare(mode, mine, ref, emu))))
    G.check(mode, mine, ref, emu, what)
    unused = [s for s in range(S.N_SLOTS) if s not in S.USED]
    assert not bool(first[unused].any()) and all(bool(first[s].any()) for s in S.USED)


def test_template_with_top_layers_tiny(dev):
    cfg = _tiny_cfg()
    sd = synth.init_state_dict(cfg, 1234, head="cpt")
    b = S.plant_slots(synth.make_batch(4, cfg, seed=S.TINY_BATCH_SEED, max_seq_len=20, img_seq_len=6))
    _template_case(dev, cfg, sd, "fp32", b, 0.0, 0.05)


def test_template_with_top_layers_base(dev, base):
    cfg0, sd, model, batch, full = base
    cfg = cfgmod.oscar_base(num_hidden_layers=NL)
    b = S.plant_slots(synth.make_batch(4, cfg, seed=2004, vary_regions=True))
    _template_case(dev, cfg, sd, "bf16", b, 0.1, 0.02)


# ---- optimizer ----------------------------------------------------------------------------------------------------------------------------------
def _tiny_mlm(dev, mode="fp32", seed=1234):
    from cpt_amd.modeling_rec import REC_MLM_CPT
    cfg = _tiny_cfg()
    m = REC_MLM_CPT(cfg)
    m.load_state_dict(synth.init_state_dict(cfg, seed, head="cpt"))
    m.tie_weights()
    m.to(dev).train()
    m.set_compute_dtype(mode)
    return m, cfg


def _opt_settings():
    t = np.load(os.path.join(GOLDEN, "tiny_train3.npz"))          # the settings of tests/test_gpu_train.py::test_tiny_train3_trace_fp32
    return dict(lr=float(t["lr0"]), betas=(float(t["beta1"]), float(t["beta2"])), weight_decay=float(t["wd"]))


def _forward_backward(m, d):
    loss, _ = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], masked_lm_labels=d["colors"],
                mask_token_pos=d["mask_token_pos"])
    loss.backward()
    return loss


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_three_optimizer_steps_equal_full_steps_with_frozen_updates_discarded(dev, mode):
    stage, steps = 3, 3
    m, cfg = _tiny_mlm(dev, mode)
    d = {k: v.to(dev) for k, v in synth.make_batch(4, cfg, seed=612, max_seq_len=20, img_seq_len=6, vary_regions=True).items()}
    start = {n: p.detach().clone() for n, p in m.named_parameters()}
    frozen = [n for n in start if engine.bucket_of(n, NL) < stage]
    assert frozen and len(frozen) < len(start)
    # the reference: full steps; after each, the frozen parameters' updates are thrown away
    ref_m, _ = _tiny_mlm(dev, mode)
    ref_opt = train.FusedAdamW(ref_m, **_opt_settings())
    named = dict(ref_m.named_parameters())
    for _ in range(steps):
        ref_opt.zero_grad()
        _forward_backward(ref_m, d)
        ref_opt.step()
        with torch.no_grad():
            for n in frozen:
                named[n].copy_(start[n])
    ref = {n: p.detach().clone() for n, p in ref_m.named_parameters()}
    # the stage
    train.freeze_layers(m, stage - 1)
    opt = train.FusedAdamW(m, **_opt_settings())
    lo, hi = opt.trainable_elements()
    eng = m._engine()
    assert (lo, hi) == (eng.buckets[stage][0], eng.flat.numel())
    shadow0 = eng.flat_lp[:lo].clone() if mode == "bf16" and eng.flat_lp is not None else None
    for i in range(steps):
        opt.zero_grad()
        _forward_backward(m, d)
        if i == 0:
            # the device clip norm is torch's over the trainable parameters (frozen ranges of the flat gradient hold zeros).  Equal up to the
            # order of the sum: cpt_grad_clip adds the squares of the flat buffer in one fixed order in fp32, torch adds per-tensor norms; the
            # reference here is the float64 sum, the bound the 1e-5 tests/test_gpu_gqa_vcr.py holds the same launch to against torch
            norm = opt.clip_grad_norm_device(1e9)
            assert float(opt.last_clip[1]) == 1.0
            live = [p for p in m.parameters() if p.requires_grad and p.grad is not None]
            tnorm = torch.nn.utils.clip_grad_norm_(live, 1e9)
            norm64 = float(sum((p.grad.double() ** 2).sum() for p in live).sqrt())
            assert abs(float(norm) - norm64) <= 1e-5 * norm64, (float(norm), norm64)
            assert abs(float(norm) - float(tnorm)) <= 1e-5 * float(tnorm), (float(norm), float(tnorm))
            assert all(p.grad is None for n, p in m.named_parameters() if n in frozen)
        opt.step()
    now = {n: p.detach().clone() for n, p in m.named_parameters()}
    for n in frozen:
        assert torch.equal(now[n], start[n]), "frozen %s moved" % n
    moved = 0
    for n in now:
        if n in frozen or n.startswith(train.NO_GRAD_PREFIXES):
            continue
        moved += int(not torch.equal(now[n], start[n]))
        if G.is_key_bias(n):          # (rounding noise on both sides, which AdamW normalises to full-size steps of either sign: _gradcheck, _param_diff_ok)
            continue
        mx = float((now[n].double() - ref[n].double()).abs().max())
        rel = G.rel(now[n], ref[n])
        # the 3-step tolerance of tests/test_gpu_train.py::test_tiny_train3_trace_fp32
        assert (mx < 5e-5) if mode == "fp32" else (rel < 2e-4), (n, mx, rel)
    assert moved > 10
    if shadow0 is not None:
        assert torch.equal(eng.flat_lp[:lo], shadow0), "the frozen stages' bf16 shadow was rewritten"
    # frozen entries of the optimizer state hold zero moments; the format is the full one
    sdo = opt.state_dict()
    assert set(sdo["state"]) == set(eng.offsets)
    for n in eng.offsets:
        z = not bool(sdo["state"][n]["exp_avg_sq"].any())
        assert z == (engine.bucket_of(n, NL) < stage or n.startswith(train.NO_GRAD_PREFIXES)), n
    # a stage change behind a stepped optimizer is refused
    train.freeze_layers(m, 1)
    opt.zero_grad()
    _forward_backward(m, d)
    with pytest.raises(RuntimeError, match="build a new optimizer"):
        opt.step()


def test_accumulation_adds_over_the_trainable_range_only(dev):
    """Two micro-steps on one batch without zero_grad: twice the single gradient on trainable parameters, nothing on frozen ones."""
    m, cfg = _tiny_mlm(dev)
    d = {k: v.to(dev) for k, v in synth.make_batch(4, cfg, seed=612, max_seq_len=20, img_seq_len=6).items()}
    train.freeze_layers(m, 2)
    one = _mlm_step(m, d)
    _forward_backward(m, d)
    for n, p in m.named_parameters():
        if one[n] is None:
            assert p.grad is None, n
        elif not G.is_key_bias(n):
            assert G.rel(p.grad, 2 * one[n]) <= SAME_RUN_BOUND, n
    st = train._state(m._engine())
    assert not bool(st.grad[:m._engine().buckets[3][0]].any()), "the frozen range of the flat gradient must hold zeros"


def test_training_loop_of_the_drivers_runs_with_a_stage(dev):
    from cpt_amd import drivers
    m, cfg = _tiny_mlm(dev)
    raw = synth.make_batch(4, cfg, seed=612, max_seq_len=20, img_seq_len=6, vary_regions=True)
    opts = types.SimpleNamespace(learning_rate=1e-3, warmup_steps=1, num_train_steps=10, lr_mul=1.0)
    train.freeze_layers(m, 3)
    start = {n: p.detach().clone() for n, p in m.named_parameters()}
    step, losses = drivers.train_batch(m, train.FusedAdamW(m, lr=1e-3), [raw, raw, raw], opts, dev)
    assert step == 3 and len(losses) == 3 and float(losses[2]) < float(losses[0])
    for n, p in m.named_parameters():
        frozen = engine.bucket_of(n, NL) < 4
        if frozen or n.startswith(train.NO_GRAD_PREFIXES):
            assert torch.equal(p.detach(), start[n]), n
    assert not torch.equal(m.cls.bias.detach(), start["cls.bias"])


# ---- data parallel: two ranks on one GPU over gloo (tests/test_gpu_train_trim.py::test_two_ranks_with_different_extents_equal_single_process) ----
DP_STEPS, DP_LR, DP_STAGE = 2, 1e-3, 3


def _dp_make(seed, dev):
    m, cfg = _tiny_mlm(dev, "fp32", seed)
    train.freeze_layers(m, DP_STAGE - 1)
    return m, cfg, train.FusedAdamW(m, lr=DP_LR, betas=(0.9, 0.98), weight_decay=0.01)


def _dp_steps(m, opt, d):
    for _ in range(DP_STEPS):
        opt.zero_grad()
        _forward_backward(m, d)
        opt.step()


def _dp_batch(cfg):
    return synth.make_batch(4, cfg, seed=77, max_seq_len=20, img_seq_len=6, n_regions=2)


def _dp_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        m, cfg, opt = _dp_make(1234 + 17 * rank, dev)          # rank 1 starts from other weights: the broadcast fixes that
        b = _dp_batch(cfg)
        _dp_steps(m, opt, {k: v[2 * rank:2 * rank + 2].to(dev) for k, v in b.items()})
        rep = opt.sync.comm_report(DP_STEPS)
        torch.save({"sd": {k: v.detach().cpu() for k, v in m.state_dict().items()}, "rs_bytes": rep["reduce_scatter_bytes_per_rank_per_step"],
                    "ag_bytes": rep["all_gather_bytes_per_rank_per_step"], "buckets": sorted(opt.sync.order), "shard": opt.m.numel()},
                   os.path.join(tmp, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_two_ranks_equal_single_process(dev):
    world = 2
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_dp_worker, args=(world, _free_port(), tmp), nprocs=world, join=True)
        r = [torch.load(os.path.join(tmp, "r%d.pt" % i)) for i in range(world)]
    m, cfg, opt = _dp_make(1234, dev)
    start = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    _dp_steps(m, opt, {k: v.to(dev) for k, v in _dp_batch(cfg).items()})
    one = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    for k in one:
        assert torch.equal(r[0]["sd"][k], r[1]["sd"][k]), k
    assert any(not torch.equal(one[k], start[k]) for k in one)
    _param_diff_ok({k: r[0]["sd"][k] for k in one}, one, DP_LR, DP_STEPS)
    for k in one:          # frozen on every rank: the bits of the start (rank 0's, broadcast)
        name = "bert.embeddings.word_embeddings.weight" if k == "cls.decoder.weight" else k
        if engine.bucket_of(name, NL) < DP_STAGE:
            assert torch.equal(r[0]["sd"][k], start[k]), k
    buckets = m._engine().buckets
    n_train = sum(hi - lo for kk, (lo, hi) in buckets.items() if kk >= DP_STAGE)
    for rank in range(world):
        assert r[rank]["buckets"] == [kk for kk in sorted(buckets) if kk >= DP_STAGE]
        assert r[rank]["rs_bytes"] == n_train * 4 and r[rank]["ag_bytes"] == n_train * 4
        assert r[rank]["shard"] == n_train // world
    assert n_train < m._engine().flat.numel() // 2
