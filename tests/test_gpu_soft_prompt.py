"""GPU: soft-template prompt tuning (cpt_amd/soft_prompt.py; cpt_model_fwd_soft, cpt_train_fwd_soft / cpt_train_bwd_soft) against the
float64 oracle construction of tests/_softcheck.py (pinned to the reference's TemplateEmbedding by tests/test_soft_prompt_cpu.py).

Forward: [MASK]-row scores within the bounds of tests/_fwdcheck.py per mode; a freshly attached template and a batch without slot ids
give the detached model's bits.  Gradient: the template's gradient, the loss and the scores within tests/_gradcheck.py's bounds as they
are (fp32 2e-4, bf16x3 5e-4, bf16 against the oracle's bf16 emulation with C = 2.5 and floor 2e-3) across the plan regimes of the frozen
backward; unused slots exactly zero; two runs the same bits.  Frozen means frozen; two data-parallel ranks equal one process."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _fwdcheck as F
import _gradcheck as G
import _softcheck as S
from cpt_amd import config as cfgmod
from cpt_amd import soft_prompt, synth
from oracle import cpt_oracle as O
from test_gpu_dp import _free_port
from test_gpu_dropout import SEED, _drop_dict

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _build(cfg, sd, dev, mode, template=None, n_slots=S.N_SLOTS):
    from cpt_amd.modeling_rec import REC_MLM_CPT
    m = REC_MLM_CPT(cfg)
    m.load_state_dict(sd)
    m.tie_weights()
    m.to(dev)
    m.set_compute_dtype(mode)
    w = soft_prompt.attach(m, n_slots=n_slots)
    if template is not None:
        with torch.no_grad():
            w.copy_(template.to(dev))
    return m


def _sd64(sd, dev):
    out = {k: v.to(dev, torch.float64) for k, v in sd.items()}
    out["cls.decoder.weight"] = out[S.WORD]
    return out


# ---- tiny: the fixture of the reference --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(dev):
    from cpt_amd.modeling_bert import BertImgForPreTraining
    from cpt_amd.modeling_rec import REC_MLM_CPT
    ck = os.path.join(GOLDEN, "tiny_ckpt")
    cfg = cfgmod.BertConfig.from_pretrained(ck)
    pre = BertImgForPreTraining.from_pretrained(ck, config=cfg)
    src = REC_MLM_CPT(cfg)
    src.copy_from_pretraining_model(pre)
    sd = {k: v.detach().clone() for k, v in src.state_dict().items()}
    g = np.load(os.path.join(GOLDEN, "soft_template_tiny.npz"))
    b = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("in_")}
    return cfg, sd, g, b


def _step(m, d, lab=None):
    for p in m.parameters():
        p.grad = None
    if lab is not None:
        loss, scores = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d.get("img_feats"), masked_lm_labels=lab)
    else:
        loss, scores = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d.get("img_feats"), masked_lm_labels=d["colors"],
                         mask_token_pos=d["mask_token_pos"])
    loss.backward()
    return loss.detach(), scores.detach(), soft_prompt.template_of(m).grad


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_tiny_forward_and_gradient_match_the_fixture(dev, tiny, mode):
    cfg, sd, g, b = tiny
    tmpl = torch.from_numpy(g["template"])
    m = _build(cfg, sd, dev, mode, tmpl).eval()
    d = {k: v.to(dev) for k, v in b.items()}
    with torch.no_grad():
        sc = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], mask_token_pos=d["mask_token_pos"])[0]
    loss, scores, grad = _step(m, d)
    assert tuple(grad.shape) == tuple(tmpl.shape) and grad.dtype == torch.float32
    sd64, d64 = _sd64(sd, dev), dict(d, img_feats=d["img_feats"].double())
    t64 = tmpl.to(dev, torch.float64)

    def oracle(bf16):
        l, gr, s = S.oracle_step(sd64, cfg.to_dict(), d64, t64, bf16=bf16)
        return {"template": gr, "loss": l.reshape(1), "scores": s}
    ref = oracle(False)
    emu = oracle(True) if mode == "bf16" else None
    # the oracle construction IS the fixture (CPU test), so this is the comparison with the reference's TemplateEmbedding
    assert float((ref["template"].cpu().float() - torch.from_numpy(g["grad_template"])).abs().max()) < 1e-5
    got = {"template": grad, "loss": loss.reshape(1), "scores": scores}
    print("\n" + G.table(G.compare(mode, got, ref, emu)))
    G.check(mode, got, ref, emu, "tiny %s" % mode)
    F.check(mode, {"mask_logits": sc}, {"mask_logits": ref["scores"]}, {"mask_logits": emu["scores"]} if emu else None, "tiny %s" % mode)
    unused = [s for s in range(S.N_SLOTS) if s not in S.USED]
    assert not bool(grad[unused].any()), "slots no position uses must have exactly zero gradient rows"
    assert all(bool(grad[s].any()) for s in S.USED)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_identity_template_and_slot_free_batch_give_the_detached_bits(dev, tiny, mode):
    cfg, sd, g, b = tiny
    d = {k: v.to(dev) for k, v in b.items()}

    def run(m, ids):
        with torch.no_grad():
            return m(ids, d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], mask_token_pos=d["mask_token_pos"])[0].clone()
    m = _build(cfg, sd, dev, mode).eval()                       # freshly attached: rows equal the word rows
    with_t = run(m, d["input_ids"])
    seq, pooled = m.bert(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"])
    soft_prompt.detach(m)
    assert torch.equal(with_t, run(m, d["input_ids"]))
    seq0, pooled0 = m.bert(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"])
    assert torch.equal(seq, seq0) and torch.equal(pooled, pooled0)
    # a template far from the word rows, a batch that uses none of its ids
    m2 = _build(cfg, sd, dev, mode, torch.from_numpy(g["template"]) + 1.0).eval()
    ids = d["input_ids"].clone()
    ids[(ids > 0) & (ids < S.N_SLOTS)] += 200
    free = run(m2, ids)
    assert not torch.equal(run(m2, d["input_ids"]), run(m, d["input_ids"]))     # (the template is live)
    soft_prompt.detach(m2)
    assert torch.equal(free, run(m2, ids))


def test_frozen_means_frozen(dev, tiny):
    from cpt_amd.train import _state
    cfg, sd, g, b = tiny
    m = _build(cfg, sd, dev, "fp32", torch.from_numpy(g["template"])).train()
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
    w = soft_prompt.template_of(m)
    opt = torch.optim.AdamW([w], lr=0.02, eps=1e-8)
    d = {k: v.to(dev) for k, v in b.items()}
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss, _ = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], masked_lm_labels=d["colors"],
                    mask_token_pos=d["mask_token_pos"])
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    for k, v in m.state_dict().items():
        if k == soft_prompt.KEY:
            assert not torch.equal(v, before[k])
        else:
            assert torch.equal(v, before[k]), k
    for n, p in m.named_parameters():
        assert (p.grad is None) == (n != soft_prompt.KEY), n
    assert losses[0] != losses[2] and losses[2] < losses[0]
    st = _state(m._engine())
    assert st.grad is None and st.sync is None                  # no flat gradient buffer, no gradient synchroniser
    # accumulation over micro-steps is plain addition (the kernel writes whole)
    _, _, g1 = _step(m, d)
    g1 = g1.clone()
    loss, _ = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], masked_lm_labels=d["colors"],
                mask_token_pos=d["mask_token_pos"])
    loss.backward()
    assert torch.equal(w.grad, g1 + g1)


# ---- Oscar-base: the plan regimes of the frozen backward ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base(dev):
    cfg = cfgmod.oscar_base()
    sd = synth.init_state_dict(cfg, 1234, head="cpt")           # N(0, 0.02) weights
    tmpl = S.make_template(sd[S.WORD], scale=0.02)
    models = {}

    def model(mode):
        if mode not in models:
            models[mode] = _build(cfgmod.oscar_base(), sd, dev, mode, tmpl).train()
        return models[mode]
    return sd, _sd64(sd, dev), tmpl, model


def _label_grid(b, dev):
    """Several labelled rows per sequence on even sequences, one on odd ones (behind the planted positions)."""
    B = b["input_ids"].size(0)
    lab = torch.full(b["attention_mask"].shape, -1, dtype=torch.long)
    for i in range(B):
        mp_ = int(b["mask_token_pos"][i])
        lab[i, mp_] = int(b["colors"][i])
        if i % 2 == 0:
            lab[i, 4] = int(synth.COLOR_IDS[i % 5])
            lab[i, mp_ + 1] = int(synth.COLOR_IDS[(i + 2) % 5])
    return lab.to(dev)


# mode, B, dropout, label grid, regions
BASE_CASES = [
    ("bf16", 4, 0.1, False, True),      # 480 rows: the pruned last layer, K-split data gradients whose fp32 partials the next LayerNorm backward adds
    ("bf16", 32, 0.1, False, True),     # 3840 rows: the bf16 partial pair (2048..6144 rows), lean LayerNorm, 8 rows per LayerNorm-backward workgroup
    ("bf16", 32, 0.0, True, True),      # a label grid: the unpruned last layer, head rows scattered by (sequence, position); dropout-free kernels
    ("bf16", 4, 0.1, False, False),     # Li = 0
    ("fp32", 4, 0.1, False, True),      # the unfused ln_bwd + dropout_rows branch
    ("bf16x3", 4, 0.0, False, True),    # ... on split operands
]


@pytest.mark.parametrize("mode,B,p,grid,regions", BASE_CASES, ids=["%s-B%d-p%g%s%s" % (c[0], c[1], c[2], "-grid" if c[3] else "", "" if c[4] else "-Li0")
                                                                   for c in BASE_CASES])
def test_base_gradient_matches_float64(dev, base, mode, B, p, grid, regions):
    from cpt_amd.train import set_dropout_seed
    sd, sd64, tmpl, model = base
    m = model(mode)
    cfg = m.config
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = p
    b = S.plant_slots(synth.make_batch(B, cfg, seed=2000 + B, vary_regions=True))
    if not regions:
        b = dict(b, attention_mask=b["attention_mask"][:, :b["input_ids"].size(1)].contiguous())
        del b["img_feats"]
    d = {k: v.to(dev) for k, v in b.items()}
    lab = _label_grid(b, dev) if grid else None
    set_dropout_seed(m, SEED, step=0)
    loss, scores, grad = _step(m, d, lab)
    first = grad.clone()
    set_dropout_seed(m, SEED, step=0)
    loss2, scores2, grad2 = _step(m, d, lab)
    # (the gradient: the forward's loss scalar is a sum of row losses in arrival order, as in the plain step)
    assert torch.equal(first, grad2) and torch.equal(scores, scores2), "two backward runs on the same inputs: the same bits"
    L = d["attention_mask"].size(1)
    drop = {k: v.to(dev) for k, v in _drop_dict(dev, cfg, p, 1, B, L).items()} if p > 0 else None
    d64 = dict(d, img_feats=d["img_feats"].double() if regions else None)
    t64 = tmpl.to(dev, torch.float64)

    def oracle(bf16):
        l, gr, s = S.oracle_step(sd64, cfg.to_dict(), d64, t64, drop=drop, labels=lab, bf16=bf16)
        return {"template": gr, "loss": l.reshape(1), "scores": s}
    ref = oracle(False)
    emu = oracle(True) if mode == "bf16" else None
    got = {"template": first, "loss": loss.reshape(1), "scores": scores}
    what = "%s B=%d p=%g%s%s" % (mode, B, p, " label grid" if grid else "", "" if regions else " Li=0")
    rows = G.compare(mode, got, ref, emu)
    print("\n%s\n%s" % (what, G.table(rows)))
    G.check(mode, got, ref, emu, what)
    unused = [s for s in range(S.N_SLOTS) if s not in S.USED]
    assert not bool(first[unused].any()) and all(bool(first[s].any()) for s in S.USED)
    for n, prm in m.named_parameters():
        assert (prm.grad is None) == (n != soft_prompt.KEY), n


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_base_forward_matches_float64(dev, base, mode):
    sd, sd64, tmpl, model = base
    m = model(mode)
    cfg = m.config
    B = 4
    b = S.plant_slots(synth.make_batch(B, cfg, seed=2000 + B, vary_regions=True))
    d = {k: v.to(dev) for k, v in b.items()}
    m.eval()
    try:
        with torch.no_grad():
            got = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], mask_token_pos=d["mask_token_pos"])[0]
    finally:
        m.train()
    st = S.oracle_state(sd64, tmpl.to(dev, torch.float64))

    def oracle(bf16):
        with torch.no_grad(), O.emulate_bf16(bf16):
            return O.rec_mlm_cpt_forward(st, cfg.to_dict(), d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"].double(),
                                         mask_rows_only=d["mask_token_pos"])[0]
    ref = {"mask_logits": oracle(False)}
    emu = {"mask_logits": oracle(True)} if mode == "bf16" else None
    print("\n" + F.table(F.compare(mode, {"mask_logits": got}, ref, emu), "base %s" % mode))
    F.check(mode, {"mask_logits": got}, ref, emu, "base %s" % mode)


# ---- data parallel: two ranks on one GPU over gloo, as tests/test_gpu_dp.py ---------------------------------------------------------
DP_STEPS = 2


def _dp_model(dev):
    cfg = cfgmod.tiny()
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
    sd = synth.init_state_dict(cfg, 1234, head="cpt")
    m = _build(cfg, sd, dev, "fp32", S.make_template(sd[S.WORD])).train()
    b = S.plant_slots(synth.make_batch(4, cfg, seed=S.TINY_BATCH_SEED, max_seq_len=20, img_seq_len=6))
    return m, {k: v.to(dev) for k, v in b.items()}


def _dp_run(m, b, rows):
    w = soft_prompt.template_of(m)
    opt = torch.optim.SGD([w], lr=1.0)
    d = {k: v[rows] for k, v in b.items()}
    for _ in range(DP_STEPS):
        opt.zero_grad()
        loss, _ = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], masked_lm_labels=d["colors"],
                    mask_token_pos=d["mask_token_pos"])
        loss.backward()
        opt.step()
    return w.detach().cpu().clone()


def _dp_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        m, b = _dp_model(dev)
        per = 4 // world
        torch.save(_dp_run(m, b, slice(rank * per, (rank + 1) * per)), os.path.join(tmp, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_two_ranks_equal_single_process(dev):
    world = 2
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_dp_worker, args=(world, _free_port(), tmp), nprocs=world, join=True)
        r = [torch.load(os.path.join(tmp, "r%d.pt" % i)) for i in range(world)]
    assert torch.equal(r[0], r[1]), "both ranks end with the same template"
    m, b = _dp_model(dev)
    start = soft_prompt.template_of(m).detach().cpu().clone()
    one = _dp_run(m, b, slice(0, 4))
    assert float((one - start).abs().max()) > 0
    assert G.rel(r[0] - start, one - start) <= G.FIXED["fp32"]
