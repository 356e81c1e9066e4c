"""GPU: the Oscar-base training step (cpt_train_fwd_ex / cpt_train_bwd_ex through REC_MLM_CPT) against the float64 oracle on the
device, at the batch sizes where the step's kernel choices change.

Each case is the full 12-layer step on synth.make_batch (L = 70 + 50, M = 120 B rows) with dropout 0.1 and the masks the library
exports (tests/test_gpu_dropout.py); it checks the loss, the head rows' scores and EVERY parameter gradient with tests/_gradcheck.py:
fixed bounds in fp32 / bf16x3, ``rel_kernel <= C * rel_emulation + FLOOR`` in bf16 against the oracle's bf16 design emulation.
"""
import time

import pytest
import torch

import _gradcheck as G
from cpt_amd import config as cfgmod
from cpt_amd import synth
from oracle import cpt_oracle as O
from test_gpu_dropout import SEED, _drop_dict

pytestmark = pytest.mark.gpu
P = 0.1
LT, LI = 70, 50

# B -> the kernel choices it is there for (M = 120 B rows; csrc/gemm.hip gemm_nn / gemm_nt_partials, csrc/bwd.hip ln_bwd / embed_bwd /
# attention_bwd, csrc/train.hip).  bf16 throughout; the second field is make_batch's vary_regions (ragged region counts).
BF16_CASES = [
    (1, True),     # 120 rows: one head row; data gradients K-split 12 / 16 ways into fp32 partials (S >= 4 up to 1024 rows); LayerNorm backward
                   # one row per wave (4 rows per workgroup below 2048 rows); attention backward one workgroup per phase
    (4, False),    # 480: configs[2]'s per-GPU share; narrow 64 x 96 forward and 64 x 128 GELU-gradient tiles (<= 512 rows); phase split
    (8, True),     # 960: the last K-split (S = 4) data gradients; 64 x 64 attention-output data gradient (<= 1024 rows); embed_bwd 4 rows per workgroup
    (11, False),   # 1320: attention-backward phase split off (2 * 11 * 12 > 256); data gradients unsplit (whole K per 64-row tile, residual epilogue)
    (16, True),    # 1920: just below 2048: no split2 pair, no lean LayerNorm; embed_bwd 16 rows per workgroup (from 1024 text rows: B >= 15)
    (18, False),   # 2160: split2 bf16 partial pairs, lean LayerNorm, LayerNorm backward 8 rows per workgroup, 256 x 192 GELU-gradient tiles;
                   # ragged last 128- and 256-row tiles
    (32, True),    # 3840: the bench training shape (triple TN launch, Q|K|V partials reduced by the next layer's launch)
    (34, False),   # 4080: the first B with the 256-row GELU-gradient tiles off (128-row tiles: 512 workgroups); split2 still on
    (51, True),    # 6120: split2 last on (M <= 6144)
    (52, False),   # 6240: split2 off: the whole-K GEMM with the residual epilogue again
    (53, True),    # 6360: `small` (64-row tiles) off for N = 768: 50 x 4 = 200 workgroups of 128 rows
]
ADVICE_B = (18, 32)      # split2 rounds the data gradient to bf16 twice per layer: layer 0 and the embeddings must stay within C too


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    sd = synth.init_state_dict(cfgmod.oscar_base(), 1234, head="cpt")
    sd64 = {k: v.to(dev, torch.float64) for k, v in sd.items()}
    sd64["cls.decoder.weight"] = sd64["bert.embeddings.word_embeddings.weight"]
    models = {}

    def model(mode):
        from cpt_amd.modeling_rec import REC_MLM_CPT
        if mode not in models:
            m = REC_MLM_CPT(cfgmod.oscar_base())
            m.load_state_dict(sd)
            m.tie_weights()
            m.to(dev).train()
            m.set_compute_dtype(mode)
            models[mode] = m
        return models[mode]
    return dev, sd64, model


def _label_grid(b, dev):
    """Several labelled rows per sequence (the [MASK] slot, position 1, the slot after [MASK]) on even sequences, one on odd ones."""
    B = b["input_ids"].size(0)
    lab = torch.full(b["attention_mask"].shape, -1, dtype=torch.long)
    for i in range(B):
        mp = int(b["mask_token_pos"][i])
        lab[i, mp] = int(b["colors"][i])
        if i % 2 == 0:
            lab[i, 1] = int(synth.COLOR_IDS[i % 5])
            lab[i, mp + 1] = int(synth.COLOR_IDS[(i + 2) % 5])
    return lab.to(dev)


def _run(env, mode, B, vary=False, p=P, grid=False):
    dev, sd64, model = env
    m = model(mode)
    cfg = m.config
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = p
    from cpt_amd.train import set_dropout_seed
    set_dropout_seed(m, SEED, step=0)
    for prm in m.parameters():
        prm.grad = None
    b = synth.make_batch(B, cfg, seed=1000 + B, vary_regions=vary)
    d = {k: v.to(dev) for k, v in b.items()}
    lab = _label_grid(b, dev) if grid else None
    t0 = time.time()
    if grid:
        loss, scores = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], masked_lm_labels=lab)
    else:
        loss, scores = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], masked_lm_labels=d["colors"],
                         mask_token_pos=d["mask_token_pos"])
    loss.backward()
    torch.cuda.synchronize()
    t1 = time.time()
    got = {n: prm.grad for n, prm in m.named_parameters()}
    got["loss"], got["scores"] = loss.detach().reshape(1), scores.detach()
    drop = None
    if p > 0:
        drop = {k: v.to(dev) for k, v in _drop_dict(dev, cfg, p, 1, B, LT + LI).items()}      # first training forward -> step 1
    d64 = dict(d, img_feats=d["img_feats"].double())
    cd = cfg.to_dict()

    def oracle(bf16):
        loss_r, grads, sc = O.train_step_grads(sd64, cd, d64, drop=drop, labels=lab, bf16=bf16, with_scores=True)
        grads["loss"], grads["scores"] = loss_r.reshape(1), sc
        return grads
    ref = oracle(False)
    emu = oracle(True) if mode == "bf16" else None
    torch.cuda.synchronize()
    t2 = time.time()
    what = "%s B=%d%s p=%g%s" % (mode, B, " ragged" if vary else "", p, " label grid" if grid else "")
    rows = G.compare(mode, got, ref, emu)
    s = G.summary(rows)
    print("\n%s: step %.2f s, oracle %.2f s; worst %s: layer 11 %.3g, layer 0 %.3g, embeddings %.3g, head %.3g | matrix %.3g, bias %.3g, "
          "layernorm %.3g, table %.3g, loss %.3g, scores %.3g" % (what, t1 - t0, t2 - t1, "ratio" if emu else "rel", s["layer 11"], s["layer 0"],
                                                                 s["embeddings"], s["head"], s["matrix"], s["bias"], s["layernorm"], s["table"],
                                                                 s["loss"], s["scores"]))
    print(G.table(rows))
    G.check(mode, got, ref, emu, what)
    return rows


@pytest.mark.parametrize("B,vary", BF16_CASES, ids=["B%d" % b for b, _ in BF16_CASES])
def test_bf16_gradients_match_emulation(env, B, vary):
    rows = _run(env, "bf16", B, vary)
    if B in ADVICE_B:
        # split2 (2048..6144 rows) leaves each data gradient of the residual stream as two bf16 partial matrices: its error must not
        # grow towards layer 0 and the embedding tables faster than the design's own
        early = [r for r in rows if r["group"] in ("layer 0", "embeddings") and r["cls"] in ("matrix", "table", "layernorm")
                 and r["emu"] >= G.FLOOR]
        assert early
        worst = max(early, key=G.ratio)
        assert G.ratio(worst) <= G.C, (worst["name"], G.ratio(worst))


@pytest.mark.parametrize("mode,B", [(m, b) for m in ("fp32", "bf16x3") for b in (4, 18, 32)])
def test_parity_modes_match_float64(env, mode, B):
    _run(env, mode, B, vary=B == 18)


def test_bf16_without_dropout(env):
    _run(env, "bf16", 32, vary=True, p=0.0)        # p = 0: the dropout-free kernels


def test_bf16_label_grid(env):
    _run(env, "bf16", 32, vary=False, grid=True)   # n_rows head rows, the last layer on all rows (tail off)
