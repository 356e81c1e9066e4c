"""CPU: length-aware training, host side.

* ``batching.label_extent`` / ``batching.trim_grid`` against a brute-force restatement on random masks and label grids, and on the edge
  cases: no region attended (Li' = 0), a label in the last text column, a batch attended to its last column (nothing cut), a grid
  without any label, a labelled region column (the text stays whole).
* The claim the feature rests on, independently of any HIP code: the float64 oracle on a padded batch and on its host-trimmed batch
  gives the same loss and the same parameter gradients to float64 rounding -- the trimmed rows contribute exact zeros -- for the MLM
  step ([MASK] rows and a label grid with several rows per sequence) and for the relation head on the pooled [CLS].
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cpt_amd import batching
from cpt_amd import config as cfgmod
from cpt_amd import synth
from oracle import cpt_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- extent and cut -------------------------------------------------------------------------------------------------------------------
def _brute_extent(mask, Lt, grid):
    """The rules of batching.batch_extent, column by column."""
    B, Lw = mask.shape
    Li = Lw - Lt
    lt, li = 1, 0
    for b in range(B):
        for c in range(Lw):
            if mask[b, c] != 0:
                if c < Lt:
                    lt = max(lt, c + 1)
                else:
                    li = max(li, c - Lt + 1)
    if grid is not None:
        for b in range(B):
            for c in range(Lw):
                if grid[b, c] != -1:
                    if c < Lt:
                        lt = max(lt, c + 1)
                    else:
                        lt = Lt
                        li = max(li, c - Lt + 1)
    return lt, li


def _brute_cut(grid, Lt, lt, li):
    return np.array([[row[c] for c in list(range(lt)) + list(range(Lt, Lt + li))] for row in grid], dtype=grid.dtype).reshape(grid.shape[0], lt + li)


def _random_case(rng, B, Lt, Li, region_label=False):
    mask = np.zeros((B, Lt + Li), np.int64)
    grid = np.full((B, Lt + Li), -1, np.int64)
    for b in range(B):
        t = int(rng.integers(1, Lt + 1))
        r = int(rng.integers(0, Li + 1))
        mask[b, :t] = 1
        mask[b, Lt:Lt + r] = 1
        if t > 2 and rng.random() < 0.3:
            mask[b, int(rng.integers(1, t - 1))] = 0            # a hole stays inside the extent
        for _ in range(int(rng.integers(0, 4))):
            grid[b, int(rng.integers(0, t))] = int(rng.integers(0, 30000))
        if region_label and Li and rng.random() < 0.5:
            grid[b, Lt + int(rng.integers(0, Li))] = 7
    return mask, grid


@pytest.mark.parametrize("seed", range(12))
def test_label_extent_and_cut_match_brute_force(seed):
    rng = np.random.default_rng(seed)
    B, Lt, Li = int(rng.integers(1, 6)), int(rng.integers(1, 24)), int(rng.integers(0, 9))
    mask, grid = _random_case(rng, B, Lt, Li, region_label=seed % 3 == 0)
    lt, li = batching.label_extent(mask, Lt, grid)
    assert (lt, li) == _brute_extent(mask, Lt, grid)
    assert batching.label_extent(mask, Lt) == _brute_extent(mask, Lt, None) == batching.batch_extent(mask, Lt)
    cut = batching.trim_grid(grid, Lt, lt, li)
    assert cut.shape == (B, lt + li) and (cut == _brute_cut(grid, Lt, lt, li)).all()
    # no label is lost and none moves relative to the text
    assert (cut != -1).sum() == (grid != -1).sum()
    rows, cols = np.nonzero(grid[:, :Lt] != -1)
    assert (cut[rows, cols] == grid[rows, cols]).all()
    # torch CPU tensors take the same route
    tcut = batching.trim_grid(torch.from_numpy(grid), Lt, lt, li)
    assert isinstance(tcut, torch.Tensor) and (tcut.numpy() == cut).all()
    assert batching.label_extent(torch.from_numpy(mask), Lt, torch.from_numpy(grid)) == (lt, li)


def test_edge_cases():
    Lt, Li = 8, 4
    mask = np.zeros((2, Lt + Li), np.int64)
    mask[0, :5] = 1
    mask[1, :3] = 1
    grid = np.full((2, Lt + Li), -1, np.int64)
    # an all -1 grid: the extent of the mask alone; Li' = 0
    assert batching.label_extent(mask, Lt, grid) == (5, 0)
    assert batching.trim_grid(grid, Lt, 5, 0).shape == (2, 5)
    # a label behind the attended text moves the extent; in the last text column it keeps the text whole
    grid[1, 6] = 11
    assert batching.label_extent(mask, Lt, grid) == (7, 0)
    grid[0, Lt - 1] = 12
    assert batching.label_extent(mask, Lt, grid) == (Lt, 0)
    cut = batching.trim_grid(grid, Lt, Lt, 0)
    assert cut[0, Lt - 1] == 12 and cut[1, 6] == 11
    # a labelled region column keeps the text whole and the region
    grid2 = np.full((2, Lt + Li), -1, np.int64)
    grid2[0, Lt + 2] = 5
    assert batching.label_extent(mask, Lt, grid2) == (Lt, 3)
    assert batching.trim_grid(grid2, Lt, Lt, 3)[0, Lt + 2] == 5
    # an all-attended batch: nothing cut, the grid comes back as it is
    full = np.ones((2, Lt + Li), np.int64)
    assert batching.label_extent(full, Lt, grid) == (Lt, Li)
    assert (batching.trim_grid(grid, Lt, Lt, Li) == grid).all()
    # an empty mask keeps the [CLS] column
    assert batching.label_extent(np.zeros((2, Lt + Li), np.int64), Lt, np.full((2, Lt + Li), -1)) == (1, 0)
    with pytest.raises(ValueError):
        batching.label_extent(mask, Lt, grid[:, :-1])
    with pytest.raises(ValueError):
        batching.trim_grid(grid, Lt, 0, 0)
    with pytest.raises(ValueError):
        batching.trim_grid(grid, Lt, Lt, Li + 1)


# ---- the float64 oracle: padded batch == trimmed batch ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """(cfg, REC_MLM_CPT state dict, pre-training state dict) of the tiny golden checkpoint, float64."""
    from cpt_amd.modeling_bert import BertImgForPreTraining
    from cpt_amd.modeling_rec import REC_MLM_CPT
    ck = os.path.join(GOLDEN, "tiny_ckpt")
    cfg = cfgmod.BertConfig.from_pretrained(ck)
    pre = BertImgForPreTraining.from_pretrained(ck, config=cfg)
    rec = REC_MLM_CPT(cfg)
    rec.copy_from_pretraining_model(pre)
    sd = {k: v.detach().double().clone() for k, v in rec.state_dict().items()}
    sd["cls.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"]
    pre_sd = {k: v.detach().double().clone() for k, v in pre.state_dict().items()}
    return cfg, sd, pre_sd


def _padded_batch(cfg, Lt=24, Li=8):
    """synth batch whose sequences are short inside a (Lt, Li) padding: region counts ragged, one sequence without regions."""
    b = synth.make_batch(4, cfg, seed=77, max_seq_len=Lt, img_seq_len=Li, n_regions=5, vary_regions=True)
    b["attention_mask"][2, Lt:] = 0
    b["img_feats"] = b["img_feats"].double()
    return b


def _close(a, b, what):
    if what.endswith("attention.self.key.bias"):
        # zero in exact arithmetic (softmax is shift-invariant): both sides hold float64 rounding noise only, as tests/_gradcheck.py notes
        assert float(a.abs().max()) < 1e-15 and float(b.abs().max()) < 1e-15, what
        return
    scale = max(float(a.abs().max()), float(b.abs().max()), 1e-30)
    assert float((a - b).abs().max()) <= 1e-11 * scale, (what, float((a - b).abs().max()), scale)


@pytest.mark.parametrize("grid", [False, True], ids=["mask-rows", "label-grid"])
def test_oracle_gradients_equal_on_the_trimmed_batch(tiny, grid):
    cfg, sd, _ = tiny
    b = _padded_batch(cfg)
    Lt = b["input_ids"].shape[1]
    lab = None
    if grid:
        lab = torch.full(b["attention_mask"].shape, -1, dtype=torch.long)
        for i in range(4):
            lab[i, int(b["mask_token_pos"][i])] = int(b["colors"][i])
            if i % 2 == 0:
                lab[i, 1] = int(synth.COLOR_IDS[i % 5]) % cfg.vocab_size
    full_grid = lab if grid else None
    lt, li = (batching.label_extent(b["attention_mask"], Lt, lab) if grid
              else batching.batch_extent(b["attention_mask"], Lt, b["mask_token_pos"]))
    assert lt < Lt and li < b["img_feats"].shape[1], "the case must cut something"
    t = batching.trim(b, lt, li)
    tlab = batching.trim_grid(lab, Lt, lt, li) if grid else None
    loss_p, grads_p, sc_p = O.train_step_grads(sd, cfg.to_dict(), b, labels=full_grid, with_scores=True)
    loss_t, grads_t, sc_t = O.train_step_grads(sd, cfg.to_dict(), t, labels=tlab, with_scores=True)
    _close(loss_p, loss_t, "loss")
    _close(sc_p, sc_t, "scores")
    n = 0
    for name, g in grads_p.items():
        if g is None:
            assert grads_t[name] is None
            continue
        _close(g, grads_t[name], name)
        n += 1
    assert n > 20
    # position rows behind the extent received exact zeros
    assert not bool(grads_p["bert.embeddings.position_embeddings.weight"][lt:Lt].any())


def test_oracle_relation_head_equal_on_the_trimmed_batch(tiny):
    cfg, _, pre_sd = tiny
    b = _padded_batch(cfg)
    Lt = b["input_ids"].shape[1]
    lt, li = batching.label_extent(b["attention_mask"], Lt)            # the relation head reads [CLS]: the mask alone
    assert lt < Lt and li < b["img_feats"].shape[1]
    t = batching.trim(b, lt, li)
    labels = torch.tensor([0, 1, 1, 0])

    def run(x):
        leaves = {k: v.clone().requires_grad_(True) for k, v in pre_sd.items() if k.startswith("bert.") or k.startswith("cls.seq_relationship")}
        _, pooled = O.bert_img_forward(leaves, cfg.to_dict(), x["input_ids"], x["segment_ids"], x["attention_mask"], None, x["img_feats"])
        rel = O.relation_head(leaves, pooled)
        loss = F.cross_entropy(rel, labels, ignore_index=-1)
        loss.backward()
        return loss.detach(), rel.detach(), {k: v.grad for k, v in leaves.items()}
    loss_p, rel_p, gp = run(b)
    loss_t, rel_t, gt = run(t)
    _close(loss_p, loss_t, "loss")
    _close(rel_p, rel_t, "rel")
    for name, g in gp.items():
        assert (g is None) == (gt[name] is None), name
        if g is not None:
            _close(g, gt[name], name)
