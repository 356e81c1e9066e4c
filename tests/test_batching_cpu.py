"""CPU: cpt_amd/batching.py -- extents of a padded batch, trimming, the length order and query packing (pure numpy, no GPU)."""
import numpy as np
import pytest
import torch

from cpt_amd import batching as BT


def _mask(rows, Lt, Li):
    """rows: per sequence (set text indices, set region indices) -> (B, Lt + Li) int64."""
    m = np.zeros((len(rows), Lt + Li), np.int64)
    for b, (t, r) in enumerate(rows):
        m[b, list(t)] = 1
        m[b, [Lt + j for j in r]] = 1
    return m


def test_extents_hole_empty_and_full_parts():
    Lt, Li = 7, 5
    m = _mask([((0, 1, 4), (0, 3)),          # a hole at text 2..3 and at regions 1..2: both stay inside the extent
               ((0, 1, 2), ()),              # no region attended
               (range(7), range(5)),         # both parts full
               ((), (4,))], Lt, Li)          # no text at all, only the last region
    t, r = BT.extents(m, Lt)
    assert t.tolist() == [5, 3, 7, 0] and r.tolist() == [4, 0, 5, 5]
    assert BT.batch_extent(m, Lt) == (7, 5)
    assert BT.batch_extent(m[:2], Lt) == (5, 4)
    assert BT.batch_extent(m[1:2], Lt) == (3, 0)                      # Li' may be 0
    assert BT.batch_extent(m[3:], Lt) == (1, 5)                       # Lt' >= 1: the [CLS] row stays
    assert BT.batch_extent(torch.from_numpy(m[:2]), Lt) == (5, 4)     # CPU tensors as well
    # text only (Li = 0)
    assert [x.tolist() for x in BT.extents(m[:, :Lt], Lt)] == [[5, 3, 7, 0], [0, 0, 0, 0]]
    with pytest.raises(ValueError):
        BT.extents(m, 0)


def test_head_rows_widen_the_extent():
    Lt, Li = 7, 5
    m = _mask([((0, 1, 2), (0,)), ((0, 1), ())], Lt, Li)
    assert BT.batch_extent(m, Lt) == (3, 1)
    assert BT.batch_extent(m, Lt, np.array([1, 5])) == (6, 1)         # a [MASK] slot beyond the last attended text index
    assert BT.batch_extent(m, Lt, np.array([[0, 2], [0, 4], [1, 1]])) == (5, 1)      # (sequence, position) pairs
    assert BT.batch_extent(m, Lt, torch.tensor([6, 0])) == (7, 1)     # the last text slot
    assert BT.batch_extent(m, Lt, np.array([0, 9])) == (7, 3)         # a region row: the text stays whole, regions reach it
    assert BT.batch_extent(m, Lt, np.array([0, 12])) == (7, 5)        # outside the sequence: nothing is trimmed
    assert BT.batch_extent(m, Lt, np.array([-1, 0])) == (7, 5)


@pytest.mark.parametrize("as_tensor", [False, True])
def test_trim_equals_the_slices(as_tensor):
    rng = np.random.Generator(np.random.PCG64(5))
    B, Lt, Li, D = 3, 7, 5, 6
    b = {"input_ids": rng.integers(0, 100, (B, Lt)), "segment_ids": rng.integers(0, 2, (B, Lt)), "position_ids": rng.integers(0, 30, (B, Lt)),
         "attention_mask": rng.integers(0, 2, (B, Lt + Li)), "img_feats": rng.standard_normal((B, Li, D)).astype(np.float32),
         "mask_token_pos": np.array([1, 2, 0])}
    if as_tensor:
        b = {k: torch.from_numpy(v) for k, v in b.items()}
    for lt, li in ((4, 2), (7, 5), (1, 0), (7, 0)):
        o = BT.trim(b, lt, li)
        eq = (lambda x, y: torch.equal(x, y)) if as_tensor else (lambda x, y: np.array_equal(x, y))
        for k in ("input_ids", "segment_ids", "position_ids"):
            assert eq(o[k], b[k][:, :lt])
        assert tuple(o["img_feats"].shape) == (B, li, D) and eq(o["img_feats"], b["img_feats"][:, :li])
        assert tuple(o["attention_mask"].shape) == (B, lt + li)
        assert eq(o["attention_mask"][:, :lt], b["attention_mask"][:, :lt]) and eq(o["attention_mask"][:, lt:], b["attention_mask"][:, Lt:Lt + li])
        assert o["mask_token_pos"] is b["mask_token_pos"]              # passed through
        assert tuple(b["input_ids"].shape) == (B, Lt)                  # the input dict is left as it was
    # optional entries may be missing or None
    o = BT.trim({"input_ids": b["input_ids"], "attention_mask": b["attention_mask"][:, :Lt], "img_feats": None}, 3, 0)
    assert tuple(o["input_ids"].shape) == (B, 3) and tuple(o["attention_mask"].shape) == (B, 3) and o["img_feats"] is None
    for bad in ((0, 2), (8, 2), (4, 6), (4, -1)):
        with pytest.raises(ValueError):
            BT.trim(b, *bad)


def test_trim_to_the_batch_extent_keeps_every_attended_column():
    Lt, Li = 9, 6
    m = _mask([((0, 1, 5), (1,)), ((0, 2), (0, 3))], Lt, Li)
    lt, li = BT.batch_extent(m, Lt)
    o = BT.trim({"input_ids": np.zeros((2, Lt), np.int64), "attention_mask": m}, lt, li)
    assert (lt, li) == (6, 4) and int(o["attention_mask"].sum()) == int(m.sum())


def test_length_order_is_stable_and_invertible():
    t = np.array([5, 3, 5, 1, 3, 9])
    r = np.array([1, 3, 1, 0, 3, 0])            # keys 6 6 6 1 6 9
    order, inv = BT.length_order(t, r)
    assert order.tolist() == [3, 0, 1, 2, 4, 5]                       # equal keys keep their order
    x = np.arange(6) * 10
    assert (x[order][inv] == x).all() and (inv[order] == np.arange(6)).all()
    order, inv = BT.length_order([], [])
    assert order.size == 0 and inv.size == 0


def test_pack_queries():
    counts = [3, 4, 9, 1, 1, 1, 8, 2, 7]
    groups = BT.pack_queries(counts, 8)
    assert groups == [[0, 1], [2], [3, 4, 5], [6], [7], [8]]
    assert [i for g in groups for i in g] == list(range(len(counts)))             # whole queries, consecutive, nothing split or lost
    assert all(sum(counts[i] for i in g) <= 8 or len(g) == 1 for g in groups)      # the cap holds; an oversize query is alone
    assert [2] in groups
    assert BT.pack_queries([], 4) == []
    assert BT.pack_queries([2, 2, 2], 100) == [[0, 1, 2]]
    assert BT.pack_queries([5, 5], 1) == [[0], [1]]
    with pytest.raises(ValueError):
        BT.pack_queries([1], 0)
    rng = np.random.Generator(np.random.PCG64(9))
    counts = rng.integers(1, 41, 200).tolist()
    groups = BT.pack_queries(counts, 64)
    assert [i for g in groups for i in g] == list(range(200))
    assert all(sum(counts[i] for i in g) <= 64 for g in groups)
    # greedy: the next query would not have fitted
    assert all(sum(counts[i] for i in g) + counts[g[-1] + 1] > 64 for g in groups[:-1])
