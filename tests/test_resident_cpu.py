"""CPU: the host side of the device-resident evaluation sets (cpt_amd/resident.py) -- the tables, their numpy gather and their extents
against the host path they replace (torch.cat of the items, batching.batch_extent, batching.trim), bit for bit; the refusals; the per-rank
tables of a data-parallel run.  The item generators are shared with tests/test_gpu_resident.py."""
import numpy as np
import pytest
import torch

from cpt_amd import batching as BT
from cpt_amd import dist as cdist
from cpt_amd import drivers
from cpt_amd import resident as R

LT, LI, D = 12, 5, 6
KEYS = ("input_ids", "segment_ids", "attention_mask", "mask_token_pos", "img_feats")


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.int32)


def ragged_queries(Lt=LT, Li=LI, dim=D, seed=0, n=9):
    """RefCOCO-layout queries of 1..4 sequences with everything the tables have to get right: blocks of 0 and of Li regions, a zero row in the
    middle of a block, a trailing row of -0.0, a (Li, D) array expanded over a query's sequences, the same array handed to two queries, a mask
    with a hole (text and regions), a [MASK] position in the region part."""
    rng = np.random.Generator(np.random.PCG64(seed))
    qs = []
    for i in range(n):
        P = int(rng.integers(1, 5))
        text = int(rng.integers(3, Lt + 1)) if i != 2 else Lt
        regions = [0, Li, 2, 3, 1, Li, 4, 2, 3][i % 9] if Li else 0
        regions = min(regions, Li)
        q = {"input_ids": torch.zeros((P, Lt), dtype=torch.int64), "segment_ids": torch.zeros((P, Lt), dtype=torch.int64),
             "attention_mask": torch.zeros((P, Lt + Li), dtype=torch.int64), "img_feats": torch.zeros((P, Li, dim))}
        for p in range(P):
            t = max(2, text - p)
            q["input_ids"][p, :t] = torch.from_numpy(rng.integers(1, 30000, t))
            q["segment_ids"][p, t // 2:t] = 1
            q["attention_mask"][p, :t] = 1
            r = max(0, regions - (p % 2))
            q["attention_mask"][p, Lt:Lt + r] = 1
            q["img_feats"][p, :r] = torch.from_numpy(rng.standard_normal((r, dim)).astype(np.float32))
        q["mask_token_pos"] = torch.from_numpy(rng.integers(1, max(2, text - P + 1), P))
        if i == 3:                              # a non-prefix mask: holes in the text part and in the region part
            q["attention_mask"][0, 1] = 0
            q["attention_mask"][0, Lt] = 0
        if i == 4 and Li:                       # a [MASK] position in the region part
            q["mask_token_pos"][0] = Lt + 1
        if i == 5 and Li >= 3:                  # a zero row in the middle of a block: it stays
            q["img_feats"][0, 1] = 0
        if i == 6 and Li:                       # a trailing row of -0.0 behind the attended regions: not zero, it stays
            q["img_feats"][0, Li - 1] = -0.0
        if i == 7 and Li:                       # one (Li, D) array expanded over the sequences: ONE block
            q["img_feats"] = q["img_feats"][0].clone().expand(P, Li, dim)
        q["colors"] = [[int(c) for c in rng.choice([5, 6, 7, 8, 9], size=int(rng.integers(1, 4)), replace=False)] for _ in range(P)]
        q["rects"] = [[[10 * j, 5 * k, 10 * j + 30, 5 * k + 40] for k in range(len(q["colors"][j]))] for j in range(P)]
        qs.append(q)
    twin = dict(qs[1])                          # the same feature array handed in twice (its own text rows)
    twin["input_ids"] = qs[1]["input_ids"].flip(0).clone()
    qs.append(twin)
    return qs


def gqa_questions(Lt=LT, Li=LI, dim=D, seed=1, n=7):
    """GQA-layout questions (1-D rows, img_feats (Li, D)); questions 2 i and 2 i + 1 share their image's array."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out, feats = [], None
    for i in range(n):
        if i % 2 == 0:
            r = int(rng.integers(0, Li + 1))
            feats = torch.zeros((Li, dim))
            feats[:r] = torch.from_numpy(rng.standard_normal((r, dim)).astype(np.float32))
        t = int(rng.integers(3, Lt + 1))
        ids, mask = np.zeros(Lt, np.int64), np.zeros(Lt + Li, np.int64)
        ids[:t] = rng.integers(1, 30000, t)
        mask[:t] = 1
        mask[Lt:Lt + r] = 1
        out.append({"input_ids": ids, "segment_ids": np.zeros(Lt, np.int64), "input_mask": mask, "img_feats": feats,
                    "mask_token_pos": [int(rng.integers(1, t)), 0], "igt": [i % 3], "q_id": 100 + i})
    return out


def host_flat(qs):
    """The host concatenation of the queries: one row per sequence."""
    return {k: torch.cat([q[k] for q in qs], 0) for k in KEYS}


def host_flat_gqa(qs):
    t = torch.as_tensor
    return {"input_ids": torch.stack([t(q["input_ids"]) for q in qs]), "segment_ids": torch.stack([t(q["segment_ids"]) for q in qs]),
            "attention_mask": torch.stack([t(q["input_mask"]) for q in qs]), "img_feats": torch.stack([t(q["img_feats"]) for q in qs]),
            "mask_token_pos": torch.tensor([int(q["mask_token_pos"][0]) for q in qs], dtype=torch.int64)}


def host_batch(flat, seq_idx, lt, li):
    """batching.trim of the rows seq_idx of the host concatenation."""
    idx = torch.as_tensor(np.asarray(seq_idx, np.int64))
    return BT.trim({k: v[idx] for k, v in flat.items()}, lt, li)


def assert_same_batch(got, want):
    for k in KEYS:
        g, w = np.asarray(got[k]), want[k].numpy()
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        if k == "img_feats":
            assert np.array_equal(bits(g), bits(w)), k
        else:
            assert np.array_equal(g, w), k


SEQ_LISTS = lambda S: [list(range(S)), [0], [S - 1, S - 1, 0, 0], list(range(S - 1, -1, -1)), [3, 1, 3, 2, 1]]
CUTS = [(1, 0), (1, 1), (LT, 0), (LT, LI), (5, 3)]


def test_gather_reference_equals_trim_of_host_concatenation():
    qs = ragged_queries()
    t = R.tables(R.from_queries(qs))
    flat = host_flat(qs)
    S = flat["input_ids"].size(0)
    assert t["n_seq"] == S == int(t["seq_first"][-1]) and t["seq_base"] == 0 and (t["Lt"], t["Li"], t["D"]) == (LT, LI, D)
    assert t["ids"].dtype == np.int32 and t["seg"].dtype == np.uint8 and t["mask"].dtype == np.uint8 and t["mask_pos"].dtype == np.int32
    assert 0 in t["block_rows"] and LI in t["block_rows"]
    for idx in SEQ_LISTS(S):
        for lt, li in CUTS + [R.extent(t, idx)]:
            assert_same_batch(R.gather_reference(t, idx, lt, li), host_batch(flat, idx, lt, li))


def test_blocks_rows_and_sharing():
    qs = ragged_queries()
    t = R.tables(R.from_queries(qs))
    sf = t["seq_first"]
    # -0.0 is not zero: the block of query 6's first sequence reaches its last row; a zero row in the middle of query 5's stays
    assert t["block_rows"][t["feat_block"][sf[6]]] == LI
    assert R.block_rows_of(np.array([[0, 0], [1, 0], [0, 0], [0, -0.0], [0, 0]], np.float32)) == 4
    assert R.block_rows_of(np.zeros((3, 2), np.float32)) == 0 and R.block_rows_of(np.zeros((0, 2), np.float32)) == 0
    b5 = t["feat_block"][sf[5]]
    assert t["block_rows"][b5] >= 3 and not t["feats"][t["block_off"][b5] + 1].any()
    # an expanded (Li, D) array is one block for all its sequences; the same array handed in twice shares its blocks
    assert len(set(t["feat_block"][sf[7]:sf[8]].tolist())) == 1
    assert t["feat_block"][sf[1]:sf[2]].tolist() == t["feat_block"][sf[len(qs) - 1]:sf[len(qs)]].tolist()
    n_blocks = sum(q["input_ids"].size(0) for i, q in enumerate(qs[:-1]) if i != 7) + 1
    assert len(t["block_rows"]) == n_blocks
    assert t["feats"].shape == (int(t["block_rows"].sum()), D) and t["block_off"].tolist() == (np.cumsum(t["block_rows"]) - t["block_rows"]).tolist()
    assert R.pitch_of(2054, "fp32") == 2056 and R.pitch_of(2054, "bf16") == 2056 and R.pitch_of(37, "fp32") == 40 and R.pitch_of(38, "bf16") == 40
    assert R.store_bytes(t, "bf16") < R.store_bytes(t, "fp32")


def test_gqa_layout_shares_blocks():
    qs = gqa_questions()
    t = R.tables(R.from_questions(qs))
    flat = host_flat_gqa(qs)
    assert t["n_seq"] == len(qs) and t["seq_first"].tolist() == list(range(len(qs) + 1))
    assert len(t["block_rows"]) == (len(qs) + 1) // 2 and t["feat_block"].tolist() == [i // 2 for i in range(len(qs))]
    for idx in SEQ_LISTS(len(qs)):
        for lt, li in CUTS + [R.extent(t, idx)]:
            assert_same_batch(R.gather_reference(t, idx, lt, li), host_batch(flat, idx, lt, li))


@pytest.mark.parametrize("walk", [dict(), dict(bucket=True), dict(cap=5), dict(cap=3, bucket=True)])
def test_extent_equals_batch_extent_on_every_batch(walk):
    qs = ragged_queries(seed=3, n=14)
    t = R.tables(R.from_queries(qs))
    sf = t["seq_first"]
    host_keys = [drivers._item_length(q["attention_mask"], LT) for q in qs]
    assert R.item_keys(t) == host_keys
    counts = [q["input_ids"].size(0) for q in qs]
    assert counts == (sf[1:] - sf[:-1]).tolist()
    groups = drivers._walk(len(qs), 3, host_keys if walk.get("bucket") else None, counts if "cap" in walk else None, walk.get("cap"))
    assert sorted(i for g in groups for i in g) == list(range(len(qs)))
    for g in groups:
        seqs = np.concatenate([np.arange(sf[i], sf[i + 1]) for i in g])
        mask = torch.cat([qs[i]["attention_mask"] for i in g], 0)
        pos = torch.cat([qs[i]["mask_token_pos"] for i in g], 0)
        assert R.extent(t, seqs) == BT.batch_extent(mask, LT, pos)
        assert R.extent(t, seqs, head=False) == BT.batch_extent(mask, LT)
    # a position outside the sequence keeps both parts whole
    t["mask_pos"][0] = LT + LI + 3
    assert R.extent(t, [0]) == (LT, LI)


def test_refusals():
    def broken(change):
        qs = ragged_queries(n=3)
        change(qs)
        return R.from_queries(qs)

    def set_(key, at, value):
        def run(qs):
            qs[1][key] = qs[1][key].clone()
            qs[1][key][at] = value
        return run
    with pytest.raises(ValueError, match="attention_mask"):
        R.tables(broken(set_("attention_mask", (0, 0), 2)))
    with pytest.raises(ValueError, match="attention_mask"):
        R.tables(broken(set_("attention_mask", (0, 0), -1)))
    with pytest.raises(ValueError, match="input_ids"):
        R.tables(broken(set_("input_ids", (0, 1), 2 ** 31)))
    with pytest.raises(ValueError, match="padded"):           # another Lt (the mask keeps its Li)
        R.tables(broken(lambda qs: qs[2].update(input_ids=qs[2]["input_ids"][:, :LT - 1], segment_ids=qs[2]["segment_ids"][:, :LT - 1],
                                                attention_mask=qs[2]["attention_mask"][:, 1:])))
    with pytest.raises(ValueError, match="padded"):           # another Li
        R.tables(broken(lambda qs: qs[2].update(attention_mask=qs[2]["attention_mask"][:, :-1], img_feats=qs[2]["img_feats"][:, :-1])))
    with pytest.raises(ValueError, match="dimension"):        # another D
        R.tables(broken(lambda qs: qs[2].update(img_feats=qs[2]["img_feats"][:, :, :-1])))
    t = R.tables(R.from_queries(ragged_queries(n=3)))
    with pytest.raises(ValueError):
        R.gather_reference(t, [t["n_seq"]], 1, 0)
    with pytest.raises(ValueError):
        R.extent(t, [-1])
    with pytest.raises(ValueError):
        R.store_bytes(t, "fp16")


@pytest.mark.parametrize("world", [2, 3])
def test_rank_tables_cover_their_shard_and_nothing_else(world):
    qs = ragged_queries(seed=5, n=10)
    items = R.from_queries(qs)
    whole = R.tables(items)
    S, seen = whole["n_seq"], []
    for rank in range(world):
        lo, hi = cdist.shard_range(len(qs), rank, world)
        t = R.tables(items, (lo, hi))
        alone = R.tables(R.from_queries(qs[lo:hi]))              # what the shard's items hold by themselves
        assert (t["item_lo"], t["item_hi"]) == (lo, hi) and t["n_items"] == len(qs)
        assert t["seq_first"].tolist() == whole["seq_first"].tolist()                       # every item's sequence count: indices stay global
        assert t["seq_base"] == whole["seq_first"][lo] and t["n_seq"] == whole["seq_first"][hi] - whole["seq_first"][lo]
        for k in ("ids", "seg", "mask", "mask_pos", "feat_block", "block_rows", "block_off", "feats", "text_len", "regions"):
            assert np.array_equal(t[k], alone[k]), k
        mine = list(range(t["seq_base"], t["seq_base"] + t["n_seq"]))
        seen += mine
        ext = R.extent(whole, mine)
        assert R.extent(t, mine) == ext
        got, want = R.gather_reference(t, mine[::-1], *ext), R.gather_reference(whole, mine[::-1], *ext)
        for k in got:
            assert np.array_equal(got[k], want[k]) and (k != "img_feats" or np.array_equal(bits(got[k]), bits(want[k])))
        for outside in ([t["seq_base"] - 1] if lo else []) + ([t["seq_base"] + t["n_seq"]] if hi < len(qs) else []):
            with pytest.raises(ValueError):
                R.gather_reference(t, [outside], 1, 0)
    assert seen == list(range(S))
