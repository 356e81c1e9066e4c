"""GPU: device-resident evaluation sets.  cpt_gather_batch against its numpy restatement (resident.gather_reference) by equality, into
outputs pre-filled with a sentinel; the drivers with a ResidentSet against the same drivers on host items, every field by its bits; the bf16
store against the engine dtype; a second pass that uploads nothing but its index list.  Everything here is equality: the gathered batch holds
the host batch's bits and the forward repeats bit for bit on equal inputs."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import test_gpu_gqa_vcr as G
import test_gpu_rec_eval as RE
import test_gpu_trim_drivers as T
import test_resident_cpu as RC
from cpt_amd import dist as cdist
from cpt_amd import drivers
from cpt_amd import ops
from cpt_amd import resident as R
from cpt_amd import scoring as SC

pytestmark = pytest.mark.gpu
LT = 12
INT_SENTINEL = -7777
NAN_BITS = 0x7FC12345                            # a quiet NaN with a payload: no gathered feature has these bits


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------
def _sentinels(B, lt, li, dim, dev):
    out = {k: torch.full(shape, INT_SENTINEL, dtype=torch.int64, device=dev)
           for k, shape in (("input_ids", (B, lt)), ("segment_ids", (B, lt)), ("attention_mask", (B, lt + li)), ("mask_token_pos", (B,)))}
    out["img_feats"] = torch.full((B, li, dim), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    return out


def _bf16_round(feats, dev):
    """The library's own bf16 rounding of (B, Li', D) fp32 features, widened back to fp32."""
    B, li, dim = feats.shape
    if B * li == 0:
        return feats
    x = torch.from_numpy(feats).to(dev).view(B * li, dim).contiguous()
    return ops.pad_cast(x, dim + dim % 2, torch.bfloat16)[:, :dim].float().view(B, li, dim).cpu().numpy()


@pytest.mark.parametrize("feature_dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("dim,Li", [(2054, 50), (38, 5), (37, 5)])       # the real row shape (odd rows 8-byte aligned only), a small even D, the scalar path
def test_gather_batch_equals_reference(dev, dim, Li, feature_dtype, monkeypatch):
    qs = RC.ragged_queries(Lt=LT, Li=Li, dim=dim, seed=2)
    t = R.tables(R.from_queries(qs))
    if dim == 38:
        monkeypatch.setattr(R, "CHUNK_BYTES", 3 * 4 * dim)              # three feature rows per chunk: the upload walks many chunks
    rs = R.upload(t, dev, feature_dtype)
    assert rs.n_items == len(qs) and rs.n_sequences == t["n_seq"] and rs.nbytes == R.store_bytes(t, feature_dtype)
    sf, S = t["seq_first"], t["n_seq"]
    empty, full, shared = int(sf[0]), int(sf[1]), int(sf[7])            # a block of 0 rows, one of Li rows, one shared by its query's sequences
    assert t["block_rows"][t["feat_block"][empty]] == 0 and t["block_rows"][t["feat_block"][full]] == Li
    lists = [[full], [empty], [shared + 1, empty, shared + 1], [S - 1, full, shared]]
    if dim == 2054:
        lists = [[S - 1, full, shared, full, 2]]                        # B = 5: about 2 MB of features
    for idx in lists:
        B = len(idx)
        seq = torch.tensor(idx, dtype=torch.int32, device=dev)
        for lt in (1, LT):
            for li in (0, 1, Li):
                for with_pos in (True, False):
                    want = R.gather_reference(t, idx, lt, li)
                    if feature_dtype == "bf16":
                        want["img_feats"] = _bf16_round(want["img_feats"], dev)
                    pre = _sentinels(B, lt, li, dim, dev)
                    got = rs.gather(seq, lt, li, mask_pos=with_pos, out=pre)
                    for k in ("input_ids", "segment_ids", "attention_mask"):
                        assert got[k].data_ptr() == pre[k].data_ptr() and np.array_equal(got[k].cpu().numpy(), want[k]), (k, idx, lt, li)
                    if with_pos:
                        assert np.array_equal(got["mask_token_pos"].cpu().numpy(), want["mask_token_pos"]), (idx, lt, li)
                    else:
                        assert got["mask_token_pos"] is None and bool((pre["mask_token_pos"] == INT_SENTINEL).all())
                    gf = pre["img_feats"].view(torch.int32).cpu().numpy()
                    assert gf.shape == (B, li, dim) and np.array_equal(gf, RC.bits(want["img_feats"])), (idx, lt, li)
    # an index outside the store is clamped to its nearest sequence (the Python side validates; the kernel never reads outside)
    got = rs.gather(torch.tensor([-5, S + 3], dtype=torch.int32, device=dev), LT, Li)
    want = R.gather_reference(t, [0, S - 1], LT, Li)
    assert np.array_equal(got["input_ids"].cpu().numpy(), want["input_ids"]) and np.array_equal(got["attention_mask"].cpu().numpy(), want["attention_mask"])
    if feature_dtype == "fp32":
        assert np.array_equal(RC.bits(got["img_feats"].cpu().numpy()), RC.bits(want["img_feats"]))
    rs.free()
    assert rs.nbytes == 0
    with pytest.raises(RuntimeError):
        rs.gather(torch.zeros(1, dtype=torch.int32, device=dev), 1, 0)


def test_gather_batch_gqa_layout_and_refusals(dev):
    qs = RC.gqa_questions()
    t = R.tables(R.from_questions(qs))
    rs = R.upload(R.from_questions(qs), dev)
    idx = [5, 0, 5, 4, 1]
    got = rs.gather(torch.tensor(idx, dtype=torch.int32, device=dev), *R.extent(t, idx))
    RC.assert_same_batch({k: v.cpu().numpy() for k, v in got.items()}, RC.host_batch(RC.host_flat_gqa(qs), idx, *R.extent(t, idx)))
    with pytest.raises(ValueError, match="bf16"):                       # the size needed and the way out are named
        R.upload(t, dev, max_bytes=16)
    with pytest.raises(ValueError):
        rs.gather(torch.tensor(idx, dtype=torch.int64, device=dev), 1, 0)
    with pytest.raises(RuntimeError, match="cpt_gather_batch"):
        rs.gather(torch.tensor(idx, dtype=torch.int32, device=dev), RC.LT + 1, 0)


def test_gather_from_a_rank_shard_takes_global_indices(dev):
    """A rank's store holds its shard's sequences only; seq_idx stays global (seq_base)."""
    qs = RC.ragged_queries(seed=5, n=10)
    items = R.from_queries(qs)
    whole = R.tables(items)
    for rank in range(3):
        lo, hi = cdist.shard_range(len(qs), rank, 3)
        t = R.tables(items, (lo, hi))
        rs = R.upload(t, dev)
        mine = list(range(t["seq_base"], t["seq_base"] + t["n_seq"]))[::-1]
        assert (rs.item_lo, rs.item_hi, rs.n_items, rs.n_sequences) == (lo, hi, len(qs), whole["n_seq"]) and (rank == 0 or t["seq_base"] > 0)
        ext = R.extent(whole, mine)
        got = rs.gather(torch.tensor(mine, dtype=torch.int32, device=dev), *ext)
        want = R.gather_reference(whole, mine, *ext)
        for k in RC.KEYS:
            assert np.array_equal(got[k].cpu().numpy(), want[k]), (rank, k)
        assert np.array_equal(RC.bits(got["img_feats"].cpu().numpy()), RC.bits(want["img_feats"]))


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------
OPTIONS = [dict(), dict(trim=True), dict(trim=True, bucket=True), dict(max_sequences=7)]
GQA_OPTIONS = [dict(), dict(trim=True), dict(trim=True, bucket=True), dict(bucket=True)]       # (val_gqa packs by questions: no max_sequences)


def _same(a, b, where=""):
    """Equal in every field: arrays and tensors by their bits, containers element by element."""
    assert type(a) is type(b), (where, type(a), type(b))
    if isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], "%s[%r]" % (where, k))
    elif isinstance(a, (np.ndarray, torch.Tensor)):
        x, y = np.asarray(a), np.asarray(b)
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), where
    elif isinstance(a, float):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), (where, a, b)
    else:
        assert a == b, (where, a, b)


def _model(dev, mode):
    m = G._gqa_model(dev).eval()
    m.set_compute_dtype(mode)
    return m


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_val_queries_and_val_rec_resident_equal_host(dev, mode):
    m = _model(dev, mode)
    qs, gts = RE._driver_queries(m.config)
    rs = R.upload(R.from_queries(qs), dev)
    shapes = T.Shapes(m)
    for opts in OPTIONS:
        for few_shot in (False, True):
            want = drivers.val_queries(m, qs, 10, dev, few_shot=few_shot, batch_queries=3, **opts)
            ran = shapes.take()
            got = drivers.val_queries(m, qs, 10, dev, few_shot=few_shot, batch_queries=3, resident=rs, **opts)
            assert shapes.take() == ran, opts                           # the same shapes ran, trimmed ones included
            _same(got, want, "val_queries %s" % opts)
            if opts.get("trim"):
                assert all(s[1] <= 24 for s in ran) and T._rows_run(ran) < sum(s[0] * (T.LT + T.LI) for s in ran)
        want = drivers.val_rec(m, qs, gts, 10, dev, batch_queries=3, return_candidate_scores=True, **opts)
        ran = shapes.take()
        got = drivers.val_rec(m, qs, gts, 10, dev, batch_queries=3, return_candidate_scores=True, resident=rs, **opts)
        assert shapes.take() == ran, opts
        _same(got, want, "val_rec %s" % opts)
        assert 0 < got["accuracy"] < 100 and "candidate_scores" in got
    # a set built from other items is refused by its counts
    other = R.upload(R.from_queries(qs[:-1]), dev)
    with pytest.raises(ValueError, match="other items"):
        drivers.val_queries(m, qs, 10, dev, resident=other)
    with pytest.raises(ValueError, match="other items"):
        drivers.val_rec(m, qs, gts, 10, dev, resident=other)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_val_gqa_resident_equals_host(dev, mode):
    m = _model(dev, mode)
    tok, qs = T._gqa_questions(10, 7)
    rs = R.upload(R.from_questions(qs), dev)
    shapes = T.Shapes(m)
    for opts in GQA_OPTIONS:
        want = drivers.val_gqa(m, qs, G.GQA_LABELS, tok, dev, batch_questions=4, **opts)
        ran = shapes.take()
        got = drivers.val_gqa(m, qs, G.GQA_LABELS, tok, dev, batch_questions=4, resident=rs, **opts)
        assert shapes.take() == ran, opts
        _same(got, want, "val_gqa %s" % opts)
        if opts.get("trim"):
            assert T._rows_run(ran) < sum(s[0] * (T.LT + T.LI) for s in ran)


def test_bf16_store_is_exact_in_bf16_mode_and_refused_elsewhere(dev):
    m = _model(dev, "bf16")
    qs, gts = RE._driver_queries(m.config)
    tok, gq = T._gqa_questions(10, 7)
    full, half = R.upload(R.from_queries(qs), dev), R.upload(R.from_queries(qs), dev, feature_dtype="bf16")
    assert half.nbytes < full.nbytes
    for opts in (dict(), dict(trim=True, bucket=True)):
        a = drivers.val_rec(m, qs, gts, 10, dev, batch_queries=3, return_candidate_scores=True, resident=full, **opts)
        b = drivers.val_rec(m, qs, gts, 10, dev, batch_queries=3, return_candidate_scores=True, resident=half, **opts)
        _same(b, a, "bf16 store %s" % opts)
    ghalf = R.upload(R.from_questions(gq), dev, feature_dtype="bf16")
    _same(drivers.val_gqa(m, gq, G.GQA_LABELS, tok, dev, batch_questions=4, resident=ghalf),
          drivers.val_gqa(m, gq, G.GQA_LABELS, tok, dev, batch_questions=4), "bf16 store, val_gqa")
    m.set_compute_dtype("fp32")
    for run in (lambda: drivers.val_queries(m, qs, 10, dev, resident=half), lambda: drivers.val_rec(m, qs, gts, 10, dev, resident=half),
                lambda: drivers.val_gqa(m, gq, G.GQA_LABELS, tok, dev, resident=ghalf)):
        with pytest.raises(ValueError, match="bf16"):
            run()


def test_second_pass_uploads_only_its_index_list(dev):
    m = _model(dev, "fp32")
    qs, gts = RE._driver_queries(m.config)
    for counter in R.H2D.values():
        counter.clear()
    rs = R.upload(R.from_queries(qs), dev)
    assert R.H2D["calls"]["tables"] > 0 and R.H2D["calls"]["features"] > 0 and R.H2D["bytes"]["features"] == 4 * rs.tables["block_rows"].sum() * rs.D
    table = SC.rec_eval_table(qs, gts, 10, sorted({c for q in qs for s in q["colors"] for c in s} | {10}))      # (uploaded once, as the set is)
    S_total = rs.n_sequences
    for opts in (dict(), dict(trim=True, bucket=True, max_sequences=7)):
        first = drivers.val_rec(m, qs, gts, 10, dev, batch_queries=3, return_candidate_scores=True, resident=rs, table=table, **opts)
        for counter in R.H2D.values():
            counter.clear()
        again = drivers.val_rec(m, qs, gts, 10, dev, batch_queries=3, return_candidate_scores=True, resident=rs, table=table, **opts)
        _same(again, first, "second pass %s" % opts)
        assert dict(R.H2D["calls"]) == {"seq_idx": 1} and dict(R.H2D["bytes"]) == {"seq_idx": 4 * S_total}, (opts, R.H2D)


def _resident_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        m = _model(dev, "fp32")
        qs, gts = RE._driver_queries(m.config)
        tok, gq = T._gqa_questions(10, 7)
        rs, grs = R.upload(R.from_queries(qs), dev), R.upload(R.from_questions(gq), dev)          # (each rank: its shard_range only)
        assert (rs.item_lo, rs.item_hi) == cdist.shard_range(len(qs), rank, world) and rs.tables["n_seq"] < rs.n_sequences
        rec = dict(batch_queries=3, trim=True, bucket=True, return_candidate_scores=True)
        res = {"rec": drivers.val_rec(m, qs, gts, 10, dev, resident=rs, **rec),
               "gqa": drivers.val_gqa(m, gq, G.GQA_LABELS, tok, dev, batch_questions=3, trim=True, resident=grs)}
        _same(res, {"rec": drivers.val_rec(m, qs, gts, 10, dev, **rec),
                    "gqa": drivers.val_gqa(m, gq, G.GQA_LABELS, tok, dev, batch_questions=3, trim=True)}, "rank %d" % rank)
        torch.save(res, os.path.join(tmp, "v%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_resident_shards_equal_two_ranks_on_host_items(dev):
    """Both ranks share cuda:0 over gloo, as the val_rec case of test_gpu_rec_eval.py.  Every rank uploads and walks its own shard and
    compares the gathered results with the host-item pass of the same two ranks; both ranks end with the same gathered results."""
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_resident_worker, args=(2, G._free_port(), tmp), nprocs=2, join=True)
        r = [torch.load(os.path.join(tmp, "v%d.pt" % i), weights_only=False) for i in range(2)]
    _same(r[0], r[1], "rank 0 against rank 1")
    assert len(r[0]["rec"]["predictions"]) == 11 and len(r[0]["gqa"]["q_ids"]) == 10
