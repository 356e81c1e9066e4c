"""GPU: the RefCOCO REC evaluation on the device.  cpt_rec_choose on planted scores against scoring.rec_eval_reference -- everything compared for
equality: indices, score bits, IoU bits, flags, counts, candidate scores -- and against the reference's own val() (tests/golden/tiny_rec_eval.npz);
then drivers.val_rec on the tiny model against drivers.val_queries + scoring.accuracy, with the length-aware options and over two ranks."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _receval as RE
import test_gpu_gqa_vcr as G
import test_gpu_trim_drivers as T
from cpt_amd import scoring as S

pytestmark = pytest.mark.gpu
GOLDEN = G.GOLDEN
W = {"red": 5, "purple": 6, "green": 7, "yellow": 8, "blue": 9, "none": RE.NONE_ID}
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _check(qs, gts, scores, dev, few_shot, want_idx=None, what=""):
    """The table of qs, one launch over all of them, compared with the host restatement; returns (buffers, reference)."""
    t = S.rec_eval_table(qs, gts, RE.NONE_ID)
    ref = S.rec_eval_reference(scores, t, few_shot)
    got = RE.run_device(scores, t, few_shot, dev)
    RE.assert_same(got, ref, what)
    assert int(got["counts"][0]) == int(got["correct"].sum())
    if want_idx is not None:
        assert ref["idx"].tolist() == want_idx, (what, ref["idx"])
    return got, ref


# ---- the kernel -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("few_shot", [False, True])
def test_one_query_one_sequence_one_colour(dev, few_shot):
    got, _ = _check([RE.query([1])], [[0, 0, 21, 31]], RE.grid_scores(1, 1), dev, few_shot, [0])
    assert got["iou"].tolist() == [1.0] and got["counts"].tolist() == [1, 1]


@pytest.mark.parametrize("few_shot", [False, True])
def test_sequences_of_5_5_and_2_colours_pad_the_column_table(dev, few_shot):
    qs = [RE.query([5, 5, 2]), RE.query([2, 5]), RE.query([1, 1, 1, 4])]
    gts = [[10, 4, 30, 40], [0, 0, 21, 31], [9, 2, 25.5, 33.25]]
    for seed in (1, 2, 3):
        sc = RE.grid_scores(9, seed)
        sc[2, W["purple"]] = 4.0 + seed                                        # query 0: the last candidate, inside the padded row
        _check(qs, gts, sc, dev, few_shot, what=seed)
    assert S.rec_eval_table(qs, gts, RE.NONE_ID)["cols"][2].tolist() == [5, 6, -1, -1, -1]


@pytest.mark.parametrize("few_shot", [False, True])
def test_seventy_candidates_take_a_second_lane_trip(dev, few_shot):
    """14 sequences x 5 colours: candidates 64..69 belong to lanes 0..5 on their second trip.  Equal maxima at 3 and 67 -- lane 3 holds both -- and
    at 3 and 66 -- two lanes: the lower index wins across the trip boundary either way; alone, 67 wins."""
    qs, gts = [RE.query([5] * 14)], [[90, 15, 25, 44]]
    base = RE.grid_scores(14, 11)
    base[:, RE.NONE_ID] = 1.0
    for cells, want in (((3, 67), 3), ((3, 66), 3), ((67,), 67), ((64, 69), 64), ((63, 64), 63)):
        sc = base.clone()
        for c in cells:
            sc[c // 5, RE.COLOURS[c % 5]] = 5.0
        _check(qs, gts, sc, dev, few_shot, [want], cells)


@pytest.mark.parametrize("few_shot", [False, True])
def test_more_than_64_sequences_cross_the_sequence_block(dev, few_shot):
    """The kernel places candidates through per-lane colour counts of 64 sequences at a time: 70 sequences of 2, 3, 4, 2, 3, 4 .. colours (three
    lane trips in the first block of sequences), a sequence without a colour in each block, a second query behind it, maxima tied inside a
    block, across the block boundary and alone in the second block."""
    counts = [i % 3 + 2 for i in range(70)]
    counts[5] = counts[66] = 0
    qs, gts = [RE.query(counts), RE.query([2, 2])], [[90, 15, 25, 44], [0, 0, 21, 31]]
    first = np.cumsum([0] + counts).tolist()
    assert 128 < first[64] <= 192 and first[70] > first[64] + 10
    for seed, cells in ((1, ()), (2, ((3, 0), (68, 1))), (3, ((68, 3),)), (4, ((63, 1), (64, 2))), (5, ((69, 0),)), (6, ((40, 2), (41, 0)))):
        sc = RE.grid_scores(72, seed)
        sc[:70, RE.NONE_ID] = 1.0
        for s, c in cells:
            sc[s, RE.COLOURS[c]] = 5.0
        _, ref = _check(qs, gts, sc, dev, few_shot, what=cells)
        if cells:
            assert int(ref["idx"][0]) == first[cells[0][0]] + cells[0][1], cells


def test_nan_counts_as_the_maximum_and_the_first_nan_wins(dev):
    qs, gts = [RE.query([5, 5]), RE.query([5] * 14)], [[0, 0, 21, 31], [90, 15, 25, 44]]
    sc = RE.grid_scores(16, 5)
    sc[1, W["green"]] = NAN                                                    # query 0: one NaN among numbers, candidate 7
    sc[2 + 13, W["purple"]] = NAN                                              # query 1: NaNs at 66 and 2 -- the first wins, across the lane trips
    sc[2 + 0, W["green"]] = NAN
    got, _ = _check(qs, gts, sc, dev, False, [7, 2])
    assert np.isnan(got["score"].cpu().numpy()).all()


def test_negative_zero_ties_with_positive_zero(dev):
    qs, gts = [RE.query([4]), RE.query([4])], [[0, 0, 21, 31]] * 2
    sc = -RE.grid_scores(2, 9).abs() - 1.0
    sc[0, W["purple"]], sc[0, W["yellow"]] = -0.0, 0.0                         # the first of the two equal maxima, whatever its sign
    sc[1, W["purple"]], sc[1, W["yellow"]] = 0.0, -0.0
    got, _ = _check(qs, gts, sc, dev, False, [1, 1])
    assert RE.bits(got["score"].cpu().numpy()).tolist() == RE.bits(np.array([-0.0, 0.0], dtype=np.float32)).tolist()


def test_few_shot_divides_by_a_negative_and_by_a_zero_none_logit(dev):
    qs = [RE.query([3, 3]), RE.query([3]), RE.query([3]), RE.query([3, 3])]
    gts = [[0, 0, 21, 31]] * 4
    sc = torch.zeros(6, RE.V)
    sc[0, 5:8], sc[0, RE.NONE_ID] = torch.tensor([3.0, 1.0, 0.5]), 2.0         # q0: 1.5 .. against -1.5 / -0.5 = 3 in the second sequence
    sc[1, 5:8], sc[1, RE.NONE_ID] = torch.tensor([2.0, -1.5, 0.25]), -0.5
    sc[2, 5:8], sc[2, RE.NONE_ID] = torch.tensor([-1.0, 2.0, 3.0]), 0.0        # q1: -inf, +inf, +inf: the first +inf
    sc[3, 5:8], sc[3, RE.NONE_ID] = torch.tensor([4.0, 0.0, -2.0]), 0.0        # q2: +inf, 0 / 0 = NaN, -inf: the NaN
    sc[4, 5:8], sc[4, RE.NONE_ID] = torch.tensor([1.0, 2.0, 3.0]), -0.0        # q3: -inf x 3, then a finite sequence
    sc[5, 5:8], sc[5, RE.NONE_ID] = torch.tensor([1.0, -2.0, 0.5]), 4.0
    got, _ = _check(qs, gts, sc, dev, True, [4, 1, 1, 3])
    assert got["score"].cpu().tolist()[:2] == [3.0, INF] and np.isnan(float(got["score"][2]))
    _check(qs, gts, sc, dev, False, [0, 2, 0, 2])


@pytest.mark.parametrize("mode", ["zsl", "fsl"])
def test_kernel_reproduces_the_reference_val_fixture(dev, mode):
    """IoU exactly 0.5 (not correct), touching boxes (intersection 0), fractional coordinates -- the case that differs in its last bits when the
    compiler fuses w1 * h1 + w2 * h2 --, the tie between two sequences and the negative "none" logit, as the reference's val() decided them."""
    g, qs, gts = RE.fixture(GOLDEN)
    t = S.rec_eval_table(qs, gts, int(g["none_id"]))
    scores = torch.from_numpy(g["scores"])
    got = RE.run_device(scores, t, mode == "fsl", dev)
    iou = got["iou"].cpu().numpy()
    print("iou", iou.tolist(), "fused forms of query 0", g["fused_iou_q0"].tolist())
    assert got["idx"].cpu().tolist() == g[mode + "_max_idx"].tolist()
    assert np.array_equal(RE.bits(iou), RE.bits(g[mode + "_iou"])), (iou, g[mode + "_iou"])
    assert got["correct"].cpu().tolist() == g[mode + "_correct"].astype(np.uint8).tolist()
    assert got["counts"].cpu().tolist() == [int(g[mode + "_correct"].sum()), len(qs)]
    assert int(got["counts"][0]) / int(got["counts"][1]) * 100 == float(g[mode + "_percent"])
    assert iou[1] == 0.5 and not got["correct"][1] and iou[2] == 0.0 and all(iou[0] != x for x in g["fused_iou_q0"].tolist())
    RE.assert_same(got, S.rec_eval_reference(scores, t, mode == "fsl"))


@pytest.mark.parametrize("few_shot", [False, True])
def test_queries_without_a_colour_or_an_annotation_are_written_and_not_counted(dev, few_shot):
    qs = [RE.query([2, 3]), {"colors": [[], []], "rects": [[], []]}, RE.query([3]), {"colors": [], "rects": []}, RE.query([1, 2])]
    gts = [[0, 0, 21, 31], [1, 1, 5, 5], None, [1, 1, 5, 5], [7, 1, 21, 32]]
    got, ref = _check(qs, gts, RE.grid_scores(7, 4), dev, few_shot)
    assert got["idx"].cpu().tolist()[1::2] == [-1, -1] and int(got["idx"][2]) >= 0
    assert got["score"].cpu().tolist()[1::2] == [-INF, -INF] and np.isnan(got["iou"].cpu().numpy()[1:4]).all()
    assert int(got["counts"][1]) == 2 and got["correct"].cpu().tolist()[1:4] == [0, 0, 0]


def _sentinels(table, dev, candidate_scores=True):
    out = S.rec_eval_buffers(table, dev, candidate_scores)
    out["idx"].fill_(-7)
    out["score"].fill_(123.0)
    out["iou"].fill_(-3.0)
    out["correct"].fill_(9)
    if candidate_scores:
        out["cand_score"].fill_(77.0)
    return out


@pytest.mark.parametrize("few_shot", [False, True])
def test_q_index_descending_and_a_subset_write_their_global_slots_only(dev, few_shot):
    qs = [RE.query([2, 3]), RE.query([5] * 14), RE.query([3]), RE.query([1, 2]), RE.query([4, 4, 1]), RE.query([2])]
    gts = [[0, 0, 21, 31], [90, 15, 25, 44], [2, 1, 20, 30], None, [7, 1, 21, 32], [1, 0, 22, 31]]
    t = S.rec_eval_table(qs, gts, RE.NONE_ID)
    scores = RE.grid_scores(int(t["seq_first"][-1]), 13)
    ref = S.rec_eval_reference(scores, t, few_shot)
    cf = t["cand_first"].tolist()
    for order in ([5, 4, 3, 2, 1, 0], [4, 1], [3, 5, 0], [2]):
        out = RE.run_device(scores, t, few_shot, dev, q_index=order, out=_sentinels(t, dev))
        host = {k: v.cpu().numpy() for k, v in out.items()}
        judged = [q for q in order if gts[q] is not None]
        assert host["counts"].tolist() == [int(sum(ref["correct"][q] for q in judged)), len(judged)], order
        for q in range(len(qs)):
            cs = host["cand_score"][cf[q]:cf[q + 1]]
            if q in order:
                assert host["idx"][q] == ref["idx"][q] and host["correct"][q] == ref["correct"][q], (order, q)
                assert RE.bits(host["score"][q:q + 1])[0] == RE.bits(ref["score"][q:q + 1])[0], (order, q)
                assert RE.bits(host["iou"][q:q + 1])[0] == RE.bits(ref["iou"][q:q + 1])[0], (order, q)
                assert np.array_equal(RE.bits(cs), RE.bits(ref["cand_score"][cf[q]:cf[q + 1]])), (order, q)
            else:
                assert (host["idx"][q], host["score"][q], host["iou"][q], host["correct"][q]) == (-7, 123.0, -3.0, 9), (order, q)
                assert (cs == 77.0).all(), (order, q)


def test_two_launches_add_into_the_same_counts_and_cand_score_may_be_null(dev):
    g, qs, gts = RE.fixture(GOLDEN)
    t = S.rec_eval_table(qs, gts, int(g["none_id"]))
    scores = torch.from_numpy(g["scores"])
    ref = S.rec_eval_reference(scores, t, False)
    for cand in (True, False):
        out = S.rec_eval_buffers(t, dev, cand)
        assert (out["cand_score"] is not None) == cand
        RE.run_device(scores, t, False, dev, q_index=[0, 1, 2], out=out)
        first = out["counts"].cpu().tolist()
        RE.run_device(scores, t, False, dev, q_index=[6, 5, 4, 3], out=out)
        assert first == [int(ref["correct"][:3].sum()), 3]
        RE.assert_same(out, ref, cand)
        assert int(out["counts"][0]) == int(out["correct"].sum())
    # a pass repeats bit for bit, and the column list of colour_columns_only gives the same result on the same columns
    col_ids = [5, 6, 7, 8, 9, 10]
    tc = S.rec_eval_table(qs, gts, int(g["none_id"]), col_ids)
    RE.assert_same(RE.run_device(scores[:, col_ids].contiguous(), tc, True, dev), S.rec_eval_reference(scores, t, True))


def test_wrapper_refuses_what_the_kernel_would_read_out_of_bounds(dev):
    qs, gts = [RE.query([2, 3]), RE.query([3])], [[0, 0, 21, 31], None]
    t = S.rec_eval_table(qs, gts, RE.NONE_ID)
    out = S.rec_eval_buffers(t, dev)
    ok = torch.zeros(3, RE.V, device=dev)
    for rows, q_index in ((ok[:2], [0, 1]), (ok, [0, 2]), (ok, [0, 0]), (ok, []), (ok[:, :10], [0, 1]), (ok.double(), [0, 1])):
        with pytest.raises(ValueError):
            S.rec_choose_device(rows, q_index, t, False, out)
    with pytest.raises(ValueError):
        S.rec_choose_device(ok, [0, 1], t, False, dict(out, idx=out["idx"].long()))


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------------
def _driver_queries(cfg, n=11, seed=5):
    """The ragged queries of the length-aware tests, one of them without a colour, and their annotations: query 0's is far larger than any box (a
    miss whatever is chosen), query 1's boxes are moved onto one another (a hit whatever is chosen), the others' are made from one candidate
    box each (hit or miss by the choice); query 7 has none."""
    qs = T._queries(cfg, n, seed)
    qs[4]["colors"] = [[] for _ in qs[4]["colors"]]
    qs[4]["rects"] = [[] for _ in qs[4]["rects"]]
    qs[1]["rects"] = [[[50 + k, 50 + j, 150 + k, 150 + j] for k in range(len(c))] for j, c in enumerate(qs[1]["colors"])]
    gts = []
    for i, q in enumerate(qs):
        flat = [r for rs in q["rects"] for r in rs] or [[0, 0, 9, 9]]
        r = flat[(3 * i) % len(flat)]
        gts.append([r[0] + (i % 3), r[1], r[2] - r[0] + 1, r[3] - r[1] + 1.5])
    gts[0], gts[1], gts[7] = [0, 0, 1000, 1000], [51, 51, 101.5, 101.0], None
    return qs, gts


def _host_accuracy(preds, gts):
    judged = {k: v[1] for k, v in preds.items() if v[1] is not None and gts[k] is not None}
    return S.accuracy(judged, gts), len(judged)


def _assert_driver(res, want, gts):
    assert res["predictions"] == want and list(res["predictions"]) == list(want)
    acc, n = _host_accuracy(want, gts)
    assert res["accuracy"] == acc and res["n_evaluated"] == n
    assert res["n_unpredicted"] == sum(1 for v in want.values() if v[0] < 0)
    for k, (idx, rect) in want.items():
        if rect is not None and gts[k] is not None:
            iou = S.compute_iou([rect[0], rect[1], rect[2] - rect[0] + 1, rect[3] - rect[1] + 1], gts[k])
            assert res["iou"][k] == iou and res["correct"][k] == (iou > 0.5), k
        else:
            assert np.isnan(res["iou"][k]) and res["correct"][k] == 0, k
    assert int(res["correct"].sum()) == round(res["accuracy"] * n / 100)


DRIVER_OPTIONS = [dict(), dict(trim=True), dict(bucket=True), dict(max_sequences=7), dict(trim=True, bucket=True, max_sequences=7),
                  dict(colour_columns_only=False), dict(colour_columns_only=False, trim=True, bucket=True)]


@pytest.mark.parametrize("few_shot", [False, True])
def test_val_rec_matches_val_queries_and_host_accuracy(dev, few_shot):
    from cpt_amd import drivers
    m = G._gqa_model(dev).eval()
    qs, gts = _driver_queries(m.config)
    plain = None
    for opts in DRIVER_OPTIONS:
        want = drivers.val_queries(m, qs, 10, dev, few_shot=few_shot, batch_queries=3, **opts)
        res = drivers.val_rec(m, qs, gts, 10, dev, few_shot=few_shot, batch_queries=3, return_candidate_scores=True, **opts)
        _assert_driver(res, want, gts)
        assert 0 < res["accuracy"] < 100 and res["n_unpredicted"] == 1 and res["n_evaluated"] == len(qs) - 2
        assert res["candidate_scores"].shape == (sum(len(c) for q in qs for c in q["colors"]),)
        if plain is None:
            plain = res
    # a table built once serves several passes; one built for another column choice is refused
    table = S.rec_eval_table(qs, gts, 10, sorted({c for q in qs for s in q["colors"] for c in s} | {10}))
    again = drivers.val_rec(m, qs, gts, 10, dev, few_shot=few_shot, batch_queries=3, table=table)
    assert again["predictions"] == plain["predictions"] and again["accuracy"] == plain["accuracy"] and "candidate_scores" not in again
    assert np.array_equal(RE.bits(again["iou"]), RE.bits(plain["iou"]))
    with pytest.raises(ValueError):
        drivers.val_rec(m, qs, gts, 10, dev, colour_columns_only=False, table=table)


def _rec_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cpt_amd import drivers
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        m = G._gqa_model(dev).eval()
        qs, gts = _driver_queries(m.config)
        res = {fs: drivers.val_rec(m, qs, gts, 10, dev, few_shot=fs, batch_queries=3, bucket=fs, return_candidate_scores=True) for fs in (False, True)}
        torch.save(res, os.path.join(tmp, "v%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_val_rec_two_ranks_equal_single_process(dev):
    """Both ranks share cuda:0 over gloo, as the val_queries case of test_gpu_dp.py; 11 queries do not divide by 2."""
    from cpt_amd import drivers
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_rec_worker, args=(2, G._free_port(), tmp), nprocs=2, join=True)
        r = [torch.load(os.path.join(tmp, "v%d.pt" % i), weights_only=False) for i in range(2)]
    m = G._gqa_model(dev).eval()
    qs, gts = _driver_queries(m.config)
    for fs in (False, True):
        single = drivers.val_rec(m, qs, gts, 10, dev, few_shot=fs, batch_queries=3, return_candidate_scores=True)
        for x in r:
            a = x[fs]
            assert a["predictions"] == single["predictions"] and a["accuracy"] == single["accuracy"]
            assert (a["n_evaluated"], a["n_unpredicted"]) == (single["n_evaluated"], single["n_unpredicted"])
            for k in ("correct", "iou", "score", "candidate_scores"):      # sequences are independent and every kernel is batch-invariant
                assert a[k].dtype == single[k].dtype and np.array_equal(a[k].view(np.uint8), single[k].view(np.uint8)), (fs, k)
