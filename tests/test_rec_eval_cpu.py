"""CPU: the host side of the RefCOCO REC evaluation -- scoring.rec_eval_table's layout and refusals, and scoring.rec_eval_reference against the
reference's own val() functions and computeIoU (tests/golden/tiny_rec_eval.npz, tools/make_golden_rec_eval.py) and against the host path a user
runs today (scoring.select_region + scoring.accuracy)."""
import numpy as np
import pytest
import torch

import _receval as RE
from cpt_amd import scoring as S


def _hand_queries():
    q0 = {"colors": [[5, 9, 7], [6]], "rects": [[[0, 0, 10, 10], [1.5, 2.5, 30.25, 40.75], [5, 5, 6, 6]], [[2, 3, 9, 11]]]}
    q1 = {"colors": [], "rects": []}                                           # a query without a sequence
    q2 = {"colors": [[], [8, 5]], "rects": [[], [[3, 3, 4, 4], [7, 7, 70, 70]]]}     # a sequence without a colour
    return [q0, q1, q2], [[0, 0, 11, 11], None, [7.5, 7.5, 60.0, 60.0]]


def test_table_layout_offsets_padding_and_column_remap():
    qs, gts = _hand_queries()
    t = S.rec_eval_table(qs, gts, none_id=10)
    assert t["seq_first"].tolist() == [0, 2, 2, 4] and t["seq_first"].dtype == torch.int32
    assert t["cand_first"].tolist() == [0, 4, 4, 6] and t["cand_first"].dtype == torch.int32
    assert t["cols"].dtype == torch.int32 and t["cols"].tolist() == [[5, 9, 7], [6, -1, -1], [-1, -1, -1], [8, 5, -1]]
    assert t["rects"].dtype == torch.float64 and t["rects"].shape == (6, 4)
    assert t["rects"].tolist() == [[0, 0, 10, 10], [1.5, 2.5, 30.25, 40.75], [5, 5, 6, 6], [2, 3, 9, 11], [3, 3, 4, 4], [7, 7, 70, 70]]
    assert t["gt"].dtype == torch.float64 and t["gt"].tolist() == [[0, 0, 11, 11], [0, 0, 0, 0], [7.5, 7.5, 60, 60]]
    assert t["has_gt"].dtype == torch.uint8 and t["has_gt"].tolist() == [1, 0, 1]
    assert (t["n_queries"], t["C"], t["none"], t["none_id"], t["col_ids"], t["n_cols_min"]) == (3, 3, 10, 10, None, 11)
    # with a column list the ids become positions in it, the "none" column too; gts may be a dict keyed by query index
    col_ids = [5, 6, 7, 8, 9, 10]
    r = S.rec_eval_table(qs, {0: gts[0], 2: gts[2]}, none_id=10, col_ids=col_ids)
    assert r["cols"].tolist() == [[0, 4, 2], [1, -1, -1], [-1, -1, -1], [3, 0, -1]]
    assert (r["none"], r["col_ids"], r["n_cols_min"]) == (5, col_ids, 6)
    for k in ("seq_first", "cand_first", "rects", "gt", "has_gt"):
        assert torch.equal(r[k], t[k]), k
    with pytest.raises(ValueError, match="column list"):
        S.rec_eval_table(qs, gts, none_id=10, col_ids=[5, 6, 7, 8, 10])         # colour 9 is missing
    with pytest.raises(ValueError, match="column list"):
        S.rec_eval_table(qs, gts, none_id=10, col_ids=[5, 6, 7, 8, 9])          # "none" is missing


@pytest.mark.parametrize("bad", [[4, 4, 4, 9], [4, 4, 9, 4], [9, 4, 4, 9], [4, 9, 9, 4], [4, 4, float("nan"), 9]])
def test_table_refuses_a_degenerate_rectangle(bad):
    qs, gts = _hand_queries()
    qs[2]["rects"][1][0] = bad                                                 # not the rectangle any score would choose: any candidate counts
    with pytest.raises(ValueError, match="degenerate"):
        S.rec_eval_table(qs, gts, none_id=10)


def test_table_refuses_a_colour_rectangle_count_mismatch():
    qs, gts = _hand_queries()
    qs[0]["rects"][0] = qs[0]["rects"][0][:2]
    with pytest.raises(ValueError, match="3 colours and 2 rectangles"):
        S.rec_eval_table(qs, gts, none_id=10)
    qs, gts = _hand_queries()
    qs[0]["rects"] = qs[0]["rects"][:1]
    with pytest.raises(ValueError, match="2 colour sets and 1 rectangle sets"):
        S.rec_eval_table(qs, gts, none_id=10)
    qs, gts = _hand_queries()
    with pytest.raises(ValueError, match="annotation"):
        S.rec_eval_table(qs, [gts[0], None, [1, 2, float("inf"), 4]], none_id=10)


@pytest.mark.parametrize("mode", ["zsl", "fsl"])
def test_reference_reproduces_the_reference_val_fixture(golden_dir, mode):
    g, qs, gts = RE.fixture(golden_dir)
    t = S.rec_eval_table(qs, gts, int(g["none_id"]))
    ref = S.rec_eval_reference(torch.from_numpy(g["scores"]), t, few_shot=mode == "fsl")
    assert ref["idx"].tolist() == g[mode + "_max_idx"].tolist()
    assert ref["rects"] == g[mode + "_rect"].tolist()
    assert np.array_equal(RE.bits(ref["iou"]), RE.bits(g[mode + "_iou"])), (ref["iou"], g[mode + "_iou"])
    assert ref["correct"].tolist() == g[mode + "_correct"].astype(np.uint8).tolist()
    assert ref["accuracy"] == float(g[mode + "_percent"])
    assert ref["counts"] == [int(g[mode + "_correct"].sum()), len(qs)]
    # the planted cases are in the fixture: a fused w1 * h1 + w2 * h2 would give other bits for query 0; 0.5 exactly is not correct; touching
    # boxes do not intersect; the two val()s disagree on the query with the negative "none" logit
    assert all(ref["iou"][0] != x for x in g["fused_iou_q0"].tolist())
    assert ref["iou"][1] == 0.5 and not ref["correct"][1] and ref["iou"][2] == 0.0
    assert g["zsl_max_idx"][4] != g["fsl_max_idx"][4]


@pytest.mark.parametrize("few_shot", [False, True])
def test_reference_agrees_with_select_region_and_accuracy(golden_dir, few_shot):
    g, qs, gts = RE.fixture(golden_dir)
    qs = qs + [RE.query([5, 5, 2]), RE.query([1]), RE.query([3, 4])]
    gts = gts + [[10, 4, 30, 40], [0, 0, 21, 31], [9, 2, 25.5, 33.25]]
    t = S.rec_eval_table(qs, gts, RE.NONE_ID)
    scores = torch.cat([torch.from_numpy(g["scores"]), RE.grid_scores(int(t["seq_first"][-1]) - g["scores"].shape[0], 7)], 0)
    ref = S.rec_eval_reference(scores, t, few_shot)
    sf, cf = t["seq_first"].tolist(), t["cand_first"].tolist()
    preds = {}
    for q, item in enumerate(qs):
        idx, rect, sc = S.select_region(scores[sf[q]:sf[q + 1]], item["colors"], item["rects"], RE.NONE_ID, few_shot=few_shot)
        assert (idx, [float(x) for x in rect]) == (int(ref["idx"][q]), ref["rects"][q])
        assert np.array_equal(RE.bits(sc.numpy()), RE.bits(ref["cand_score"][cf[q]:cf[q + 1]]))
        assert RE.bits(sc[idx].numpy().reshape(1))[0] == RE.bits(ref["score"][q:q + 1])[0]
        preds[q] = rect
    assert ref["accuracy"] == S.accuracy(preds, gts)
    assert ref["counts"][1] == len(qs) and ref["counts"][0] == int(ref["correct"].sum())


def test_reference_leaves_out_what_val_could_not_judge():
    qs, gts = _hand_queries()
    t = S.rec_eval_table(qs, gts, none_id=10)
    ref = S.rec_eval_reference(RE.grid_scores(4, 3), t)
    assert ref["idx"][1] == -1 and ref["rects"][1] is None and np.isnan(ref["iou"][1]) and ref["score"][1] == -np.inf
    assert ref["counts"][1] == 2 and ref["accuracy"] == ref["counts"][0] / 2 * 100
    t = S.rec_eval_table(qs, [gts[0], None, None], none_id=10)
    ref = S.rec_eval_reference(RE.grid_scores(4, 3), t)
    assert ref["idx"][2] >= 0 and ref["rects"][2] is not None and np.isnan(ref["iou"][2]) and ref["counts"][1] == 1


def test_device_entry_is_bound_and_has_no_cpu_fallback():
    from cpt_amd import _lib as L
    from cpt_amd import build
    build.build(verbose=False)
    lib = L.lib()
    p = 4096                                                                   # (never dereferenced: refused before any launch)
    args = [p, 1, 12, p, 1, 1, p, p, 1, p, p, p, p, 10, 0, p, p, p, p, None, p, None]
    assert lib.cpt_rec_choose(*([None] + args[1:])) == -6
    assert lib.cpt_rec_choose(*(args[:20] + [None, None])) == -6               # counts is not optional
    for at, v in ((1, 0), (2, 0), (4, 0), (5, 0), (8, 0), (13, 12), (13, -1)):
        a = list(args)
        a[at] = v
        assert lib.cpt_rec_choose(*a) == -1, at
    qs, gts = _hand_queries()
    t = S.rec_eval_table(qs, gts, none_id=10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.rec_choose_device(torch.zeros(2, 12), [0], t, False, {})
