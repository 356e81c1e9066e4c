"""Shared by the REC evaluation tests: the tiny_rec_eval fixture as queries, hand-built queries on planted scores, and the comparison of a device
pass with scoring.rec_eval_reference -- everything for equality, floats by their bits."""
import os

import numpy as np
import torch

from cpt_amd import scoring as S

COLOURS = [5, 6, 7, 8, 9]
NONE_ID = 10
V = 12


def fixture(golden_dir):
    """(fixture arrays, queries, gts): the queries carry ``colors`` and ``rects`` only -- all the table builder reads."""
    g = np.load(os.path.join(golden_dir, "tiny_rec_eval.npz"))
    queries, s = [], 0
    first = g["rect_first"].tolist()
    for q, n in enumerate(g["n_seq"].tolist()):
        colors = [[int(c) for c in row if c >= 0] for row in g["colors"][s:s + n]]
        flat = g["rects"][first[q]:first[q + 1]].tolist()
        rects, at = [], 0
        for c in colors:
            rects.append(flat[at:at + len(c)])
            at += len(c)
        queries.append({"colors": colors, "rects": rects})
        s += n
    return g, queries, [row.tolist() for row in g["gt"]]


def query(colour_counts, rects=None):
    """A query of len(colour_counts) sequences; sequence j holds colour_counts[j] colours (cycling through COLOURS) and as many distinct boxes."""
    colors = [[COLOURS[k % 5] for k in range(n)] for n in colour_counts]
    if rects is None:
        rects = [[[7 * j + k, 3 * k + j, 7 * j + k + 20 + k, 3 * k + j + 30 + j] for k in range(n)] for j, n in enumerate(colour_counts)]
    return {"colors": colors, "rects": rects}


def grid_scores(n_seq, seed, width=V):
    """(n_seq, width) fp32 on a coarse grid (exact ties are common), "none" logits positive."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = torch.from_numpy((rng.integers(-8, 9, (n_seq, width)) / 4.0).astype(np.float32))
    rows[:, NONE_ID] = torch.from_numpy(rng.choice([0.5, 1.25, 2.0, 3.0], n_seq).astype(np.float32))
    return rows


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def assert_same(got, ref, what=""):
    """got: rec_eval_buffers after a pass (device tensors) or host arrays under the same names; ref: rec_eval_reference's dict."""
    host = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in got.items() if v is not None}
    assert host["idx"].tolist() == ref["idx"].tolist(), (what, host["idx"], ref["idx"])
    assert np.array_equal(bits(host["score"]), bits(ref["score"])), (what, host["score"], ref["score"])
    assert np.array_equal(bits(host["iou"]), bits(ref["iou"])), (what, host["iou"], ref["iou"])
    assert host["correct"].tolist() == ref["correct"].tolist(), (what, host["correct"], ref["correct"])
    if "counts" in host:
        assert host["counts"].tolist() == ref["counts"], (what, host["counts"], ref["counts"])
    if "cand_score" in host:
        assert np.array_equal(bits(host["cand_score"]), bits(ref["cand_score"])), (what, host["cand_score"], ref["cand_score"])


def run_device(scores, table, few_shot, dev, q_index=None, candidate_scores=True, out=None):
    """One cpt_rec_choose launch over the queries q_index (all, in order, by default) on their rows of ``scores`` (table order)."""
    sf = table["seq_first"].tolist()
    q_index = list(range(table["n_queries"])) if q_index is None else list(q_index)
    rows = torch.cat([scores[sf[q]:sf[q + 1]] for q in q_index], 0)
    out = S.rec_eval_buffers(table, dev, candidate_scores) if out is None else out
    return S.rec_choose_device(rows.to(dev), q_index, table, few_shot, out)
