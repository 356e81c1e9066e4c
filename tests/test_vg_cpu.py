"""VG-CPT predicate scoring, host side: the candidate / template tables the device scoring reads, the torch restatement of
val()'s loop (Oscar/oscar/fewshot/vg_cpt.py:271-290) and the new entry points of the C ABI binding."""
import os
import re

import pytest
import torch

from cpt_amd import scoring as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_candidates_table():
    idx2pred = {1: [5], 2: [7, 8], 3: [9, 10, 11], 4: [5, 7], 6: [11]}
    cols, cc, cl = S.vg_candidates(idx2pred)
    assert cols.tolist() == [5, 7, 8, 9, 10, 11]
    assert cl.tolist() == [0, 1, 2, 3, 2, 0, 1]             # 0: background, 5: no predicate
    for idx, pieces in idx2pred.items():
        assert [cols[int(cc[idx, j])].item() for j in range(len(pieces))] == pieces


def test_candidates_reject_four_pieces():
    with pytest.raises(ValueError, match="4 word-pieces"):
        S.vg_candidates({1: [1, 2, 3, 4]})


def test_slot_rows_follow_the_dataset_layout():
    # pair i: sequences 6i + 3d + k - 1 carry k head rows, rows numbered in sequence order
    n_pairs = 3
    first, r = {}, 0
    for s in range(6 * n_pairs):
        first[s] = r
        r += s % 3 + 1
    want = torch.tensor([[first[6 * (g // 2) + 3 * (g % 2) + k] for k in range(3)] for g in range(2 * n_pairs)], dtype=torch.int32)
    assert torch.equal(S.vg_slot_rows(n_pairs), want)


def test_slot_rows_from_actual_rows():
    seq = torch.tensor([s for s in range(12) for _ in range(s % 3 + 1)])
    assert torch.equal(S.vg_slot_rows_from(seq, 12), S.vg_slot_rows(2))
    bad = seq.clone()
    bad[1] = 0                                       # sequence 0 with 2 rows, sequence 1 with 1
    with pytest.raises(ValueError, match="sequence 0 holds 2"):
        S.vg_slot_rows_from(bad, 12)
    with pytest.raises(ValueError, match="ascending"):
        S.vg_slot_rows_from(seq.flip(0), 12)
    with pytest.raises(ValueError, match="6 sequences"):
        S.vg_slot_rows_from(seq[:10], 10)


def test_val_restatement_against_log_softmax():
    """The restated loop equals mean log_softmax of the pieces at the k-mask template's rows; background slot 0."""
    g = torch.Generator().manual_seed(0)
    V = 50
    idx2pred = {1: [3], 2: [4, 9], 3: [10, 11, 12], 4: [3, 3]}
    seqs = [torch.randn(s % 3 + 1, V, generator=g) * 3 for s in range(12)]
    got = S.vg_val_scores_reference(seqs, idx2pred)
    assert got.shape == (2, 2, 5)
    for i in range(2):
        for d in range(2):
            assert got[i, d, 0] == 0
            for idx, pieces in idx2pred.items():
                rows = seqs[6 * i + 3 * d + len(pieces) - 1].log_softmax(-1)
                want = torch.stack([rows[j, t] for j, t in enumerate(pieces)]).mean()
                assert abs(got[i, d, idx] - want) <= 1e-5


def test_rows_entry_points_declared_and_bound():
    from cpt_amd import _lib
    src = open(os.path.join(ROOT, "include", "cpt_hip.h")).read()
    for name in ("cpt_fwd_rows_workspace_bytes", "cpt_model_fwd_rows", "cpt_mean_logprob_scores"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.exported_symbols(), name


def _golden_vg():
    import numpy as np
    g = np.load(os.path.join(ROOT, "tests", "golden", "tiny_vg_val.npz"))
    idx2pred = {i: [int(t) for t in row if t >= 0] for i, row in enumerate(g["pred_pieces"]) if (row >= 0).any()}
    return g, idx2pred


def test_val_restatement_matches_reference_val_pt():
    """The torch restatement against the prediction dict the reference's val() saved (tools/make_golden_vg.py)."""
    g, idx2pred = _golden_vg()
    rows = torch.from_numpy(g["row_logits"])
    seq = torch.from_numpy(g["row_seq"])
    seq_rows = [rows[seq == s] for s in range(int(seq.max()) + 1)]
    got = S.vg_val_scores_reference(seq_rows, idx2pred)
    want = torch.from_numpy(g["val_scores"])
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-5


def test_tables_follow_reference_rows():
    """The candidate table and the slot rows taken from the reference batch's own row list give val()'s scores on the host."""
    g, idx2pred = _golden_vg()
    cols, cc, cl = S.vg_candidates(idx2pred)
    rows = torch.from_numpy(g["row_logits"]).double()
    lse = torch.logsumexp(rows, -1)
    slot = S.vg_slot_rows_from(torch.from_numpy(g["row_seq"]), int(g["row_seq"].max()) + 1)
    lp = rows[:, cols] - lse[:, None]
    got = torch.zeros(slot.size(0), cl.numel(), dtype=torch.float64)
    for gi in range(slot.size(0)):
        for c in range(cl.numel()):
            n = int(cl[c])
            if n:
                s = int(slot[gi, n - 1])
                got[gi, c] = sum(lp[s + j, int(cc[c, j])] for j in range(n)) / n
    want = torch.from_numpy(g["val_scores"]).double().reshape(got.shape)
    assert (got - want).abs().max().item() <= 1e-5
