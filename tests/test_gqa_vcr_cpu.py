"""CPU: the host side of the GQA-CPT and VCR Q->A drivers (scoring.gqa_string_ids / gqa_choose_reference / gqa_accuracy, drivers.gqa_label_grid /
gqa_accumulation / set_dropout, the VCR accuracy rule) against what the reference's own evaluate() functions produced
(tools/make_golden_gqa_vcr_eval.py), and the new entry points of the library with their error codes (no GPU: the checks come before any launch)."""
import os
import tempfile

import numpy as np
import pytest
import torch

from cpt_amd import scoring as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def tok():
    from transformers import BertTokenizer
    g = np.load(os.path.join(GOLDEN, "tiny_gqa_vcr_prompts.npz"))
    d = tempfile.mkdtemp()
    vf = os.path.join(d, "vocab.txt")
    with open(vf, "w") as f:
        f.write("\n".join(str(w) for w in g["vocab"]) + "\n")
    return BertTokenizer(vf, do_lower_case=True)


@pytest.fixture(scope="module")
def gqa():
    g = np.load(os.path.join(GOLDEN, "tiny_gqa_eval.npz"))
    return {k: g[k] for k in g.files}


def _igts(g):
    return [[int(x) for x in row if x >= 0] for row in g["igt"]]


def test_gqa_string_ids_carry_the_first_piece_quirk(tok, gqa):
    labels = [str(x) for x in gqa["labels"]]
    token_ids, label_sid, piece_sid = S.gqa_string_ids(labels, tok)
    ids, pieces = S.gqa_first_pieces(labels, tok)
    assert token_ids == ids == [tok.convert_tokens_to_ids(tok.tokenize(lb))[0] for lb in labels]
    assert label_sid == list(range(len(labels)))                     # distinct strings: one id each
    at = labels.index
    assert pieces[at("cats")] == "cat" and piece_sid[at("cats")] == label_sid[at("cat")]          # a first piece that is another whole label
    assert piece_sid[at("dogs")] == piece_sid[at("dog")] == label_sid[at("dog")]                   # two labels sharing a first piece
    assert token_ids[at("dogs")] == token_ids[at("dog")]                                            # (the column list has duplicates)
    assert pieces[at("holding cup")] == "holding" and piece_sid[at("holding cup")] == -2           # a first piece that is no label
    assert piece_sid[at("red")] == label_sid[at("red")]
    # a repeated label string shares its id
    _, sid2, piece2 = S.gqa_string_ids(labels + ["cat"], tok)
    assert sid2[-1] == sid2[at("cat")] and piece2[-1] == sid2[at("cat")]
    # the label-column logits the reference pickled are those columns of the rows, duplicates kept
    assert np.array_equal(gqa["rows"][:, token_ids], gqa["logits"], equal_nan=True)


def test_gqa_choose_reference_and_accuracy_match_reference_evaluate(tok, gqa):
    labels = [str(x) for x in gqa["labels"]]
    _, answer_labels = S.gqa_first_pieces(labels, tok)
    res = S.gqa_choose_reference(torch.from_numpy(gqa["logits"]), labels, answer_labels, _igts(gqa), q_ids=gqa["q_ids"].tolist())
    assert [r["answer"] for r in res] == [str(a) for a in gqa["answer"]]
    assert [bool(r["correct"]) for r in res] == gqa["correct"].tolist()
    assert [r["question_id"] for r in res] == gqa["question_id"].tolist()
    assert S.gqa_accuracy(res, len(res)) == float(gqa["acc"])
    # the repeated question_id: its last entry decides, the divisor stays the number of questions
    qid = gqa["q_ids"].tolist()
    rep = [i for i, q in enumerate(qid) if qid.count(q) > 1]
    assert len(rep) == 2 and res[rep[0]]["correct"] != res[rep[1]]["correct"]
    assert S.gqa_accuracy(res, len(res)) == (sum(r["correct"] for r in res) - res[rep[0]]["correct"]) / len(res)
    # string ids say the same as the strings
    _, label_sid, piece_sid = S.gqa_string_ids(labels, tok)
    gt = S.gqa_gt_table(_igts(gqa), label_sid)
    pred = torch.from_numpy(gqa["logits"]).argmax(1)
    by_id = [bool(((gt[i] >= 0) & (gt[i] == piece_sid[int(pred[i])])).any()) for i in range(len(res))]
    assert by_id == gqa["correct"].tolist()
    assert gt.shape == (len(res), 3) and int((gt[0] >= 0).sum()) == 1 and int((gt[2] >= 0).sum()) == 3


def test_gqa_label_grid_and_accumulation():
    from cpt_amd import drivers
    ids = torch.tensor([[101, 7, 103, 102, 0], [101, 103, 9, 9, 102]])
    msk = torch.ones(2, 8, dtype=torch.long)
    tokens = torch.tensor([150, 200, 201])
    grid = drivers.gqa_label_grid(ids, msk, torch.tensor([[2], [0]]), tokens)
    want = torch.full((2, 8), -1, dtype=torch.long)
    want[0, 2], want[1, 1] = 201, 150
    assert torch.equal(grid, want)
    with pytest.raises(RuntimeError):          # two [MASK] slots in one sequence: the reference's index assignment fails too
        drivers.gqa_label_grid(torch.tensor([[101, 103, 103, 102, 0], [101, 103, 9, 9, 102]]), msk, torch.tensor([2, 0]), tokens)
    # gqa_cpt.py:328-334
    assert drivers.gqa_accumulation(1000, 4, 8, 250, num_train_epochs=5) == (31, 40)
    assert drivers.gqa_accumulation(3, 4, 8, 1, num_train_epochs=5) == (1, 5)
    assert drivers.gqa_accumulation(1000, 4, 8, 250, num_train_epochs=5, max_steps=17) == (31, 17)


def test_set_dropout_reaches_the_training_step():
    from cpt_amd import config as cfgmod, drivers, train as T
    from cpt_amd.modeling_rec import REC_MLM_CPT
    m = REC_MLM_CPT(cfgmod.tiny()).train()
    drivers.set_dropout(m, 0.3)
    assert m.config.hidden_dropout_prob == 0.3
    assert all(d.p == 0.3 for d in (getattr(m, "dropout", None), getattr(m.bert, "dropout", None), getattr(m.bert.embeddings, "dropout", None))
               if d is not None)
    st = T._TrainState(None)
    st.drop_seed = 1
    assert abs(T.dropout_for(m, st).p_hidden - 0.3) < 1e-7
    drivers.set_dropout(m, 0.0)
    m.config.attention_probs_dropout_prob = 0.0
    assert T.dropout_for(m, st) is None


def test_vcr_accuracy_rule_matches_reference_evaluate():
    g = np.load(os.path.join(GOLDEN, "tiny_vcr_nsp_eval.npz"))
    interval = int(g["interval"])
    rel = torch.from_numpy(g["rel"])
    scores, preds = S.nsp_choose(rel, interval)
    assert preds == g["answer"].tolist()
    assert np.allclose(scores.view(-1, interval).numpy(), g["choice_logits"], atol=1e-6)
    flags = [p == int(lb) for p, lb in zip(preds, g["labels"])]
    assert flags == g["correct"].tolist()
    res = [{"questionId": int(q), "correct": c} for q, c in zip(g["q_ids"], flags)]
    assert S.nsp_accuracy(res, len(res)) == float(g["acc"])
    qid = g["q_ids"].tolist()
    assert len(set(qid)) == len(qid) - 1


def test_new_entry_points_and_their_error_codes():
    """cpt_gqa_choose / cpt_nsp_choose / cpt_grad_clip exist, are bound, and refuse null pointers (-6) and bad shapes (-1) before any launch."""
    from cpt_amd import build, _lib as L
    build.build(verbose=False)
    lib = L.lib()
    assert lib.cpt_version() == 8
    p = 4096          # any non-null value: the argument checks return before a pointer is used
    assert lib.cpt_gqa_choose(None, 1, 1, p, p, 1, p, p, None, None) == -6
    assert lib.cpt_gqa_choose(p, 1, 1, p, p, 1, None, p, None, None) == -6
    assert lib.cpt_gqa_choose(p, 0, 1, p, p, 1, p, p, None, None) == -1
    assert lib.cpt_gqa_choose(p, 1, 0, p, p, 1, p, p, None, None) == -1
    assert lib.cpt_gqa_choose(p, 1, 1, p, p, 0, p, p, None, None) == -1
    assert lib.cpt_nsp_choose(None, 8, 2, 4, p, p, p, p, None, None) == -6
    assert lib.cpt_nsp_choose(p, 8, 2, 4, None, p, p, p, None, None) == -6
    assert lib.cpt_nsp_choose(p, 8, 1, 4, p, p, p, p, None, None) == -1          # n_rel >= 2
    assert lib.cpt_nsp_choose(p, 8, 2, 0, p, p, p, p, None, None) == -1
    assert lib.cpt_nsp_choose(p, 9, 2, 4, p, p, p, p, None, None) == -1          # a remainder
    assert b"whole number" in lib.cpt_last_error()
    ws = lib.cpt_grad_clip_workspace_bytes()
    assert ws >= 256 + 4
    assert lib.cpt_grad_clip(None, 8, 1.0, None, p, p, ws, None) == -6
    assert lib.cpt_grad_clip(p, 8, 1.0, None, None, p, ws, None) == -6
    assert lib.cpt_grad_clip(p, 8, 1.0, None, p, None, ws, None) == -6
    assert lib.cpt_grad_clip(p, 0, 1.0, None, p, p, ws, None) == -1
    assert lib.cpt_grad_clip(p, 8, 1.0, None, p, p, ws - 1, None) == -5
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.gqa_choose_device(torch.zeros(2, 3), [0, 1, 2], [[0], [1]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.nsp_choose_device(torch.zeros(8, 2), 4, [0, 1])
