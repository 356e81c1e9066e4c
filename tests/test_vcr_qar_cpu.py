"""CPU: VCR Q->AR (fewshot/vcr_qar_nsp_cpt.py) -- the prompt blocks (prompts.assemble_vcr_qar), the class-0 labels, the host restatement of
evaluate()'s choice and its accuracy rule, VCRQAR_NSPCPT's state dict and the new C entry points."""
import math
import os

import numpy as np
import pytest
import torch

from cpt_amd import config as cfgmod
from cpt_amd import prompts
from cpt_amd import scoring as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COLORS, NAMES = {"0": "red", "1_2": "blue"}, {"0": "person", "1_2": "dog and cat", "3": "table", "1": "dog"}
QUESTION = ["why", "is", [0], "looking", "at", [2, 1], "?"]
ANSWERS = [["because", [0], "wants", "the", "frisbee", "."], [[3], "is", "next", "to", [1], "."], ["she", "is", "holding", "a", "cup", "."],
           ["he", "is", "sitting", "."]]
RATIONALES = [["she", "wants", "it", "."], [[1], "is", "on", "the", "table", "."], ["no", "."], ["yes", "because", [0], "is", "holding", "it"]]


@pytest.fixture(scope="module")
def tok(tmp_path_factory):
    from transformers import BertTokenizer
    g = np.load(os.path.join(GOLDEN, "tiny_gqa_vcr_prompts.npz"))
    vf = tmp_path_factory.mktemp("vocab") / "vocab.txt"
    vf.write_text("\n".join(str(w) for w in g["vocab"]) + "\n")
    return BertTokenizer(str(vf), do_lower_case=True)


@pytest.mark.parametrize("n_rats", [4, 16])
def test_assemble_vcr_qar_blocks(tok, n_rats):
    rats = (RATIONALES * 4)[:n_rats]
    q = prompts.assemble_vcr_qar(tok, QUESTION, ANSWERS, rats, COLORS, NAMES, 5, label=(2, 1), q_id=7)
    assert (q["n_ans"], q["n_rats"], q["label"], q["q_id"]) == (4, n_rats, (2, 1), 7)
    # Q->A: exactly assemble_vcr
    qa = prompts.assemble_vcr(tok, QUESTION, ANSWERS, COLORS, NAMES, 5, label=2, q_id=7)
    for k in ("input_ids", "input_mask", "segment_ids"):
        assert np.array_equal(q["q_a"][k], qa[k])
    assert q["q_a"]["texts_b"] == qa["texts_b"] and q["q_a"]["text_a"] == qa["text_a"]
    # QA->R: text_a = question + the GROUND-TRUTH answer, written out (vcr_qar_nsp_cpt.py:180-186)
    r = q["qa_r"]
    assert r["text_a"] == prompts.vcr_textize(QUESTION + ANSWERS[2], COLORS, NAMES)
    assert r["text_a"] == "why is person in red looking at dog and cat in blue ? she is holding a cup ."
    assert r["texts_b"] == [prompts.vcr_textize(x, COLORS, NAMES, colorful=True) for x in rats]
    assert r["input_ids"].shape == (n_rats, 165) and r["input_mask"].shape == (n_rats, 210) and r["segment_ids"].shape == (n_rats, 165)
    ids, msk, seg, _ = prompts.tokenize_pair(tok, r["text_a"], r["texts_b"][1], 5, split_b_on_semicolons=True)
    assert np.array_equal(r["input_ids"][1], ids) and np.array_equal(r["input_mask"][1], msk) and np.array_equal(r["segment_ids"][1], seg)
    assert r["label"] == 1 and q["q_a"]["label"] == 2


def test_assemble_vcr_qar_needs_label(tok):
    with pytest.raises(ValueError):
        prompts.assemble_vcr_qar(tok, QUESTION, ANSWERS, RATIONALES, COLORS, NAMES, 5)
    with pytest.raises(ValueError):
        prompts.assemble_vcr_qar(tok, QUESTION, ANSWERS, RATIONALES, COLORS, NAMES, 5, label=(4, 0))


def test_qar_choice_labels():
    a, r = S.qar_choice_labels([2, 0], [1, 15], 4, 16)
    assert a.tolist() == [1, 1, 0, 1, 0, 1, 1, 1]
    want = [1] * 32
    want[1] = want[16 + 15] = 0
    assert r.tolist() == want and a.dtype == r.dtype == torch.int64


def test_choose_reference_rules():
    nan = float("nan")
    # question 0: tie -> first maximum; question 1: NaN counts as the maximum
    qa = torch.tensor([0.2, 0.9, 0.9, 0.1, 0.3, nan, 0.9, nan])
    qr = torch.tensor([0.5, 0.5, 0.1, 0.0, 0.0, 0.1, nan, 0.7])
    res = S.vcr_qar_choose_reference(qa, qr, [1, 2], [0, 2], 4, 4, q_ids=[10, 11])
    assert [x["answer"] for x in res] == [[1, 0], [1, 2]]
    assert [x["correct"] for x in res] == [True, False]
    assert [x["gt"] for x in res] == [[1, 0], [2, 2]]
    # 16 rationales: the slice [ans_label * n_ans, (ans_label + 1) * n_ans) with the GROUND-TRUTH answer, block width n_ans, as written
    qr16 = torch.zeros(16)
    qr16[4 * 3 + 2] = 1.0             # the maximum inside the slice of answer 3
    qr16[0] = 5.0                     # outside it: never chosen
    res = S.vcr_qar_choose_reference(torch.tensor([0.0, 0.0, 0.0, 1.0]), qr16, [3], [2], 4, 16)
    assert res[0]["answer"] == [3, 2] and res[0]["correct"] and len(res[0]["logits"][1]) == 4


def test_accuracy_dedup_last_wins():
    res = [{"questionId": 1, "correct": True}, {"questionId": 2, "correct": False}, {"questionId": 1, "correct": False},
           {"questionId": 3, "correct": True}]
    assert S.vcr_qar_accuracy(res, 4) == 0.25          # q1's last entry is wrong; divided by len(eval_dataset)
    assert math.isclose(S.vcr_qar_accuracy(res[:2], 2), 0.5)


def test_qar_accumulation_rule():
    from cpt_amd import drivers
    assert drivers.qar_accumulation(100, 1, 1, 100, num_train_epochs=5) == (100, 5)
    assert drivers.qar_accumulation(100, 1, 8, 13, num_train_epochs=2) == (12, 2)
    assert drivers.qar_accumulation(3, 4, 2, 1) == (1, 1)
    assert drivers.qar_accumulation(100, 1, 1, 100, max_steps=7) == (100, 7)


def test_state_dict_keys_and_param_specs():
    from cpt_amd import synth
    from cpt_amd.modeling_bert import BertImgForPreTraining
    from cpt_amd.modeling_vcr import VCRQAR_NSPCPT
    cfg = cfgmod.tiny()
    pre = BertImgForPreTraining(cfg)
    pre.load_state_dict(synth.init_state_dict(cfg, 1, head="pretrain"))
    m = VCRQAR_NSPCPT(cfg)
    assert m.cls_ans is None and m.cls_rat is None
    m.copy_from_pretraining_model(pre)
    keys = list(m.state_dict().keys())
    assert keys[-4:] == ["cls_ans.weight", "cls_ans.bias", "cls_rat.weight", "cls_rat.bias"]
    assert not any(k.startswith("cls.") for k in keys)
    assert keys == [n for n, _, kind in synth.param_specs(cfg, "qar") if kind != "tied"]
    # cls_ans IS the pre-training head; cls_rat an independent copy
    assert m.cls_ans is pre.cls.seq_relationship and m.cls_rat is not m.cls_ans
    assert torch.equal(m.cls_rat.weight, m.cls_ans.weight) and m.cls_rat.weight.data_ptr() != m.cls_ans.weight.data_ptr()
    from cpt_amd.engine import bucket_of
    assert bucket_of("cls_rat.weight", cfg.num_hidden_layers) == cfg.num_hidden_layers + 1
    with pytest.raises(RuntimeError):
        m.forward(torch.zeros(1, 4, dtype=torch.long), next_sentence_label=torch.zeros(1, dtype=torch.long), head="")


def test_new_entry_points_exported():
    from cpt_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.lib()
    for n in ("cpt_rel2_workspace_bytes", "cpt_rel2_scores", "cpt_train_fwd_rel2", "cpt_train_bwd_rel2", "cpt_train_zero_grads_rel2",
              "cpt_vcr_qar_choose"):
        assert hasattr(lib, n) and n in _lib._SIGS, n
    assert lib.cpt_rel2_workspace_bytes(0) == 0 and lib.cpt_rel2_workspace_bytes(8) >= 256 + 32


# ---- against the reference's own code (tools/make_golden_vcr_qar.py) ----------------------------------------------------------------------
def _gold(name):
    return np.load(os.path.join(GOLDEN, name))


@pytest.fixture(scope="module")
def gold_tok(tmp_path_factory):
    from transformers import BertTokenizer
    g = _gold("tiny_vcr_qar_prompts.npz")
    vf = tmp_path_factory.mktemp("vocab_qar") / "vocab.txt"
    vf.write_text("\n".join(str(w) for w in g["vocab"]) + "\n")
    return BertTokenizer(str(vf), do_lower_case=True)


@pytest.mark.parametrize("row", [0, 1])
def test_assemble_vcr_qar_matches_reference_tensorize(gold_tok, row):
    """VCRDataset.tensorize_example of vcr_qar_nsp_cpt.py (4 rationales on row 0, 16 on row 1): ids, masks, segments, the QA->R text_a built from
    the ground-truth answer, the rationale texts and each block's label."""
    import json
    g = _gold("tiny_vcr_qar_prompts.npz")
    a = json.loads(str(g["args"]))
    k = "row%d_" % row
    inp = json.loads(str(g[k + "in"]))
    q = prompts.assemble_vcr_qar(gold_tok, inp["question"], inp["answers"], inp["rationales"], inp["colors"], inp["names"], inp["n_regions"],
                                 label=tuple(inp["label"]), q_id=inp["q_id"], max_seq_length=a["max_seq_length"],
                                 max_img_seq_length=a["max_img_seq_length"])
    assert q["n_rats"] == len(inp["rationales"]) == (4, 16)[row]
    for part in ("q_a", "qa_r"):
        for key, name in (("input_ids", "ids"), ("input_mask", "mask"), ("segment_ids", "seg")):
            assert np.array_equal(q[part][key], g[k + part + "_" + name]), (part, key)
        assert (g[k + part + "_qid"] == inp["q_id"]).all()
        assert (g[k + part + "_label"] == q[part]["label"]).all()
    assert q["qa_r"]["text_a"] == str(g[k + "qa_r_text_a"])
    assert q["qa_r"]["texts_b"] == [str(x) for x in g[k + "qa_r_texts_b"]]


def test_choice_labels_match_reference_driver():
    g = _gold("tiny_vcr_qar_model.npz")
    a, r = S.qar_choice_labels(g["ans"].tolist(), g["rat"].tolist(), 4, 4)
    assert np.array_equal(a.numpy(), g["q_a_cls"]) and np.array_equal(r.numpy(), g["qa_r_cls"])


@pytest.mark.parametrize("layout", ["r4", "r16"])
def test_choose_and_accuracy_match_reference_evaluate(layout):
    """The reference evaluate() on fixed relation scores (planted ties, a repeated questionId): its pickled answer / correct / gt and its acc."""
    g = _gold("tiny_vcr_qar_eval.npz")
    k = layout + "_"
    n_rats = int(g[k + "n_rats"])
    qa = S.choice_scores(torch.from_numpy(g[k + "q_a_rel"]))
    qr = S.choice_scores(torch.from_numpy(g[k + "qa_r_rel"]))
    res = S.vcr_qar_choose_reference(qa, qr, g[k + "ans"].tolist(), g[k + "rat"].tolist(), 4, n_rats, q_ids=g[k + "q_ids"].tolist())
    assert [x["answer"] for x in res] == g[k + "answer"].tolist()
    assert [x["correct"] for x in res] == g[k + "correct"].tolist()
    assert [x["gt"] for x in res] == g[k + "gt"].tolist()
    assert [x["questionId"] for x in res] == g[k + "questionId"].tolist()
    assert S.vcr_qar_accuracy(res, len(res)) == float(g[k + "acc"])


def test_state_dict_keys_match_reference_model():
    from cpt_amd import synth
    from cpt_amd.modeling_bert import BertImgForPreTraining
    from cpt_amd.modeling_vcr import VCRQAR_NSPCPT
    cfg = cfgmod.tiny()
    pre = BertImgForPreTraining(cfg)
    pre.load_state_dict(synth.init_state_dict(cfg, 4321, head="pretrain"))
    m = VCRQAR_NSPCPT(cfg)
    m.copy_from_pretraining_model(pre)
    assert list(m.state_dict().keys()) == [str(k) for k in _gold("tiny_vcr_qar_model.npz")["keys"]]
