"""Golden vectors of VCR Q->AR from the reference's own code (Oscar/oscar/fewshot/vcr_qar_nsp_cpt.py, modeling/modeling_vcr.py:194-251).

Runs on a CPU box with the reference checked out (default /root/reference, or $CPT_REFERENCE), importing its modules through
oracle/ref_stub.py as oracle/make_golden_gqa_vcr.py does; nothing of the reference is copied.  Three fixtures:
  1. tiny_vcr_qar_prompts.npz -- VCRDataset.tensorize_example of the Q->AR driver on two hand-written rows, one with 4 rationales and one
     with 16; the dataset object is built with object.__new__ (its __init__ wants the VCR annotation trees on disk).
  2. tiny_vcr_qar_model.npz -- the reference VCRQAR_NSPCPT on config.tiny(), weights synth.init_state_dict(..., head="pretrain") through
     copy_from_pretraining_model, cls_rat then moved by a seeded offset (stored) so that a swapped head cannot pass: both heads' scores on
     2 questions x (4 + 4) sequences, q_a_loss + qa_r_loss with the driver's labels, and the autograd gradients of cls_ans.*, cls_rat.*, the
     pooler and the layer-0 query (eval mode: no dropout).
  3. tiny_vcr_qar_eval.npz -- the reference evaluate() itself, with a stand-in model that returns fixed seeded relation scores (planted ties,
     a repeated questionId) and a list-based dataset in vcr_collate_fn form, for the 4- and the 16-rationale layouts: what it pickles
     (answer, correct, gt) and its acc.

    python tools/make_golden_vcr_qar.py     # rewrites the three files identically
"""
import json
import logging
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("CPT_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
OUT = os.path.join(ROOT, "tests", "golden")

import ref_stub  # noqa: E402

pkg = ref_stub.install()
from transformers import BertTokenizer  # noqa: E402

pkg.WEIGHTS_NAME = "pytorch_model.bin"
pkg.BertTokenizer = BertTokenizer
for _n in ("AdamW", "WarmupLinearSchedule", "WarmupConstantSchedule"):
    setattr(pkg, _n, type(_n, (), {}))
sys.modules.setdefault("tqdm", types.SimpleNamespace(tqdm=lambda it, **kw: it))
sys.path.insert(0, os.path.join(REF, "Oscar"))
import oscar.fewshot.vcr_qar_nsp_cpt as V  # noqa: E402
from oscar.modeling.modeling_bert import BertImgForPreTraining  # noqa: E402
from oscar.modeling.modeling_vcr import VCRQAR_NSPCPT  # noqa: E402
from oscar.utils.task_utils import InputInstance  # noqa: E402
from oscar.utils.tsv_file import TSVFile  # noqa: E402

from cpt_amd import config as cfgmod  # noqa: E402
from cpt_amd import synth  # noqa: E402

# the vocabulary of tests/golden/tiny_gqa_vcr_prompts.npz (the CPU tests build their tokenizer from it)
VOCAB = [str(w) for w in np.load(os.path.join(OUT, "tiny_gqa_vcr_prompts.npz"))["vocab"]]
COLORS, NAMES = {"0": "red", "1_2": "blue"}, {"0": "person", "1_2": "dog and cat", "3": "table", "1": "dog", "2": "cat"}
QUESTION = ["why", "is", [0], "looking", "at", [2, 1], "?"]
ANSWERS = [["because", [0], "wants", "the", "frisbee", "."], [[3], "is", "next", "to", [1], "."], ["she", "is", "holding", "a", "cup", "."],
           ["he", "is", "sitting", "."]]
RATS4 = [["she", "wants", "it", "."], [[1], "is", "on", "the", "table", "."], ["no", "."], ["yes", "because", [0], "is", "holding", "it"]]
RATS16 = [RATS4[i % 4] + (["and", "the", "cup"] * (i // 4)) for i in range(16)]
ROWS = [("88", RATS4, (2, 1), 5), ("89", RATS16, (1, 13), 3)]
MAX_SEQ, MAX_IMG = 40, 6


def prompts_fixture(tmp, rng):
    import base64
    vf = os.path.join(tmp, "vocab.txt")
    with open(vf, "w") as f:
        f.write("\n".join(VOCAB) + "\n")
    tok = BertTokenizer(vf, do_lower_case=True)
    args = types.SimpleNamespace(max_seq_length=MAX_SEQ, max_img_seq_length=MAX_IMG, output_mode="classification", model_type="bert", load_fast=False,
                                 img_feature_type="faster_r-cnn")
    g = {"vocab": np.array(VOCAB), "args": np.array(json.dumps({"max_seq_length": MAX_SEQ, "max_img_seq_length": MAX_IMG}))}
    for i, (key, rats, label, nbox) in enumerate(ROWS):
        bl = [{"rect": [float(v) for v in rng.integers(0, 200, 4)], "class": ["dog", "cat", "person", "table"][j % 4], "conf": 0.5,
               "feature": base64.b64encode(rng.standard_normal(2054).astype(np.float32).tobytes()).decode("utf-8")} for j in range(nbox)]
        tsv = os.path.join(tmp, "rows%d.tsv" % i)
        with open(tsv, "w") as f:
            f.write(key + "_0\t" + json.dumps({"objects": [bl, [COLORS, NAMES]]}) + "\n")
        ex = InputInstance(guid=key, text_a=QUESTION, text_b=[ANSWERS, rats], label=label, img_key=key + "_0", q_id=int(key))
        ds = object.__new__(V.VCRDataset)
        ds.args, ds.tokenizer = args, tok
        ds.feat_tsv = TSVFile(tsv, generate_lineidx=True)
        ds.imgid2feat = {key + "_0": 0}
        q_a, qa_r = ds.tensorize_example(ex, cls_token=tok.cls_token, sep_token=tok.sep_token, cls_token_segment_id=0, pad_token_segment_id=0)
        k = "row%d_" % i
        g[k + "in"] = np.array(json.dumps({"question": QUESTION, "answers": ANSWERS, "rationales": rats, "colors": COLORS, "names": NAMES,
                                           "n_regions": nbox, "label": list(label), "q_id": int(key)}))
        for part, out in (("q_a", q_a), ("qa_r", qa_r)):
            g[k + part + "_ids"] = np.stack([o[0].numpy() for o in out])
            g[k + part + "_mask"] = np.stack([o[1].numpy() for o in out])
            g[k + part + "_seg"] = np.stack([o[2].numpy() for o in out])
            g[k + part + "_qid"] = np.array([o[4] for o in out])
            g[k + part + "_label"] = np.array([o[5] for o in out])
        g[k + "qa_r_text_a"] = np.array(ds._vcr_textize(QUESTION + ANSWERS[label[0]], COLORS, NAMES))
        g[k + "qa_r_texts_b"] = np.array([ds._vcr_textize(c, COLORS, NAMES, colorful=True) for c in rats])
    g["n_rows"] = np.array(len(ROWS))
    np.savez_compressed(os.path.join(OUT, "tiny_vcr_qar_prompts.npz"), **g)


def model_fixture():
    cfg = cfgmod.tiny()
    rc = ref_stub.BertConfig(**cfg.to_dict())
    pre = BertImgForPreTraining(rc)
    pre.load_state_dict(synth.init_state_dict(cfg, 4321, head="pretrain"), strict=True)
    pre.tie_weights()
    m = VCRQAR_NSPCPT(rc)
    m.copy_from_pretraining_model(pre)
    gen = torch.Generator().manual_seed(4322)
    with torch.no_grad():        # cls_rat off cls_ans: a swapped head must not pass
        m.cls_rat.weight.add_(torch.randn(m.cls_rat.weight.shape, generator=gen) * 0.05)
        m.cls_rat.bias.add_(torch.randn(m.cls_rat.bias.shape, generator=gen) * 0.05)
    m.eval()
    n_ans = n_rats = 4
    ans, rat = [2, 0], [1, 3]
    b = synth.make_batch(16, cfg, seed=23, max_seq_len=20, img_seq_len=6, n_regions=6, vary_regions=True)
    qa = {k: v[:8] for k, v in b.items()}
    qr = {k: v[8:] for k, v in b.items()}
    # the driver's labels (vcr_qar_nsp_cpt.py:462-472)
    q_a_cls = torch.ones([8], dtype=torch.long)
    for i, lb in enumerate(ans):
        q_a_cls[i * n_ans + lb] = 0
    qa_r_cls = torch.ones([8], dtype=torch.long)
    for i, lb in enumerate(rat):
        qa_r_cls[i * n_rats + lb] = 0
    q_a_loss, q_a_rel = m(qa["input_ids"], qa["segment_ids"], qa["attention_mask"], next_sentence_label=q_a_cls, img_feats=qa["img_feats"],
                          head="ans")[:2]
    qa_r_loss, qa_r_rel = m(qr["input_ids"], qr["segment_ids"], qr["attention_mask"], next_sentence_label=qa_r_cls, img_feats=qr["img_feats"],
                            head="rat")[:2]
    loss = q_a_loss + qa_r_loss
    m.zero_grad()
    loss.backward()
    g = {"in_" + k: v.numpy() for k, v in b.items()}
    g.update(q_a_rel=q_a_rel.detach().numpy(), qa_r_rel=qa_r_rel.detach().numpy(), loss=loss.detach().numpy(),
             q_a_loss=q_a_loss.detach().numpy(), qa_r_loss=qa_r_loss.detach().numpy(), q_a_cls=q_a_cls.numpy(), qa_r_cls=qa_r_cls.numpy(),
             ans=np.array(ans), rat=np.array(rat), cls_rat_weight=m.cls_rat.weight.detach().numpy(), cls_rat_bias=m.cls_rat.bias.detach().numpy(),
             grad_cls_ans_weight=m.cls_ans.weight.grad.numpy(), grad_cls_ans_bias=m.cls_ans.bias.grad.numpy(),
             grad_cls_rat_weight=m.cls_rat.weight.grad.numpy(), grad_cls_rat_bias=m.cls_rat.bias.grad.numpy(),
             grad_pooler_weight=m.bert.pooler.dense.weight.grad.numpy(),
             grad_q0_weight=m.bert.encoder.layer[0].attention.self.query.weight.grad.numpy(),
             keys=np.array(list(m.state_dict().keys())))
    np.savez_compressed(os.path.join(OUT, "tiny_vcr_qar_model.npz"), **g)


class _ListDataset(list):
    name = "val"


class _ScoreModel(object):
    """evaluate() is a function of the relation scores the model returns: hand it fixed ones, in call order."""

    def __init__(self, queue):
        self.queue = list(queue)

    def eval(self):
        return self

    def __call__(self, **kw):
        rel = self.queue.pop(0)
        assert rel.size(0) == kw["input_ids"].size(0) and kw["head"] in ("ans", "rat")
        return (rel,)


def eval_fixture(tmp, rng):
    g = {}
    for layout, n_rats in (("r4", 4), ("r16", 16)):
        n_ans, n_q, bs = 4, 7, 3
        q_ids = [500 + i for i in range(n_q)]
        q_ids[5] = q_ids[2]                          # a repeated questionId: the last entry wins, acc still divides by len(dataset)
        ans = [int(x) for x in rng.integers(0, n_ans, n_q)]
        rat = [int(x) for x in rng.integers(0, n_ans if n_rats > n_ans else n_rats, n_q)]
        rat[0] = 9 if n_rats > n_ans else rat[0]      # 16 rationales: a label outside the 4-wide slice is never right
        items = []
        for q in range(n_q):
            def seqs(n, lab):
                return [(torch.zeros(4, dtype=torch.long), torch.ones(6, dtype=torch.long), torch.zeros(4, dtype=torch.long), torch.zeros(2, 3),
                         q_ids[q], lab, []) for _ in range(n)]
            items.append((seqs(n_ans, ans[q]), seqs(n_rats, rat[q])))
        ds = _ListDataset(items)
        # relation scores in call order (batch by batch: q_a then qa_r), few distinct values so that choice scores tie
        queue, all_qa, all_qr = [], [], []
        for s in range(0, n_q, bs):
            nb = min(bs, n_q - s)
            for n, store in ((nb * n_ans, all_qa), (nb * n_rats, all_qr)):
                rel = torch.from_numpy(rng.integers(0, 3, (n, 2)).astype(np.float32) / 2)
                queue.append(rel)
                store.append(rel)
        args = types.SimpleNamespace(task_name="vcr_qar", output_dir=os.path.join(tmp, "out"), local_rank=-1, per_gpu_eval_batch_size=bs, n_gpu=1,
                                     workers=0, device=torch.device("cpu"), model_type="bert", img_feature_dim=3,
                                     result_dir=os.path.join(tmp, "res_" + layout))
        results, acc = V.evaluate(args, _ScoreModel(queue), ds)
        with open(os.path.join(args.result_dir, "val_results.pk"), "rb") as f:
            pk = pickle.load(f)
        k = layout + "_"
        g[k + "q_a_rel"] = torch.cat(all_qa).numpy()
        g[k + "qa_r_rel"] = torch.cat(all_qr).numpy()
        g[k + "ans"], g[k + "rat"], g[k + "q_ids"] = np.array(ans), np.array(rat), np.array(q_ids)
        g[k + "n_rats"], g[k + "batch"] = np.array(n_rats), np.array(bs)
        g[k + "answer"] = np.array([r["answer"] for r in pk])
        g[k + "correct"] = np.array([r["correct"] for r in pk])
        g[k + "gt"] = np.array([[int(x) for x in r["gt"]] for r in pk])
        g[k + "questionId"] = np.array([int(r["questionId"]) for r in pk])
        g[k + "acc"] = np.array(acc)
    np.savez_compressed(os.path.join(OUT, "tiny_vcr_qar_eval.npz"), **g)


def main():
    logging.disable(logging.INFO)
    torch.manual_seed(0)
    rng = np.random.Generator(np.random.PCG64(707))
    tmp = tempfile.mkdtemp()
    prompts_fixture(tmp, rng)
    model_fixture()
    eval_fixture(tmp, rng)
    for n in ("tiny_vcr_qar_prompts.npz", "tiny_vcr_qar_model.npz", "tiny_vcr_qar_eval.npz"):
        print("wrote", os.path.join(OUT, n), os.path.getsize(os.path.join(OUT, n)), "bytes")


if __name__ == "__main__":
    main()
