"""Golden vectors of the GQA-CPT and VCR Q->A driver loops from the reference's own code (Oscar/oscar/fewshot/gqa_cpt.py, vcr_nsp_cpt.py).

Runs on a CPU box with the reference checked out (default /root/reference, or $CPT_REFERENCE), importing its modules through oracle/ref_stub.py
as tools/make_golden_vcr_qar.py does; nothing of the reference is copied.  Three fixtures, data only:
  1. tiny_gqa_eval.npz -- the reference gqa_cpt.evaluate() itself with a stand-in model that returns fixed seeded scores and the tiny vocabulary
     of tiny_gqa_vcr_prompts.npz.  The label list holds two labels sharing a first word-piece, multi-piece labels whose first piece is another
     whole label (one placed BEFORE that label), and one whose first piece is no label; questions have one or several ground truths, one
     question_id is repeated, the scores tie exactly in many places and one row holds a NaN.  Stored: labels, the (R, V) [MASK]-row scores, the
     (R, C) label-column logits the reference pickles, eval_dic, and per question answer / correct, plus acc.
  2. tiny_vcr_nsp_eval.npz -- the reference vcr_nsp_cpt.evaluate() with fixed relation scores drawn from a small pool of rows: two choice
     scores of a question are either exactly tied (identical rows) or at least 1e-3 apart (asserted), so no fp32 softmax difference can flip an
     argmax.  Stored: rel, labels, q_ids (one repeated), answer / correct per question, acc.
  3. tiny_gqa_vcr_train.npz -- 3 optimizer steps x 2 micro-steps, dropout 0, of the reference's own REC_MLM_CPT and NSPCPT on config.tiny()
     with the training-loop lines of gqa_cpt.py:423-462 / vcr_nsp_cpt.py:430-473 restated here (label construction, loss / accumulation steps,
     backward, torch.nn.utils.clip_grad_norm_ on every micro-step, scheduler before optimizer, zero_grad).  pytorch_transformers' AdamW and
     WarmupLinearSchedule are not under the reference tree: the oracle's restatements stand in (oracle/cpt_oracle.py adamw_step_hf,
     warmup_linear_schedule).  Stored: the loss of every micro-step, the gradient norm before every clip (max_grad_norm is chosen so that the
     coefficient is below 1 every time: asserted), and a fixed sample of parameters after every step.

    python tools/make_golden_gqa_vcr_eval.py     # rewrites the three files identically
"""
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
import oscar.fewshot.gqa_cpt as G  # noqa: E402
import oscar.fewshot.vcr_nsp_cpt as V  # noqa: E402
from oscar.modeling.modeling_bert import BertImgForPreTraining  # noqa: E402
from oscar.modeling.modeling_rec import REC_MLM_CPT  # noqa: E402
from oscar.modeling.modeling_vcr import NSPCPT  # noqa: E402

import cpt_oracle as O  # noqa: E402
from cpt_amd import config as cfgmod  # noqa: E402
from cpt_amd import synth  # noqa: E402

VOCAB = [str(w) for w in np.load(os.path.join(OUT, "tiny_gqa_vcr_prompts.npz"))["vocab"]]
# "cats" / "dogs" / "cups" split into <word> + "##s": first piece = another whole label ("cats" comes BEFORE "cat": a tie between their shared
# column goes to "cats", whose predicted string is "cat"); "dog" / "dogs" share a first piece; "holding cup" -> "holding", which is no label
GQA_LABELS = ["cats", "dog", "dogs", "holding cup", "cat", "cup", "red", "sitting", "table", "yes", "no", "cups"]


class _Args(types.SimpleNamespace):
    pass


def _args(tmp, name, bs):
    return _Args(task_name=name, output_dir=os.path.join(tmp, "out_" + name), local_rank=-1, per_gpu_eval_batch_size=bs, n_gpu=1, workers=0,
                 device=torch.device("cpu"), model_type="bert", img_feature_dim=3, result_dir=os.path.join(tmp, "res_" + name))


class _GQADataset(list):
    pass


class _RowModel(object):
    """gqa_cpt.evaluate() reads outputs[b, mask_pos[b], :]: hand it fixed rows there, in call order."""

    def __init__(self, rows, mask_pos, L):
        self.rows, self.mask_pos, self.L, self.at = rows, mask_pos, L, 0

    def eval(self):
        return self

    def __call__(self, **kw):
        B = kw["input_ids"].size(0)
        out = torch.zeros(B, self.L, self.rows.size(1))
        for b in range(B):
            out[b, self.mask_pos[self.at + b]] = self.rows[self.at + b]
        self.at += B
        return (out,)


def gqa_eval_fixture(tmp, rng):
    vf = os.path.join(tmp, "vocab.txt")
    with open(vf, "w") as f:
        f.write("\n".join(VOCAB) + "\n")
    tok = BertTokenizer(vf, do_lower_case=True)
    labels = GQA_LABELS
    Vn, L, n_q, bs = len(VOCAB), 8, 10, 4
    col = {w: tok.convert_tokens_to_ids([w])[0] for w in ("cat", "dog", "cup", "holding", "red", "yes")}
    rows = torch.from_numpy(rng.integers(0, 3, (n_q, Vn)).astype(np.float32) / 2)      # three distinct values: ties everywhere
    rows[1, col["cat"]] = 5.0                       # "cats" / "cat" share the column: the tie goes to "cats" (index 0), predicted string "cat"
    rows[2, col["dog"]] = 5.0                       # "dog" / "dogs"
    rows[3, col["holding"]] = 5.0                   # predicted string "holding": equal to no label, never right
    rows[4, col["cup"]] = float("nan")              # NaN counts as the maximum: "cup" (index 5) before "cups" (index 11)
    rows[5, col["red"]] = 5.0
    rows[5, col["yes"]] = 5.0                       # a planted exact tie between two labels: "red" (index 6) wins
    rows[8, col["red"]] = 5.0                       # (the second entry of the repeated question_id: wrong, where the first is right)
    q_ids = [700 + i for i in range(n_q)]
    q_ids[8] = q_ids[2]                             # a repeated question_id: the last entry wins, acc still divides by len(dataset)
    L_ = labels.index
    igt = {700: [L_("no")], 701: [L_("cat")], 702: [L_("table"), L_("dog"), L_("yes")], 703: [L_("holding cup")], 704: [L_("cups"), L_("cup")],
           705: [L_("yes")], 706: [L_("red"), L_("sitting")], 707: [L_("cats")], 709: [L_("dogs"), L_("no"), L_("cat")]}
    mask_pos = [int(x) for x in rng.integers(1, L, n_q)]
    ds = _GQADataset()
    for i in range(n_q):
        ds.append((torch.zeros(L, dtype=torch.long), torch.ones(L + 2, dtype=torch.long), torch.zeros(L, dtype=torch.long),
                   torch.tensor([igt[q_ids[i]][0]]), torch.zeros(len(labels)), torch.zeros(2, 3), torch.tensor([q_ids[i]]), [mask_pos[i]]))
    ds.labels = labels
    ds.eval_dic = {str(k): v for k, v in igt.items()}
    seen = []
    h = logging.Handler()
    h.emit = lambda rec: seen.append(rec.getMessage())
    G.logger.addHandler(h)
    G.logger.setLevel(logging.INFO)
    args = _args(tmp, "gqa", bs)
    results = G.evaluate(args, _RowModel(rows, mask_pos, L), ds, tokenizer=tok)
    G.logger.removeHandler(h)
    with open(os.path.join(args.result_dir, "val_results.pk"), "rb") as f:
        kept = pickle.load(f)
    acc = sum(bool(r["correct"]) for r in kept) / len(ds)
    score = [m for m in seen if m.startswith("Eval Score:")]
    assert len(score) == 1 and score[0] == "Eval Score: %.3f" % (100 * acc), (score, acc)
    assert len(results) == n_q and len(kept) == n_q - 1
    correct = [bool(r["correct"]) for r in results]
    assert any(correct) and not all(correct)
    assert results[1]["answer"] == "cat" and results[3]["answer"] == "holding" and not correct[3] and results[4]["answer"] == "cup"
    assert correct[2] != correct[8]                 # the repeated question_id decides the accuracy
    G_max = max(len(v) for v in igt.values())
    gt = np.full((n_q, G_max), -1, dtype=np.int64)
    for i in range(n_q):
        gt[i, :len(igt[q_ids[i]])] = igt[q_ids[i]]
    np.savez_compressed(os.path.join(OUT, "tiny_gqa_eval.npz"), labels=np.array(labels), rows=rows.numpy(), mask_pos=np.array(mask_pos),
                        logits=np.stack([r["logits"] for r in results]), q_ids=np.array(q_ids), igt=gt, batch=np.array(bs),
                        answer=np.array([r["answer"] for r in results]), correct=np.array(correct),
                        question_id=np.array([int(r["question_id"]) for r in results]), acc=np.array(acc))


class _ListDataset(list):
    name = "val"


class _RelModel(object):
    def __init__(self, rel):
        self.rel, self.at = rel, 0

    def eval(self):
        return self

    def __call__(self, **kw):
        B = kw["input_ids"].size(0)
        out = self.rel[self.at:self.at + B]
        self.at += B
        return (out,)


def vcr_eval_fixture(tmp, rng):
    interval, n_q, bs, n_rel = 4, 7, 3, 3
    pool = torch.from_numpy(rng.standard_normal((6, n_rel)).astype(np.float32))
    sc = 1 - pool.double().softmax(-1)[:, 1]
    gaps = (sc[:, None] - sc[None, :]).abs() + torch.eye(6)
    assert float(gaps.min()) >= 1e-3, "pool rows must be 1e-3 apart in choice score"
    pick = rng.integers(0, 6, (n_q, interval))
    pick[3] = pick[3, 0]                             # all four choices identical: the first wins
    pick[5, 2] = pick[5, 0]
    rel = pool[torch.from_numpy(pick.reshape(-1))]
    # tie-or-gap rule inside every question (identical rows or >= 1e-3 apart): by construction of the pool, asserted anyway
    s64 = (1 - rel.double().softmax(-1)[:, 1]).view(n_q, interval)
    for q in range(n_q):
        for a in range(interval):
            for b in range(a + 1, interval):
                same = bool((rel[q * interval + a] == rel[q * interval + b]).all())
                assert same or abs(float(s64[q, a] - s64[q, b])) >= 1e-3
    labels = [int(x) for x in rng.integers(0, interval, n_q)]
    labels[3] = 0
    q_ids = [900 + i for i in range(n_q)]
    q_ids[6] = q_ids[1]
    items = []
    for q in range(n_q):
        items.append([(torch.zeros(4, dtype=torch.long), torch.ones(6, dtype=torch.long), torch.zeros(4, dtype=torch.long), torch.zeros(2, 3),
                       q_ids[q], labels[q], []) for _ in range(interval)])
    args = _args(tmp, "vcr", bs)
    results, acc = V.evaluate(args, _RelModel(rel), _ListDataset(items))
    assert len(results) == n_q
    correct = [bool(r["correct"]) for r in results]
    assert any(correct) and not all(correct)
    np.savez_compressed(os.path.join(OUT, "tiny_vcr_nsp_eval.npz"), rel=rel.numpy(), labels=np.array(labels), q_ids=np.array(q_ids),
                        interval=np.array(interval), batch=np.array(bs), answer=np.array([int(r["answer"]) for r in results]),
                        correct=np.array(correct), questionId=np.array([int(r["questionId"]) for r in results]),
                        choice_logits=np.stack([r["logits"] for r in results]), acc=np.array(float(acc)))


# ---- the training traces ----
NO_DECAY = ["bias", "LayerNorm.weight"]                 # gqa_cpt.py:337, vcr_nsp_cpt.py:380
SAMPLE = ["bert.embeddings.LayerNorm.weight", "bert.img_embedding.weight", "bert.encoder.layer.0.attention.self.query.weight",
          "bert.encoder.layer.1.intermediate.dense.weight", "bert.encoder.layer.1.output.LayerNorm.weight", "bert.encoder.layer.1.output.dense.bias"]
N_SAMPLE = 24
TRAIN = {"micro": 6, "gas": 2, "B": 4, "max_seq_len": 20, "img_seq_len": 6, "warmup_steps": 1, "t_total": 4,
         "gqa": {"lr": 5e-5, "eps": 1e-8, "weight_decay": 0.05, "max_grad_norm": 0.05, "seed0": 41},      # gqa_cpt.py:844-845 defaults, cmds' decay
         "vcr": {"lr": 5e-5, "eps": 1e-6, "weight_decay": 0.01, "max_grad_norm": 0.05, "seed0": 61}}
GQA_LABEL_TOKENS = [150, 200, 201, 333, 150, 410, 277]  # first-piece ids of seven labels (one id twice, as in the real label list)


class _HFAdamW(object):
    """The call pattern of pytorch_transformers.AdamW on named parameters, arithmetic from the oracle's restatement."""

    def __init__(self, model, lr, eps, weight_decay):
        self.named = [(n, p) for n, p in model.named_parameters()]
        self.lr0, self.lr, self.eps, self.wd, self.state = lr, lr, eps, weight_decay, {}

    def step(self):
        for n, p in self.named:
            if p.grad is None:
                continue
            st = self.state.setdefault(n, {"step": 0, "m": torch.zeros_like(p), "v": torch.zeros_like(p)})
            st["step"] += 1
            wd = 0.0 if any(nd in n for nd in NO_DECAY) else self.wd
            with torch.no_grad():
                new, st["m"], st["v"] = O.adamw_step_hf(p.data, p.grad, st["m"], st["v"], st["step"], self.lr, 0.9, 0.999, self.eps, wd)
                p.data.copy_(new)


def _trace(model, micro_losses, hp):
    opt = _HFAdamW(model, hp["lr"], hp["eps"], hp["weight_decay"])
    epoch = 0
    opt.lr = hp["lr"] * O.warmup_linear_schedule(epoch, TRAIN["warmup_steps"], TRAIN["t_total"])
    gas = TRAIN["gas"]
    losses, norms, params = [], [], []
    named = dict(model.named_parameters())
    model.zero_grad()
    for step, loss in enumerate(micro_losses):
        if gas > 1:
            loss = loss / gas
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(model.parameters(), hp["max_grad_norm"])
        assert hp["max_grad_norm"] / (float(norm) + 1e-6) < 1.0, "the clip must act on every micro-step"
        losses.append(float(loss.detach()))
        norms.append(float(norm))
        if (step + 1) % gas == 0:
            epoch += 1                                   # scheduler.step()
            opt.lr = hp["lr"] * O.warmup_linear_schedule(epoch, TRAIN["warmup_steps"], TRAIN["t_total"])
            opt.step()
            model.zero_grad()
            params.append(np.stack([named[n].detach().reshape(-1)[:N_SAMPLE].numpy().copy() for n in SAMPLE]))
    return np.array(losses, dtype=np.float64), np.array(norms, dtype=np.float64), np.stack(params)


def _ref_models():
    cfg = cfgmod.tiny()
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
    rc = ref_stub.BertConfig(**cfg.to_dict())

    def pre():
        p = BertImgForPreTraining(rc)
        p.load_state_dict(synth.init_state_dict(cfg, 4321, head="pretrain"), strict=True)
        p.tie_weights()
        return p
    gq = REC_MLM_CPT(rc)
    gq.copy_from_pretraining_model(pre())
    vc = NSPCPT(rc)
    vc.copy_from_pretraining_model(pre())
    return cfg, gq.train(), vc.train()


def train_fixture(rng):
    cfg, gq, vc = _ref_models()
    T = TRAIN
    g = {"sample_names": np.array(SAMPLE), "n_sample": np.array(N_SAMPLE), "gqa_label_tokens": np.array(GQA_LABEL_TOKENS)}
    for k in ("micro", "gas", "B", "max_seq_len", "img_seq_len", "warmup_steps", "t_total"):
        g[k] = np.array(T[k])
    batches = lambda s0: [synth.make_batch(T["B"], cfg, seed=s0 + i, max_seq_len=T["max_seq_len"], img_seq_len=T["img_seq_len"], vary_regions=True)
                          for i in range(T["micro"])]
    # GQA (gqa_cpt.py:427-441): -1 everywhere, label_token_ids[label] at the input_ids == 103 slots
    label_ids = rng.integers(0, len(GQA_LABEL_TOKENS), (T["micro"], T["B"]))
    label_token_ids = torch.tensor(GQA_LABEL_TOKENS, dtype=torch.long)

    def gqa_micro():
        for i, b in enumerate(batches(T["gqa"]["seed0"])):
            mlm_labels = torch.zeros(b["attention_mask"].size(), dtype=torch.long)
            mlm_labels[:] = -1
            idxs = (b["input_ids"] == 103).nonzero(as_tuple=False).tolist()
            idxs0, idxs1 = [x[0] for x in idxs], [x[1] for x in idxs]
            mlm_labels[idxs0, idxs1] = label_token_ids[torch.from_numpy(label_ids[i])]
            yield gq(input_ids=b["input_ids"], attention_mask=b["attention_mask"], token_type_ids=b["segment_ids"], masked_lm_labels=mlm_labels,
                     img_feats=b["img_feats"])[0]
    g["gqa_label_ids"] = label_ids
    g["gqa_loss"], g["gqa_norm"], g["gqa_params"] = _trace(gq, gqa_micro(), T["gqa"])
    # VCR (vcr_nsp_cpt.py:433-444): one question of 4 choices per micro-step, class 0 at the right choice
    interval = T["B"]
    vcr_labels = rng.integers(0, interval, T["micro"])

    def vcr_micro():
        for i, b in enumerate(batches(T["vcr"]["seed0"])):
            cls_labels = torch.ones([interval], dtype=torch.long)
            cls_labels[0 * interval + int(vcr_labels[i])] = 0
            yield vc(input_ids=b["input_ids"], attention_mask=b["attention_mask"], token_type_ids=b["segment_ids"], next_sentence_label=cls_labels,
                     img_feats=b["img_feats"])[0]
    g["vcr_labels"] = vcr_labels
    g["vcr_loss"], g["vcr_norm"], g["vcr_params"] = _trace(vc, vcr_micro(), T["vcr"])
    for task in ("gqa", "vcr"):
        g[task + "_hyper"] = np.array([T[task][k] for k in ("lr", "eps", "weight_decay", "max_grad_norm")])
        g[task + "_seed0"] = np.array(T[task]["seed0"])
    np.savez_compressed(os.path.join(OUT, "tiny_gqa_vcr_train.npz"), **g)
    print("gqa loss", g["gqa_loss"], "norm", g["gqa_norm"])
    print("vcr loss", g["vcr_loss"], "norm", g["vcr_norm"])


def main():
    logging.disable(logging.DEBUG)
    torch.manual_seed(0)
    rng = np.random.Generator(np.random.PCG64(808))
    tmp = tempfile.mkdtemp()
    gqa_eval_fixture(tmp, rng)
    vcr_eval_fixture(tmp, rng)
    train_fixture(rng)
    for n in ("tiny_gqa_eval.npz", "tiny_vcr_nsp_eval.npz", "tiny_gqa_vcr_train.npz"):
        print("wrote", os.path.join(OUT, n), os.path.getsize(os.path.join(OUT, n)), "bytes")


if __name__ == "__main__":
    main()
