"""Golden vectors of VG-CPT predicate scoring from the reference's own val() (Oscar/oscar/fewshot/vg_cpt.py:255-305).

Runs on a CPU box with the reference checked out (default /root/reference, or $CPT_REFERENCE), importing its modules through
oracle/ref_stub.py as oracle/make_golden_gqa_vcr.py does; nothing of the reference is copied.  val() gets:
  - a small word-piece vocabulary ([MASK] = 103) with predicates of 1, 2 and 3 pieces, "has" scored as "having" (rel2rel);
  - a list-based loader of two batches in test_collate's form (6 sequences per pair, k mask positions on the k-mask sequences);
  - a stand-in model that returns fixed random (B, L, V) prediction scores -- val() is a function of those scores only.
eval_vg is replaced by a no-op and reads an empty ground-truth pickle: the golden is the prediction dict val() saves as val.pt.

Writes tests/golden/tiny_vg_val.npz and tests/golden/tiny_vg_META.json.  Deterministic: re-running rewrites identical files.
"""
import hashlib
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
OUT = os.path.join(ROOT, "tests", "golden")

import ref_stub  # noqa: E402

pkg = ref_stub.install()
from transformers import BertTokenizer  # noqa: E402

pkg.BertTokenizer = BertTokenizer
sys.modules.setdefault("tqdm", types.SimpleNamespace(tqdm=lambda it, **kw: it))
sys.path.insert(0, os.path.join(REF, "Oscar"))
import oscar.fewshot.vg_cpt as VG  # noqa: E402

VOCAB = (["[PAD]"] + ["[unused%d]" % i for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"] +
         ["the", "a", "is", "man", "shirt", "table", "on", "having", "wearing", "in", "front", "of", "next", "to", "under", "near",
          "holding", "sitting", "behind", "above", "riding", "parked", "along", "with"])
PREDICATES = {"1": "on", "2": "has", "3": "wears", "4": "in front of", "5": "next to", "6": "under", "7": "near", "8": "holding",
              "9": "sitting on", "10": "behind", "11": "above", "12": "riding", "13": "parked along", "14": "with"}
N_PRED = len(PREDICATES)      # val() scores len(idx2pred) + 1 slots, 0 = background


def main():
    torch.manual_seed(0)
    tmp = tempfile.mkdtemp()
    vf = os.path.join(tmp, "vocab.txt")
    with open(vf, "w") as f:
        f.write("\n".join(VOCAB) + "\n")
    tok = BertTokenizer(vf, do_lower_case=True)
    assert tok.convert_tokens_to_ids(["[MASK]"]) == [103]
    vocab_json = os.path.join(tmp, "vg_vocab.json")
    with open(vocab_json, "w") as f:
        json.dump({"idx_to_predicate": PREDICATES}, f)
    gt_path = os.path.join(tmp, "val_gt.pkl")
    with open(gt_path, "wb") as f:
        pickle.dump([], f)
    V, L = len(VOCAB), 12
    batches, all_logits, all_pos, keys = [], [], [], []
    pair_keys = [["1.jpg_0_1", "1.jpg_2_0"], ["2.jpg_1_3"]]
    for bk in pair_keys:
        B = 6 * len(bk)
        mpos = [list(range(2, 2 + s % 3 + 1)) for s in range(B)]
        logits = torch.randn(B, L, V) * 3
        batch = (torch.zeros(B, 4, 8), torch.zeros(B, L, dtype=torch.long), torch.ones(B, L, dtype=torch.long),
                 torch.zeros(B, L, dtype=torch.long), mpos, [None] * B)
        batches.append((bk, batch))
        all_logits.append(logits)
        all_pos += mpos
        keys += bk
    step = {"i": 0}

    def model(input_ids, segment_ids, input_mask, img_feats=None):
        out = all_logits[step["i"]]
        step["i"] += 1
        return (out,)
    model.eval = lambda: None
    args = types.SimpleNamespace(vocab=vocab_json, device="cpu", result_dir=os.path.join(tmp, "result"))
    VG.eval_vg = lambda preds, gts: {}
    VG.logger = logging.getLogger("make_golden_vg")      # (val() logs through the module global main() sets up)
    VG.val(args, batches, model, tok, gt_path)
    preds = torch.load(os.path.join(args.result_dir, "val.pt"))
    scores = np.stack([np.stack([preds[k].numpy(), preds[VG.reverse_imkey(k)].numpy()]) for k in keys]).astype(np.float32)
    assert scores.shape == (len(keys), 2, N_PRED + 1)
    idx2pred = {int(i): tok.convert_tokens_to_ids(tok.tokenize({"has": "having", "wears": "wearing", "says": "saying"}.get(p, p)))
                for i, p in PREDICATES.items()}
    rows = np.concatenate([lg[s, list(range(2, 2 + s % 3 + 1))].numpy() for lg, bk in zip(all_logits, pair_keys) for s in range(6 * len(bk))], 0)
    row_seq = np.array([s for s, p in enumerate(all_pos) for _ in p], dtype=np.int64)
    pieces = np.full((N_PRED + 1, 3), -1, dtype=np.int64)
    for i, t in idx2pred.items():
        pieces[i, :len(t)] = t
    g = {"row_logits": rows.astype(np.float32), "row_seq": row_seq, "pred_pieces": pieces, "val_scores": scores,
         "vocab": np.array(VOCAB), "predicates": np.array([PREDICATES.get(str(i), "") for i in range(N_PRED + 1)])}
    path = os.path.join(OUT, "tiny_vg_val.npz")
    np.savez(path, **g)
    with open(path, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()
    meta = {"tiny_vg_val.npz": {
        "generator": "tools/make_golden_vg.py",
        "reference": "Oscar/oscar/fewshot/vg_cpt.py val() (lines 255-305), run unmodified on a list-based loader; eval_vg replaced by a no-op",
        "contents": "row_logits: [MASK]-row scores (n, V) of 18 sequences (3 pairs, 6 sequences each, k rows on the k-mask sequences); "
                    "row_seq: their sequence; pred_pieces: word-pieces of each predicate index (-1 = none), as val() tokenizes them "
                    "(rel2rel applied); val_scores: (pairs, 2, 15) = predictions[im_key], predictions[reverse_imkey(im_key)] read back from val.pt",
        "sha256": digest}}
    with open(os.path.join(OUT, "tiny_vg_META.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, digest)


if __name__ == "__main__":
    main()
