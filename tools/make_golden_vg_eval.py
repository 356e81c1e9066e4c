"""Golden vectors of the VG-CPT prompt rows and Recall@K from the reference's own code: ZSLVGDataset / FtVGDataset.__getitem__
(Oscar/oscar/datasets/vg_test_dataset.py:37-77, vg_cpt_dataset.py:37-101) and eval_vg (Oscar/oscar/utils/vg_eval.py).

Runs on a CPU box with the reference checked out (default /root/reference, or $CPT_REFERENCE), importing its modules through
oracle/ref_stub.py as tools/make_golden_vg.py does; nothing of the reference is copied.  Writes
  tests/golden/tiny_vg_rows.tsv (+ .lineidx): four VG rows over two images, 2054-d random features, 3-4 regions; rel_name "on",
    "has" (rel2rel: "having"), "next to" (2 word-pieces) and "in front of" (3);
  tests/golden/tiny_vg_eval.npz: the datasets' outputs for every row (zsl*/tr* arrays), and eval_vg's string on a val.pt-style
    prediction dict (keys + scores (n, 51)) and ground truth covering an image without prediction, one with fewer than 20 candidates,
    one with more than 100, a pair whose reverse is also a key, and predicates absent from the ground truth;
  tests/golden/tiny_vg_eval_META.json.
Deterministic: re-running rewrites identical files.
"""
import base64
import hashlib
import io as _io
import json
import os
import sys
import tempfile
import types
from contextlib import redirect_stdout

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
from oscar.utils.tsv_file import TSVFile  # noqa: E402
from oscar.utils.vg_eval import eval_vg  # noqa: E402
import oscar.datasets.vg_test_dataset as ZD  # noqa: E402
import oscar.datasets.vg_cpt_dataset as FD  # noqa: E402

VOCAB = (["[PAD]"] + ["[unused%d]" % i for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"] +
         ["the", "a", "is", "in", "color", "red", "blue", "green", "man", "shirt", "table", "dog", "hat", "on", "having", "wearing",
          "next", "to", "front", "of", "irrelevant", "no", "relation", "with", "near"])
# (image name, box classes, [subject colour, object colour], [subject name, object name], rel_name)
ROWS = [("10.jpg_0_1", ["man", "shirt", "table"], ["red", "blue"], ["man", "shirt"], "has"),
        ("10.jpg_1_0", ["man", "shirt", "table"], ["blue", "red"], ["shirt", "man"], "on"),
        ("10.jpg_2_0", ["man", "shirt", "table"], ["green", "red"], ["table", "man"], "next to"),
        ("20.jpg_1_0", ["dog", "hat", "man", "table"], ["red", "green"], ["hat", "dog"], "in front of")]
N_SLOTS = 51


def tokenizer(tmp):
    vf = os.path.join(tmp, "vocab.txt")
    with open(vf, "w") as f:
        f.write("\n".join(VOCAB) + "\n")
    tok = BertTokenizer(vf, do_lower_case=True)
    assert tok.convert_tokens_to_ids(["[MASK]"]) == [103]
    return tok


def write_rows(rng):
    tsv = os.path.join(OUT, "tiny_vg_rows.tsv")
    lines = []
    for name, classes, colors, names, rel in ROWS:
        boxes = []
        for j, c in enumerate(classes):
            f = rng.standard_normal(2054).astype(np.float32)
            boxes.append({"rect": [float(10 * j), 5.0, float(10 * j + 40), 60.0], "class": c, "conf": 0.5,
                          "feature": base64.b64encode(f.tobytes()).decode("utf-8")})
        lines.append(name + "\t" + json.dumps({"objects": [[boxes], colors, names, rel]}))
    with open(tsv, "w") as f:
        f.write("\n".join(lines) + "\n")
    if os.path.exists(os.path.join(OUT, "tiny_vg_rows.lineidx")):
        os.remove(os.path.join(OUT, "tiny_vg_rows.lineidx"))
    return tsv


def prompt_case(g, tok, tsv):
    for cls, tag in ((ZD.ZSLVGDataset, "zsl"), (FD.FtVGDataset, "tr")):
        ds = object.__new__(cls)
        ds.tokenizer, ds.vocab, ds.txt_seq_len, ds.img_seq_len, ds.is_train = tok, tok.vocab, 70, 60, tag == "tr"
        ds.corpus_tsvfile = TSVFile(tsv, generate_lineidx=True)
        for i in range(len(ROWS)):
            out = ds[i]
            k = "%s%d_" % (tag, i)
            g[k + "ids"], g[k + "mask"], g[k + "seg"] = [torch.stack(x).numpy() for x in out[2:5]]
            mpos = out[5]
            g[k + "mpos"] = np.array([[s, int(p)] for s, ps in enumerate(mpos) for p in torch.as_tensor(ps).reshape(-1).tolist()])
            g[k + "feat_sum"] = np.array([float(f.double().sum()) for f in out[1]])
            if tag == "tr":
                g[k + "labels"] = np.array([y for x in out[7] for y in x])


def recall_case(g, rng):
    """A val.pt-style dict: image 1 has no prediction, image 2 few candidates (a pair and its reverse both keys), image 3 132 candidates,
    image 4 a few; 51-slot scores, continuous (no ties at the K boundaries); predicates 40.. never in the ground truth."""
    preds = {}
    for img, boxes, every in (("2.jpg", 4, False), ("3.jpg", 12, True), ("4.jpg", 3, True)):
        pairs = [(s, o) for s in range(boxes) for o in range(boxes) if s != o]
        if not every:
            pairs = [(0, 1), (1, 0), (2, 3), (3, 1), (1, 2)]
        for s, o in pairs:
            v = torch.from_numpy(rng.standard_normal(N_SLOTS).astype(np.float32) * 2 - 3)
            preds["%s_%d_%d" % (img, s, o)] = v
    # let the ground truth hit some top-ranked predictions: the predicted relation of a few pairs
    def best(k):
        return int(preds[k][1:].argmax()) + 1
    gts = [{"img_path": "1.jpg", "relations": np.array([[0, 1, 3], [1, 0, 7]])},
           {"img_path": "2.jpg", "relations": np.array([[0, 1, best("2.jpg_0_1")], [1, 0, best("2.jpg_1_0")], [2, 3, 5], [3, 1, 9]])},
           {"img_path": "3.jpg", "relations": np.array([[s, o, best("3.jpg_%d_%d" % (s, o)) if (s + o) % 3 else 1 + (s * 7 + o) % 30]
                                                        for s, o in [(0, 1), (2, 5), (7, 3), (11, 4), (6, 9), (1, 10), (5, 6), (8, 2), (4, 7)]] + [[5, 5, 4]])},
           {"img_path": "4.jpg", "relations": np.array([[0, 2, best("4.jpg_0_2")], [2, 1, 12]])}]
    with redirect_stdout(_io.StringIO()):
        rst = eval_vg(preds, gts)
    g["pred_keys"] = np.array(list(preds.keys()))
    g["pred_scores"] = torch.stack(list(preds.values())).numpy()
    g["gt_imgs"] = np.array([x["img_path"] for x in gts])
    g["gt_rels"] = np.concatenate([x["relations"] for x in gts]).astype(np.int64)
    g["gt_counts"] = np.array([len(x["relations"]) for x in gts])
    g["eval_string"] = np.array(rst)
    return rst


def main():
    torch.manual_seed(0)
    rng = np.random.Generator(np.random.PCG64(150))
    tmp = tempfile.mkdtemp()
    tok = tokenizer(tmp)
    tsv = write_rows(rng)
    g = {"vocab": np.array(VOCAB)}
    prompt_case(g, tok, tsv)
    rst = recall_case(g, rng)
    path = os.path.join(OUT, "tiny_vg_eval.npz")
    np.savez(path, **g)
    meta = {}
    for f in ("tiny_vg_eval.npz", "tiny_vg_rows.tsv", "tiny_vg_rows.lineidx"):
        with open(os.path.join(OUT, f), "rb") as fh:
            meta[f] = {"sha256": hashlib.sha256(fh.read()).hexdigest()}
    meta["tiny_vg_eval.npz"].update({
        "generator": "tools/make_golden_vg_eval.py",
        "reference": "ZSLVGDataset / FtVGDataset.__getitem__ (datasets/vg_test_dataset.py, vg_cpt_dataset.py) on tiny_vg_rows.tsv; "
                     "eval_vg (utils/vg_eval.py) on pred_keys / pred_scores and gt_imgs / gt_rels / gt_counts",
        "contents": "zsl<i>_{ids,mask,seg,mpos,feat_sum}, tr<i>_{ids,mask,seg,mpos,feat_sum,labels} per TSV row i (mpos: (sequence, position) "
                    "rows); pred_keys, pred_scores (n, 51) in dict order; ground truth; eval_string: eval_vg's returned string"})
    with open(os.path.join(OUT, "tiny_vg_eval_META.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(rst, end="")
    print("wrote", path)


if __name__ == "__main__":
    main()
