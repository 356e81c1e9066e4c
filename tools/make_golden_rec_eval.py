"""Golden vectors of the RefCOCO REC evaluation from the reference's own code: the two val() functions (Oscar/oscar/zeroshot/refcoco_cpt.py:208-288,
Oscar/oscar/fewshot/refcoco_cpt.py:258-315) and oscar.utils.iou.computeIoU.

Runs on a CPU box with the reference checked out (default /root/reference, or $CPT_REFERENCE), importing its modules through oracle/ref_stub.py as
tools/make_golden_gqa_vcr_eval.py does; nothing of the reference is copied.  Both val() functions run WHOLE, on planted [MASK]-row scores: a stand-in
model hands the planted row back at every sequence's mask_token_pos, a stand-in loader yields batches in test_collate's layout, a stand-in tokenizer
maps the colour words to ids.  What val() keeps to itself is read off its own call of computeIoU (the module's name is wrapped by a recorder that
calls the real function): the converted box, the annotation and the IoU of every query.  The chosen rectangle -- and with it max_idx, every
candidate rectangle of a query being distinct -- is the candidate whose conversion [x1, y1, x2 - x1 + 1, y2 - y1 + 1] equals the recorded box.
tiny_rec_eval_META.json says what ran from the reference and what this file restates.  The fixture holds data only.

Planted: fractional coordinates whose IoU changes in its last bits when w1 * h1 + w2 * h2 is fused (checked here with exact rational arithmetic,
both ways of fusing); a chosen box with IoU exactly 0.5 (not correct: the test is >); a pair of touching boxes (intersection 0 by the strict <);
an exact tie between two sequences of one query (the first wins); a negative "none" logit (the few-shot quotient reverses the order); sequences
of 5, 5 and 2 colours; integer and float rectangles.

    python tools/make_golden_rec_eval.py     # rewrites tests/golden/tiny_rec_eval.npz and tiny_rec_eval_META.json (the same arrays every time)
"""
import json
import logging
import os
import sys
import types
from fractions import Fraction

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
import oscar.zeroshot.refcoco_cpt as Z  # noqa: E402
import oscar.fewshot.refcoco_cpt as F  # noqa: E402
from oscar.utils.iou import computeIoU  # noqa: E402

WORDS = {"red": 5, "purple": 6, "green": 7, "yellow": 8, "blue": 9, "none": 10}
V, L, BATCH = 12, 6, 2


class _Tokenizer(object):
    def convert_tokens_to_ids(self, tokens):
        return [WORDS[t] for t in tokens]


class _RowModel(object):
    """val() reads output[b, mask_token_pos[b], :]: hand it the planted rows there, in call order."""

    def __init__(self, rows, mask_pos):
        self.rows, self.mask_pos, self.at = rows, mask_pos, 0

    def eval(self):
        return self

    def __call__(self, input_ids, segment_ids, input_mask, img_feats=None):
        B = input_ids.size(0)
        out = torch.zeros(B, L, self.rows.size(1))
        for b in range(B):
            out[b, self.mask_pos[self.at + b]] = self.rows[self.at + b]
        self.at += B
        return (out,)


class _Loader(list):
    pass


def _round_fraction(x):
    return float(x)            # Fraction -> float is correctly rounded


def fused_variants(rect, gt):
    """computeIoU of the converted box with w1 * h1 + w2 * h2 fused either way (one rounding for product + sum), exact rational arithmetic."""
    p = [rect[0], rect[1], rect[2] - rect[0] + 1, rect[3] - rect[1] + 1]
    ix1, iy1 = max(p[0], gt[0]), max(p[1], gt[1])
    ix2, iy2 = min(p[0] + p[2] - 1, gt[0] + gt[2] - 1), min(p[1] + p[3] - 1, gt[1] + gt[3] - 1)
    inter = (ix2 - ix1 + 1) * (iy2 - iy1 + 1) if (ix1 < ix2 and iy1 < iy2) else 0
    a = _round_fraction(Fraction(p[2]) * Fraction(p[3]) + Fraction(gt[2] * gt[3])) - inter
    b = _round_fraction(Fraction(p[2] * p[3]) + Fraction(gt[2]) * Fraction(gt[3])) - inter
    return float(inter) / a, float(inter) / b


def find_fractional_case(rng):
    """A box and an annotation with fractional coordinates whose IoU differs from BOTH fused forms (a clear hit either way: above 0.6)."""
    for _ in range(100000):
        x1, y1 = [round(float(v), 2) for v in rng.uniform(5, 60, 2)]
        w, h = [round(float(v), 2) for v in rng.uniform(40, 120, 2)]
        rect = [x1, y1, x1 + w, y1 + h]
        gt = [round(float(v), 2) for v in (x1 + rng.uniform(-8, 8), y1 + rng.uniform(-8, 8), w + rng.uniform(-6, 6), h + rng.uniform(-6, 6))]
        p = [rect[0], rect[1], rect[2] - rect[0] + 1, rect[3] - rect[1] + 1]
        iou = computeIoU(p, gt)
        fa, fb = fused_variants(rect, gt)
        if iou != fa and iou != fb and iou > 0.6:
            return rect, gt
    raise RuntimeError("no contraction-sensitive case found")


def build_queries(rng):
    """(queries, annotations): a query = (key, colour words per sequence, rectangles per sequence)."""
    frac_rect, frac_gt = find_fractional_case(rng)
    qs, gts = [], {}

    def add(colors, rects, bbox):
        k = "q%d" % len(qs)
        qs.append((k, colors, rects))
        gts[k] = {"bbox": bbox, "file_name": k + ".jpg", "caption": "the thing " + k}

    five = ["red", "purple", "green", "yellow", "blue"]
    # 0: fractional coordinates; the chosen one (planted) is the contraction-sensitive rectangle
    add([five[:3]], [[[3.25, 4.5, 50.75, 61.125], frac_rect, [70.1, 10.2, 99.9, 40.4]]], frac_gt)
    # 1: IoU exactly 0.5 -- [0, 0, 10, 10] against [0, 0, 10, 5]: 50 / (100 + 50 - 50)
    add([five[:2], five[:1]], [[[20, 20, 25, 26], [0, 0, 9, 9]], [[40, 40, 45, 47]]], [0, 0, 10, 5])
    # 2: touching boxes -- the chosen [0, 0, 10, 10] and the annotation [9, 0, 10, 10] share the pixel column 9: inter_x1 == inter_x2, intersection 0
    add([five[:2]], [[[0, 0, 9, 9], [30, 30, 50, 50]]], [9, 0, 10, 10])
    # 3: an exact tie between two sequences (planted): the first sequence's candidate wins; the annotation fits the SECOND one
    add([five[:2], five[:2]], [[[10, 10, 40, 40], [12, 60, 30, 90]], [[100, 100, 140, 150], [1, 2, 3, 4]]], [100, 100, 41, 51])
    # 4: a negative "none" logit in its second sequence (planted): zero-shot takes the largest logit, few-shot the most negative one of that sequence
    add([five[:3], five[:3]], [[[5, 5, 60, 60], [6, 70, 61, 120], [70, 5, 120, 60]], [[8, 8, 58, 58], [64, 64, 128, 128], [2, 90, 40, 126]]],
        [8.0, 8.0, 51.0, 51.0])
    # 5: sequences of 5, 5 and 2 colours, float annotation
    r5 = [[[10 * j + 3 * k, 7 * k + 2 * j, 10 * j + 3 * k + 25 + k, 7 * k + 2 * j + 31 + j] for k in range(n)] for j, n in enumerate((5, 5, 2))]
    add([five, five, five[:2]], r5, [13.0, 9.5, 27.25, 33.5])
    # 6: one sequence, one colour, a clean hit
    add([five[:1]], [[[15, 25, 115, 225]]], [15, 25, 101, 201])
    return qs, gts, frac_rect


def plant_scores(rng, qs):
    """(S_total, V) fp32 [MASK]-row scores and each sequence's mask position.  Random rows drawn from a coarse grid, "none" logits positive, then
    the planted cells."""
    n_seq = sum(len(c) for _, c, _ in qs)
    rows = torch.from_numpy((rng.integers(-8, 9, (n_seq, V)) / 4.0).astype(np.float32))
    rows[:, WORDS["none"]] = torch.from_numpy(rng.choice([0.5, 1.25, 2.0, 3.0], n_seq).astype(np.float32))
    first = np.cumsum([0] + [len(c) for _, c, _ in qs]).tolist()
    W = WORDS
    # (the planted maxima sit in rows with "none" = 1 and exceed 2 / 0.5, the largest quotient a random cell can reach: both val()s choose them)
    rows[first[0], W["purple"]], rows[first[0], W["none"]] = 6.0, 1.0   # q0: the fractional rectangle
    rows[first[1], W["purple"]], rows[first[1], W["none"]] = 7.0, 1.0   # q1: [0, 0, 9, 9]
    rows[first[2], W["red"]], rows[first[2], W["none"]] = 7.5, 1.0      # q2: [0, 0, 9, 9]
    for s in (first[3], first[3] + 1):                                  # q3: both sequences alike: logit 5 / none 2 at "red", nothing above
        rows[s, W["red"]], rows[s, W["purple"]], rows[s, W["none"]] = 5.0, 1.0, 2.0
    s = first[4]                                                        # q4: first sequence none = 2; second sequence none = -0.5
    rows[s, W["red"]], rows[s, W["purple"]], rows[s, W["green"]], rows[s, W["none"]] = 3.0, 1.0, 0.5, 2.0
    rows[s + 1, W["red"]], rows[s + 1, W["purple"]], rows[s + 1, W["green"]], rows[s + 1, W["none"]] = 2.0, -1.5, 0.25, -0.5
    rows[first[5] + 2, W["purple"]], rows[first[5] + 2, W["none"]] = 9.0, 1.0      # q5: the last candidate, in the 2-colour sequence
    mask_pos = [int(x) for x in rng.integers(1, L, n_seq)]
    return rows, mask_pos


def run_val(mod, qs, anns, rows, mask_pos):
    """mod.val() whole, on the planted scores.  Returns (percent, [(converted box, annotation, iou) per computeIoU call, in call order])."""
    seen = []
    real = mod.computeIoU

    def recorder(box1, box2):
        iou = real(box1, box2)
        seen.append((list(box1), list(box2), iou))
        return iou
    loader = _Loader()
    at = 0
    for b0 in range(0, len(qs), BATCH):
        chunk = qs[b0:b0 + BATCH]
        n = sum(len(c) for _, c, _ in chunk)
        batch = (torch.zeros(n, 2, 3), torch.zeros(n, L, dtype=torch.long), torch.ones(n, L + 2, dtype=torch.long), torch.zeros(n, L, dtype=torch.long),
                 torch.tensor(mask_pos[at:at + n], dtype=torch.long), tuple(c for _, c, _ in chunk), tuple(r for _, _, r in chunk))
        loader.append((tuple(k for k, _, _ in chunk), batch))
        at += n
    loader.dataset = types.SimpleNamespace(anns_dic=anns)
    mod.logger = logging.getLogger("rec_eval_fixture")
    mod.computeIoU = recorder
    try:
        pct = mod.val(types.SimpleNamespace(device=torch.device("cpu")), loader, _RowModel(rows, mask_pos), _Tokenizer())
    finally:
        mod.computeIoU = real
    return pct, seen


def main():
    rng = np.random.Generator(np.random.PCG64(2718))
    qs, anns, frac_rect = build_queries(rng)
    rows, mask_pos = plant_scores(rng, qs)
    Q = len(qs)
    C = max(len(c) for _, cs, _ in qs for c in cs)
    n_seq = [len(c) for _, c, _ in qs]
    colors = np.full((sum(n_seq), C), -1, dtype=np.int64)
    rect_rows, rect_first = [], [0]
    s = 0
    for _, cs, rs in qs:
        for c, r in zip(cs, rs):
            colors[s, :len(c)] = [WORDS[w] for w in c]
            rect_rows += [[float(x) for x in box] for box in r]
            s += 1
        rect_first.append(len(rect_rows))
    g = {"scores": rows.numpy(), "mask_pos": np.array(mask_pos), "n_seq": np.array(n_seq), "colors": colors, "rects": np.array(rect_rows, dtype=np.float64),
         "rect_first": np.array(rect_first), "gt": np.array([anns[k]["bbox"] for k, _, _ in qs], dtype=np.float64), "none_id": np.array(WORDS["none"]),
         "batch": np.array(BATCH), "vocab": np.array(V)}
    for name, mod in (("zsl", Z), ("fsl", F)):
        pct, seen = run_val(mod, qs, anns, rows, mask_pos)
        assert len(seen) == Q
        max_idx, chosen, ious, flags = [], [], [], []
        for (k, cs, rs), (box, bbox, iou) in zip(qs, seen):
            assert bbox == anns[k]["bbox"]
            cand = [r for rset in rs for r in rset]
            hits = [i for i, r in enumerate(cand) if [r[0], r[1], r[2] - r[0] + 1, r[3] - r[1] + 1] == box]
            assert len(hits) == 1, (k, hits)
            max_idx.append(hits[0])
            chosen.append([float(x) for x in cand[hits[0]]])
            ious.append(iou)
            flags.append(iou > 0.5)
        assert pct == sum(flags) / Q * 100
        g[name + "_max_idx"], g[name + "_rect"] = np.array(max_idx), np.array(chosen, dtype=np.float64)
        g[name + "_iou"], g[name + "_correct"], g[name + "_percent"] = np.array(ious, dtype=np.float64), np.array(flags), np.array(pct, dtype=np.float64)
        print(name, "max_idx", max_idx, "iou", ["%.4f" % x for x in ious], "percent", pct)
    # the planted cases did what they were planted for
    z, f = g["zsl_max_idx"].tolist(), g["fsl_max_idx"].tolist()
    assert z[0] == f[0] == 1 and [float(x) for x in frac_rect] == g["zsl_rect"][0].tolist()
    fa, fb = fused_variants(frac_rect, anns["q0"]["bbox"])
    assert g["zsl_iou"][0] != fa and g["zsl_iou"][0] != fb, "q0 must tell a fused w1 * h1 + w2 * h2 from Python's two roundings"
    assert g["zsl_iou"][1] == 0.5 and not g["zsl_correct"][1] and z[1] == 1
    assert g["zsl_iou"][2] == 0.0 and z[2] == 0
    assert z[3] == f[3] == 0 and not g["zsl_correct"][3]                # the tie goes to the first sequence; the second would have been right
    assert z[4] == 0 and f[4] == 4 and g["zsl_iou"][4] != g["fsl_iou"][4]      # -1.5 / -0.5 = 3 beats 3 / 2
    assert z[5] == f[5] == 11 and z[6] == f[6] == 0 and g["zsl_correct"][6]
    assert 0 < g["zsl_percent"] < 100 and g["zsl_percent"] != g["fsl_percent"]
    g["fused_iou_q0"] = np.array([fa, fb], dtype=np.float64)
    path = os.path.join(OUT, "tiny_rec_eval.npz")
    np.savez_compressed(path, **g)
    meta = {
        "fixture": "tiny_rec_eval.npz",
        "written_by": "tools/make_golden_rec_eval.py",
        "ran_from_the_reference": [
            "oscar.zeroshot.refcoco_cpt.val, the whole function, once (zsl_* arrays)",
            "oscar.fewshot.refcoco_cpt.val, the whole function, once (fsl_* arrays)",
            "oscar.utils.iou.computeIoU, as val() calls it: the module's name is wrapped by a recorder that calls the real function and keeps its "
            "arguments and result (zsl_iou / fsl_iou are its return values, bit for bit; *_percent is val()'s return value)"],
        "stand_ins": ["the model (returns the planted row at every sequence's mask_token_pos)", "the data loader (batches in test_collate's layout, "
                      "dataset.anns_dic)", "the tokenizer (convert_tokens_to_ids on six colour words)", "the module-level logger val() expects",
                      "transformers.pytorch_transformers through oracle/ref_stub.py, tqdm"],
        "restated_here": [
            "max_idx and the chosen rectangle are not returned by val(): they are the one candidate of the query whose conversion "
            "[x1, y1, x2 - x1 + 1, y2 - y1 + 1] equals the box val() passed to computeIoU (every candidate of a query is distinct: asserted)",
            "correct = iou > 0.5, the comparison val() applies to the recorded iou; asserted to give val()'s percentage",
            "fused_iou_q0: computeIoU of query 0 with w1 * h1 + w2 * h2 rounded once (either product fused), by exact rational arithmetic -- what a "
            "contracted multiply-add would give; both differ from zsl_iou[0]"],
        "planted": {"q0": "fractional coordinates, contraction-sensitive", "q1": "IoU exactly 0.5: not correct", "q2": "touching boxes: intersection 0",
                    "q3": "exact tie between two sequences: the first wins", "q4": "negative none logit: few-shot chooses candidate 4, zero-shot 0",
                    "q5": "sequences of 5, 5 and 2 colours", "q6": "one sequence, one colour"},
        "queries": Q, "sequences": int(sum(n_seq)), "vocab": V, "batch_queries": BATCH,
    }
    with open(os.path.join(OUT, "tiny_rec_eval_META.json"), "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
