"""Score extraction and region selection and IoU accuracy.

Counterparts of /root/reference/Oscar/oscar/zeroshot/refcoco_cpt.py:219-254 (raw colour logits),
Oscar/oscar/fewshot/refcoco_cpt.py:277-295 (colour logit / "none" logit) and
Oscar/oscar/utils/iou.py:1-12.  Two forms.  Host-side (select_region, compute_iou, accuracy): the inputs
are the (B, V) [MASK]-row logits the HIP path returns; only B x n_colour values are touched, and
torch.argmax's first-max tie-break is kept.  On the device (rec_eval_table + rec_choose_device, what
drivers.val_rec runs): the selection, the float64 IoU and the accuracy counts of a batch in one launch
(cpt_rec_choose) against tables uploaded once per split; rec_eval_reference is its host yardstick.
"""
import numpy as np
import torch


def gather_color_scores(mask_scores, color_id_sets, none_id, divide_by_none=False):
    """mask_scores (P, V): one row per proposal sequence of ONE query; color_id_sets: per sequence
    the colour-token ids of its painted proposals.  Returns the concatenated score vector."""
    out = []
    for row, ids in zip(mask_scores, color_id_sets):
        cur = row[list(ids) + [none_id]]
        out.append(cur[0:-1] / cur[-1] if divide_by_none else cur[0:-1])
    return torch.cat(out, -1)


def select_region(mask_scores, color_id_sets, rect_sets, none_id, few_shot=False):
    """-> (max_idx, chosen rect, scores).  zeroshot/refcoco_cpt.py:224-246; few_shot=True uses the
    ratio to the "none" logit (fewshot/refcoco_cpt.py:291)."""
    scores = gather_color_scores(mask_scores, color_id_sets, none_id, divide_by_none=few_shot)
    rects = [r for rs in rect_sets for r in rs]
    idx = int(scores.argmax())
    return idx, rects[idx], scores


def compute_iou(box1, box2):
    """Boxes [x, y, w, h] with inclusive pixel extents (Oscar/oscar/utils/iou.py)."""
    ix1, iy1 = max(box1[0], box2[0]), max(box1[1], box2[1])
    ix2 = min(box1[0] + box1[2] - 1, box2[0] + box2[2] - 1)
    iy2 = min(box1[1] + box1[3] - 1, box2[1] + box2[3] - 1)
    inter = (ix2 - ix1 + 1) * (iy2 - iy1 + 1) if (ix1 < ix2 and iy1 < iy2) else 0
    return float(inter) / (box1[2] * box1[3] + box2[2] * box2[3] - inter)


def accuracy(predictions, gts, thresh=0.5):
    """predictions {key: [x1,y1,x2,y2]}, gts {key: [x,y,w,h]} -> percent with IoU > thresh
    (zeroshot/refcoco_cpt.py:267-280: predicted xyxy is converted with +1 extents)."""
    hit = 0
    for k, p in predictions.items():
        assert p[2] > p[0] and p[3] > p[1]
        q = [p[0], p[1], p[2] - p[0] + 1, p[3] - p[1] + 1]
        hit += compute_iou(q, gts[k]) > thresh
    return hit / max(len(predictions), 1) * 100


def nsp_choice_labels(labels, interval, n_seq, device=None):
    """fewshot/vcr_nsp_cpt.py:433-436: class 0 for the correct answer choice of each question, 1 elsewhere."""
    cls_labels = torch.ones([n_seq], dtype=torch.long, device=device)
    for i, lb in enumerate(labels):
        cls_labels[i * interval + int(lb)] = 0
    return cls_labels


def nsp_choose(rel_scores, interval):
    """fewshot/vcr_nsp_cpt.py:597-604: choice score = 1 - softmax(rel)[:, 1]; first-max argmax inside each
    question's `interval` answer choices.  Returns (scores (N,), [pred per question])."""
    logits = 1 - (rel_scores[:, :].softmax(-1)[:, 1].view(-1))
    n = rel_scores.size(0) // interval
    return logits, [int(logits[q * interval:(q + 1) * interval].argmax()) for q in range(n)]


def select_regions_device(mask_scores, color_id_sets, query_first, none_id, few_shot=False, return_scores=False):
    """Device-side region selection for a whole batch of queries (include/cpt_hip.h cpt_select_regions): the
    (S, V) [MASK]-row logits stay on the GPU and only one index per query comes back.
    mask_scores (S, V) CUDA fp32; color_id_sets: per sequence its colour-token ids; query_first: first sequence
    index of every query plus the total (len Q+1).  Same result as ``select_region`` per query
    (zeroshot/refcoco_cpt.py:224-246, fewshot/refcoco_cpt.py:277-295), torch.argmax tie-break included."""
    from . import _lib as L
    if not mask_scores.is_cuda:
        raise RuntimeError("cpt_amd: select_regions_device needs the logits on the GPU (no CPU fallback)")
    dev = mask_scores.device
    S, V = mask_scores.shape
    C = max(1, max((len(c) for c in color_id_sets), default=1))
    ids = torch.full((S, C), -1, dtype=torch.int64)
    for i, c in enumerate(color_id_sets):
        if len(c):
            ids[i, :len(c)] = torch.as_tensor(list(c), dtype=torch.int64)
    ids = ids.to(dev)
    qf = torch.as_tensor(list(query_first), dtype=torch.int32, device=dev)
    Q = qf.numel() - 1
    out = torch.empty(Q, dtype=torch.int64, device=dev)
    sc = torch.empty(Q, dtype=torch.float32, device=dev) if return_scores else None
    ms = mask_scores.contiguous()
    L.check(L.lib().cpt_select_regions(ms.data_ptr(), V, ids.data_ptr(), C, qf.data_ptr(), Q, int(none_id), 1 if few_shot else 0,
                                       out.data_ptr(), L.ptr(sc), L.stream_ptr()), "cpt_select_regions")
    return (out, sc) if return_scores else out


# ---- RefCOCO REC evaluation on the device (zeroshot/refcoco_cpt.py:224-246, 267-280; fewshot/refcoco_cpt.py:277-297, 305-315) ----------------
def rec_eval_table(queries, gts, none_id, col_ids=None, device=None):
    """val()'s bookkeeping as flat tables, once per split.  queries: the dicts drivers.val_queries takes (``colors``: per proposal sequence its
    colour-token ids, ``rects``: per sequence its x1, y1, x2, y2 rectangles); gts: per query its annotation [x, y, w, h] or None (a list, or a dict
    keyed by query index); col_ids: the vocabulary column list the scores are computed for (drivers' colour_columns_only) -- colour ids and
    none_id then become positions in it.  Raises ValueError, before anything runs, for a rectangle that breaks the reference's
    ``x2 > x1 and y2 > y1`` assert (any candidate may be the chosen one), for a sequence whose colour count differs from its rectangle count,
    and for a non-finite annotation.
    Returns a dict of CPU tensors -- seq_first (Q + 1,) int32, cols (S_total, C) int32 (-1 = trailing padding), cand_first (Q + 1,) int32,
    rects (R_total, 4) float64 in val()'s concatenation order, gt (Q, 4) float64, has_gt (Q,) uint8 -- plus n_queries, C, none (the "none"
    column), none_id, col_ids and n_cols_min (the columns the scores need at least).  device: upload now (rec_table_device); otherwise on first
    use."""
    col_of = None if col_ids is None else {int(c): i for i, c in enumerate(col_ids)}

    def column(c, what):
        if col_of is None:
            return int(c)
        if int(c) not in col_of:
            raise ValueError("cpt_amd: %s id %d is not in the column list" % (what, int(c)))
        return col_of[int(c)]

    none = column(none_id, '"none"')
    seq_first, cand_first, col_rows, rects = [0], [0], [], []
    for qi, q in enumerate(queries):
        if len(q["colors"]) != len(q["rects"]):
            raise ValueError("cpt_amd: query %d has %d colour sets and %d rectangle sets" % (qi, len(q["colors"]), len(q["rects"])))
        for si, (cs, rs) in enumerate(zip(q["colors"], q["rects"])):
            if len(cs) != len(rs):
                raise ValueError("cpt_amd: query %d sequence %d has %d colours and %d rectangles" % (qi, si, len(cs), len(rs)))
            for r in rs:
                if len(r) != 4 or not (r[2] > r[0] and r[3] > r[1]):
                    raise ValueError("cpt_amd: query %d sequence %d holds the degenerate rectangle %s (val() asserts x2 > x1 and y2 > y1)"
                                     % (qi, si, list(r)))
                rects.append([float(x) for x in r])
            col_rows.append([column(c, "colour") for c in cs])
        seq_first.append(len(col_rows))
        cand_first.append(len(rects))
    Q = len(queries)
    C = max(1, max((len(r) for r in col_rows), default=1))
    cols = torch.full((max(len(col_rows), 1), C), -1, dtype=torch.int32)[:len(col_rows)]
    for i, r in enumerate(col_rows):
        if r:
            cols[i, :len(r)] = torch.tensor(r, dtype=torch.int32)
    gt = torch.zeros((Q, 4), dtype=torch.float64)
    has_gt = torch.zeros(Q, dtype=torch.uint8)
    for qi in range(Q):
        g = gts.get(qi) if isinstance(gts, dict) else gts[qi]
        if g is None:
            continue
        g = [float(x) for x in g]
        if len(g) != 4 or not all(np.isfinite(g)):
            raise ValueError("cpt_amd: query %d has the annotation %s (four finite numbers x, y, w, h)" % (qi, g))
        gt[qi] = torch.tensor(g, dtype=torch.float64)
        has_gt[qi] = 1
    i32 = torch.int32
    table = {"seq_first": torch.tensor(seq_first, dtype=i32), "cols": cols.contiguous(), "cand_first": torch.tensor(cand_first, dtype=i32),
             "rects": torch.tensor(rects, dtype=torch.float64).view(-1, 4), "gt": gt, "has_gt": has_gt, "n_queries": Q, "C": C, "none": none,
             "none_id": int(none_id), "col_ids": None if col_ids is None else [int(c) for c in col_ids],
             "n_cols_min": max(none, int(cols.max()) if cols.numel() else 0) + 1, "_seq_first": seq_first}
    if device is not None:
        rec_table_device(table, device)
    return table


_REC_TABLE_KEYS = ("seq_first", "cols", "cand_first", "rects", "gt", "has_gt")


def rec_table_device(table, device):
    """The six tables of rec_eval_table on ``device``: packed into one byte buffer on the host (16-byte aligned pieces), ONE upload, typed
    views of it.  Cached in the table per device."""
    device = torch.device(device)
    dt = table.get("_dev")
    if dt is not None and dt[0] == device:
        return dt[1]
    offs, total = {}, 0
    for k in _REC_TABLE_KEYS:
        offs[k] = total
        total += (table[k].numel() * table[k].element_size() + 15) // 16 * 16
    host = torch.zeros(max(total, 16), dtype=torch.uint8)
    for k in _REC_TABLE_KEYS:
        b = table[k].contiguous().view(-1).view(torch.uint8)
        host[offs[k]:offs[k] + b.numel()] = b
    buf = host.to(device)
    views = {}
    for k in _REC_TABLE_KEYS:
        n = table[k].numel() * table[k].element_size()
        views[k] = buf[offs[k]:offs[k] + n].view(table[k].dtype).view(table[k].shape)
    views["_buffer"] = buf
    table["_dev"] = (device, views)
    return views


def rec_eval_buffers(table, device, candidate_scores=False):
    """The result buffers of one evaluation pass on the device, one slot per query of the split: idx int32 (-1), score fp32 (0), iou float64
    (NaN), correct uint8 (0), counts (2,) int32 = (correct, evaluated), zeroed, and cand_score (R_total,) fp32 (0) or None."""
    Q = table["n_queries"]
    return {"idx": torch.full((Q,), -1, dtype=torch.int32, device=device), "score": torch.zeros(Q, dtype=torch.float32, device=device),
            "iou": torch.full((Q,), float("nan"), dtype=torch.float64, device=device), "correct": torch.zeros(Q, dtype=torch.uint8, device=device),
            "counts": torch.zeros(2, dtype=torch.int32, device=device),
            "cand_score": torch.zeros(table["rects"].size(0), dtype=torch.float32, device=device) if candidate_scores else None}


def rec_choose_device(mask_scores, q_index, table, few_shot, out):
    """cpt_rec_choose, one launch: mask_scores (S_b, V') fp32 on the GPU, the head rows of the queries ``q_index`` (global indices in table
    order, any order, each once) one after the other; ``out`` the buffers of rec_eval_buffers, written at the queries' global indices and
    counted into out["counts"].  Only q_index is uploaded, nothing is read back.  The sizes are checked on the host against the table."""
    from . import _lib as L
    if not mask_scores.is_cuda:
        raise RuntimeError("cpt_amd: rec_choose_device needs the logits on the GPU (no CPU fallback: rec_eval_reference is the host form)")
    dev = mask_scores.device
    qi = [int(i) for i in q_index]
    Q = table["n_queries"]
    S, V = mask_scores.shape
    if not qi or min(qi) < 0 or max(qi) >= Q or len(set(qi)) != len(qi):
        raise ValueError("cpt_amd: rec_choose_device takes distinct query indices in [0, %d)" % Q)
    sf = table["_seq_first"]
    n_seq = sum(sf[i + 1] - sf[i] for i in qi)
    if n_seq != S or V < table["n_cols_min"] or mask_scores.dtype != torch.float32:
        raise ValueError("cpt_amd: rec_choose_device got %s %s scores; the %d queries hold %d sequences and read column %d"
                         % (tuple(mask_scores.shape), mask_scores.dtype, len(qi), n_seq, table["n_cols_min"] - 1))
    for k, dtype, n in (("idx", torch.int32, Q), ("score", torch.float32, Q), ("iou", torch.float64, Q), ("correct", torch.uint8, Q),
                        ("counts", torch.int32, 2), ("cand_score", torch.float32, table["rects"].size(0))):
        t = out[k]
        if t is None and k == "cand_score":
            continue
        if t.dtype != dtype or t.numel() != n or t.device != dev or not t.is_contiguous():
            raise ValueError("cpt_amd: rec_choose_device out[%r] must be a contiguous %s tensor of %d elements on %s" % (k, dtype, n, dev))
    t = rec_table_device(table, dev)
    qd = torch.tensor(qi, dtype=torch.int32).to(dev, non_blocking=True)
    ms = mask_scores.contiguous()
    L.check(L.lib().cpt_rec_choose(ms.data_ptr(), S, V, qd.data_ptr(), len(qi), Q, t["seq_first"].data_ptr(), t["cols"].data_ptr(), table["C"],
                                   t["cand_first"].data_ptr(), t["rects"].data_ptr(), t["gt"].data_ptr(), t["has_gt"].data_ptr(), table["none"],
                                   1 if few_shot else 0, out["idx"].data_ptr(), out["score"].data_ptr(), out["iou"].data_ptr(),
                                   out["correct"].data_ptr(), L.ptr(out["cand_score"]), out["counts"].data_ptr(), L.stream_ptr()), "cpt_rec_choose")
    return out


def rec_eval_reference(mask_scores, table, few_shot=False):
    """The host yardstick of cpt_rec_choose, no device call: the two val() post-loops (zeroshot/refcoco_cpt.py:224-246, 267-280;
    fewshot/refcoco_cpt.py:277-297, 305-315) and compute_iou restated literally in torch and Python floats.  mask_scores (S_total, V') CPU fp32:
    the head row of every sequence of the table, in order.  A query without a colour (the reference's torch.cat would raise) gets idx -1,
    score -inf; it and a query without an annotation (the reference's gts[k] would raise) get iou NaN and count in neither sum.
    Returns {"idx" (Q,) int32, "score" (Q,) fp32, "iou" (Q,) float64, "correct" (Q,) uint8, "cand_score" (R_total,) fp32 numpy arrays,
    "rects": per query the chosen x1, y1, x2, y2 or None, "counts": [correct, evaluated], "accuracy": percent}."""
    sf, cf = table["seq_first"].tolist(), table["cand_first"].tolist()
    cols, none = table["cols"].tolist(), table["none"]
    all_rects, gts, has_gt = table["rects"].tolist(), table["gt"].tolist(), table["has_gt"].tolist()
    Q = table["n_queries"]
    idx = np.full(Q, -1, dtype=np.int32)
    score = np.full(Q, -np.inf, dtype=np.float32)
    iou_out = np.full(Q, float("nan"), dtype=np.float64)
    flags = np.zeros(Q, dtype=np.uint8)
    cand_score = np.zeros(len(all_rects), dtype=np.float32)
    predictions = {}
    for q in range(Q):
        collected_rects = all_rects[cf[q]:cf[q + 1]]
        collected_scores = []
        for s in range(sf[q], sf[q + 1]):
            cur_color_id_set = [c for c in cols[s] if c >= 0] + [none]
            cur_color_scores = mask_scores[s][cur_color_id_set]
            collected_scores.append(cur_color_scores[0:-1] / cur_color_scores[-1] if few_shot else cur_color_scores[0:-1])
        if not collected_rects:
            continue
        collected_scores = torch.cat(collected_scores, -1)
        max_idx = collected_scores.argmax()
        predictions[q] = collected_rects[int(max_idx)]
        idx[q] = int(max_idx)
        score[q] = collected_scores[int(max_idx)].numpy()
        cand_score[cf[q]:cf[q + 1]] = collected_scores.numpy()
    miou, n = 0, 0
    for k, p in predictions.items():
        if not has_gt[k]:
            continue
        assert p[2] > p[0] and p[3] > p[1]
        p = [p[0], p[1], p[2] - p[0] + 1, p[3] - p[1] + 1]
        iou = compute_iou(p, gts[k])
        miou += iou > 0.5
        n += 1
        iou_out[k] = iou
        flags[k] = iou > 0.5
    return {"idx": idx, "score": score, "iou": iou_out, "correct": flags, "cand_score": cand_score,
            "rects": [predictions.get(q) for q in range(Q)], "counts": [int(miou), n], "accuracy": miou / max(n, 1) * 100}


def argmax_columns_device(scores, ids):
    """GQA answer scoring (gqa_cpt.py:598-601): argmax over the label-token columns, on the device."""
    from . import _lib as L
    if not scores.is_cuda:
        raise RuntimeError("cpt_amd: argmax_columns_device needs the logits on the GPU (no CPU fallback)")
    R, V = scores.shape
    idt = torch.as_tensor(ids, dtype=torch.int64, device=scores.device).contiguous()
    out = torch.empty(R, dtype=torch.int64, device=scores.device)
    sc = scores.contiguous()
    L.check(L.lib().cpt_argmax_columns(sc.data_ptr(), V, idt.data_ptr(), idt.numel(), R, out.data_ptr(), None, L.stream_ptr()),
            "cpt_argmax_columns")
    return out


# ---- VG-CPT predicate scoring (Oscar/oscar/fewshot/vg_cpt.py:255-290) ----------------------------------------------------------
# Every (subject, object) pair gives 6 sequences: "S is [MASK] x k a O" for k = 1, 2, 3, then the same with S and O swapped
# (datasets/vg_test_dataset.py), i.e. 1 + 2 + 3 head rows per direction, 12 per pair, in sequence order.  A predicate of n
# word-pieces is scored on the n-mask template as the mean log-probability (softmax over all V columns) of its pieces.
VG_MAX_PIECES = 3


def vg_candidates(idx2pred):
    """idx2pred {predicate index: [word-piece ids]} (vg_cpt.py:260-262) -> (cols, cand_cols (C, 3) int32, cand_len (C,) int32):
    cols = the sorted union of the word-piece ids (the decoder columns to compute), cand_cols[c][j] = position of piece j of
    predicate c in cols.  C = max index + 1; indices without a predicate (0: background) have length 0.  Raises on a predicate
    of more than 3 pieces (the reference would fail with an IndexError: there is no such template)."""
    for idx, pieces in idx2pred.items():
        if not 1 <= len(pieces) <= VG_MAX_PIECES:
            raise ValueError("cpt_amd: predicate %s has %d word-pieces; VG templates hold 1 to %d [MASK]s" % (idx, len(pieces), VG_MAX_PIECES))
    cols = sorted({int(t) for pieces in idx2pred.values() for t in pieces})
    where = {t: i for i, t in enumerate(cols)}
    C = max(int(i) for i in idx2pred) + 1
    cand_cols = torch.zeros((C, VG_MAX_PIECES), dtype=torch.int32)
    cand_len = torch.zeros(C, dtype=torch.int32)
    for idx, pieces in idx2pred.items():
        cand_len[int(idx)] = len(pieces)
        for j, t in enumerate(pieces):
            cand_cols[int(idx), j] = where[int(t)]
    return torch.tensor(cols, dtype=torch.int64), cand_cols, cand_len


def vg_slot_rows(n_pairs):
    """(2 * n_pairs, 3) int32: first head row of the k-mask template (column k - 1) of group g = 2 * pair + direction,
    for head rows laid out as 6 sequences per pair with k [MASK] rows each (k = 1, 2, 3; forward, then reversed)."""
    first = torch.tensor([0, 1, 3], dtype=torch.int32)
    g = torch.arange(2 * n_pairs, dtype=torch.int32)[:, None]
    return (g * 6 + first[None, :]).contiguous()


def vg_slot_rows_from(row_seq, n_seq):
    """slot_row (2 * n_seq / 6, 3) of an actual head-row list: row_seq (n,) the sequence of every head row, ascending.  Checks the
    VG layout -- sequence 6 i + 3 d + k - 1 holds exactly k rows (k = 1, 2, 3) -- and raises ValueError otherwise, so that rows are
    never scored against another template's slots."""
    seq = torch.as_tensor(row_seq).reshape(-1).cpu().long()
    if n_seq % 6:
        raise ValueError("cpt_amd: VG batches hold 6 sequences per pair (got %d sequences)" % n_seq)
    if seq.numel() and (bool((seq[1:] < seq[:-1]).any()) or int(seq.min()) < 0 or int(seq.max()) >= n_seq):
        raise ValueError("cpt_amd: head rows must be grouped by ascending sequence in [0, %d)" % n_seq)
    counts = torch.bincount(seq, minlength=n_seq)
    want = torch.arange(n_seq) % 3 + 1
    if not torch.equal(counts, want):
        bad = int((counts != want).nonzero()[0])
        raise ValueError("cpt_amd: sequence %d holds %d head rows; the VG layout gives sequence s exactly s %% 3 + 1" % (bad, int(counts[bad])))
    first = (torch.cumsum(counts, 0) - counts).to(torch.int32)
    return first.view(-1, 3).contiguous()


def mean_logprob_scores_device(logits, row_lse, slot_row, cand_cols, cand_len):
    """include/cpt_hip.h cpt_mean_logprob_scores, one launch: out[g][c] = mean over the len = cand_len[c] pieces of
    logits[s + j][cand_cols[c][j]] - row_lse[s + j], s = slot_row[g][len - 1]; 0 for len 0.  logits (n, n_cols) and row_lse (n,)
    fp32 on the GPU; the int tables are moved there.  Returns (G, C)."""
    from . import _lib as L
    if not logits.is_cuda:
        raise RuntimeError("cpt_amd: mean_logprob_scores_device needs the scores on the GPU (no CPU fallback)")
    dev = logits.device
    lg = logits.contiguous().float()
    ls = row_lse.contiguous().float()
    sr = slot_row.to(device=dev, dtype=torch.int32).contiguous()
    cc = cand_cols.to(device=dev, dtype=torch.int32).contiguous()
    cl = cand_len.to(device=dev, dtype=torch.int32).contiguous()
    G, K = sr.shape
    C = cl.numel()
    if cc.shape != (C, K):
        raise RuntimeError("cpt_amd: cand_cols shape %s != (%d, %d)" % (tuple(cc.shape), C, K))
    out = torch.empty((G, C), device=dev, dtype=torch.float32)
    L.check(L.lib().cpt_mean_logprob_scores(lg.data_ptr(), lg.size(1), lg.size(0), ls.data_ptr(), sr.data_ptr(), G, K, cc.data_ptr(),
                                            cl.data_ptr(), C, out.data_ptr(), L.stream_ptr()), "cpt_mean_logprob_scores")
    return out


def vg_val_scores_reference(seq_row_logits, idx2pred):
    """Torch restatement of val()'s scoring loop (vg_cpt.py:271-290) over FULL score rows: seq_row_logits is a list with one
    (k, V) tensor per sequence (6 per pair, in dataset order), the logits of its k [MASK] rows.  Returns (pairs, 2, C): per pair
    the forward and the reversed direction's scores (the values of predictions[im_key] and predictions[reverse_imkey(im_key)])."""
    C = max(int(i) for i in idx2pred) + 1
    scores = [x.float().softmax(-1) for x in seq_row_logits]
    n_pairs = len(scores) // 6
    out = torch.zeros((n_pairs, 2, C))
    for i in range(n_pairs):
        for d in range(2):
            cur = [None] + scores[i * 6 + 3 * d: i * 6 + 3 * d + 3]
            for idx, pred in idx2pred.items():
                prob_list = cur[len(pred)][torch.arange(len(pred)), torch.as_tensor(pred)]
                out[i, d, int(idx)] = torch.mean(torch.log(prob_list))
    return out


def vg_predicate_scores(model, input_ids, segment_ids, attention_mask, img_feats, mask_token_pos, idx2pred):
    """Device scoring of a batch of VG pairs (6 sequences each): mask_token_pos (n, 2) (sequence, position) of the 12 head rows per
    pair in sequence order.  forward_rows on the union of the predicate word-pieces (the full-vocabulary normaliser computed on the
    device), then cpt_mean_logprob_scores.  Returns (pairs, 2, C) on the GPU."""
    cols, cand_cols, cand_len = vg_candidates(idx2pred)
    dev = input_ids.device
    B = input_ids.size(0)
    slot_row = vg_slot_rows_from(mask_token_pos[:, 0], B)
    out = model._engine().forward_rows(input_ids, segment_ids, attention_mask, None, img_feats, row_seq=mask_token_pos[:, 0],
                                       mask_pos=mask_token_pos[:, 1], cols=cols.to(dev), lse=True, trim=model.trim_padding)
    n_pairs = B // 6
    sc = mean_logprob_scores_device(out["logits"], out["lse"], slot_row, cand_cols, cand_len)
    return sc.view(n_pairs, 2, -1)


# ---- VG Recall@K / mean Recall@K (Oscar/oscar/utils/vg_eval.py eval_vg) ----------------------------------------------------------
# Prediction keys are "<image>.jpg_<subject>_<object>" (vg_cpt.py:211-214); eval_vg groups them by image in dict order, adds an all-zero
# dummy row for every ground-truth image without one, ranks each image's pairs by the score of their best predicate (index >= 1), and
# counts a ground-truth triplet (s, o, r) as hit@K when (s, o, r) is among the top K.  The device form ranks once (cpt_vg_recall_ranks);
# hit@K = rank < K for every K, reduced in float64 on the device.
VG_MODES = (20, 50, 100)


def reverse_imkey(key):
    """vg_cpt.py:211-214: the key of the same image with subject and object swapped."""
    s, o = [int(x) for x in key.split("_")[-2:]]
    return key.split(".jpg")[0] + ".jpg" + "_" + str(o) + "_" + str(s)


def _imkey_split(key):
    return key.split(".jpg")[0] + ".jpg", [int(x) for x in key.split("_")[-2:]]


def vg_eval_table(keys, gts, n_slots=51):
    """eval_vg's bookkeeping as CSR tables, once per split.  keys: the prediction key of every score row, in the order the rows were
    written (predictions[k] = v: a repeated key keeps its first position and takes the LAST row); gts: the ground-truth list of eval_vg
    (dicts with "img_path" and "relations" (n, 3) = subject, object, predicate).  Images come in ground-truth order; an image without a
    prediction gets the reference's dummy candidate (pair (0, 0), all-zero row: relation 1 at score 0).  Raises ValueError where
    eval_vg fails: a predicted image absent from the ground truth, an image without ground-truth relations, a predicate >= n_slots
    (and, refused outright, a negative predicate or a repeated ground-truth image).
    Returns a dict of int32 CPU tensors: cand_off (n_img + 1), cand (n_cand, 3) = (s, o, row; -1 = dummy), gt_off (n_img + 1),
    gt (n_gt, 3), gt_img (n_gt,), plus images, n_rows = len(keys), n_slots."""
    where = {}
    for i, k in enumerate(keys):
        where[k] = i                                   # dict assignment: first position, last value
    by_img = {}
    for k, row in where.items():
        img, pair = _imkey_split(k)
        by_img.setdefault(img, []).append((pair[0], pair[1], row))
    images = [str(g["img_path"]) for g in gts]
    if len(set(images)) != len(images):
        raise ValueError("cpt_amd: the ground truth lists an image twice (eval_vg's length assert fails)")
    known = set(images)
    extra = [img for img in by_img if img not in known]
    if extra:
        raise ValueError("cpt_amd: predicted image %r is absent from the ground truth (eval_vg's length assert fails)" % extra[0])
    cand_off, cand, gt_off, gt, gt_img = [0], [], [0], [], []
    for gi, g in enumerate(gts):
        img = images[gi]
        cand += by_img.get(img, [(0, 0, -1)])
        cand_off.append(len(cand))
        rel = torch.as_tensor(g["relations"]).long().reshape(-1, 3)
        if rel.size(0) == 0:
            raise ValueError("cpt_amd: image %r has no ground-truth relation (eval_vg divides 0 by 0.0)" % img)
        if int(rel[:, 2].max()) >= n_slots or int(rel[:, 2].min()) < 0:
            raise ValueError("cpt_amd: image %r has a ground-truth predicate outside [0, %d)" % (img, n_slots))
        gt.append(rel)
        gt_img += [gi] * rel.size(0)
        gt_off.append(gt_off[-1] + rel.size(0))
    i32 = torch.int32
    return {"cand_off": torch.tensor(cand_off, dtype=i32), "cand": torch.tensor(cand, dtype=i32).view(-1, 3),
            "gt_off": torch.tensor(gt_off, dtype=i32), "gt": torch.cat(gt).to(i32), "gt_img": torch.tensor(gt_img, dtype=torch.int64),
            "images": images, "n_rows": len(keys), "n_slots": int(n_slots)}


def vg_recall_ranks_device(scores, table):
    """cpt_vg_recall_ranks, one launch: scores (n_rows, C) or (pairs, 2, C) on the GPU, rows in the order of vg_eval_table's keys.
    Returns (n_gt,) int32 ranks on the device: INT32_MAX where the triplet is not predicted, hit@K = rank < K."""
    from . import _lib as L
    if not scores.is_cuda:
        raise RuntimeError("cpt_amd: vg_recall_ranks_device needs the scores on the GPU (no CPU fallback)")
    dev = scores.device
    sc = scores.reshape(-1, scores.size(-1)).contiguous().float()
    if sc.size(0) != table["n_rows"]:
        raise ValueError("cpt_amd: %d score rows for %d prediction keys" % (sc.size(0), table["n_rows"]))
    dt = table.get("_dev")
    if dt is None or dt[0] != dev:
        ws_bytes = int(L.lib().cpt_vg_recall_workspace_bytes(table["cand_off"].data_ptr(), len(table["images"])))
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        dt = (dev, {k: table[k].to(dev).contiguous() for k in ("cand_off", "cand", "gt_off", "gt", "gt_img")}, ws, ws_bytes)
        table["_dev"] = dt
    _, t, ws, ws_bytes = dt
    n_gt = t["gt"].size(0)
    out = torch.empty(n_gt, dtype=torch.int32, device=dev)
    L.check(L.lib().cpt_vg_recall_ranks(sc.data_ptr(), sc.size(0), sc.size(1), t["cand_off"].data_ptr(), t["cand"].data_ptr(), t["cand"].size(0),
                                        t["gt_off"].data_ptr(), t["gt"].data_ptr(), n_gt, len(table["images"]), out.data_ptr(),
                                        ws.data_ptr() if ws_bytes else None, ws_bytes, L.stream_ptr()), "cpt_vg_recall_ranks")
    return out


def vg_recall_from_ranks(ranks, table, modes=VG_MODES):
    """R@K and mR@K from per-triplet ranks, in float64 torch on the ranks' device.  R@K: mean over images of hits / |gt|.  mR@K: mean over
    predicates 1..n_slots-1 of the mean over images holding the predicate of that image's recall of it (0 for a predicate never seen;
    the reference's range(51) makes n_slots = 51 divide by 50 whatever the vocabulary)."""
    dev = ranks.device
    n_img, S = len(table["images"]), table["n_slots"]
    gimg = table["gt_img"].to(dev)
    rel = table["gt"][:, 2].to(device=dev, dtype=torch.int64)
    cell = gimg * S + rel
    f64 = torch.float64
    n_per_img = torch.zeros(n_img, dtype=f64, device=dev).index_add_(0, gimg, torch.ones_like(gimg, dtype=f64))
    cnt = torch.zeros(n_img * S, dtype=f64, device=dev).index_add_(0, cell, torch.ones_like(cell, dtype=f64)).view(n_img, S)
    seen = cnt > 0
    n_seen = seen.sum(0).to(f64)
    recall, mrecall = {}, {}
    for K in modes:
        hit = (ranks.long() < K).to(f64)
        per_img = torch.zeros(n_img, dtype=f64, device=dev).index_add_(0, gimg, hit) / n_per_img
        recall[K] = per_img.mean()
        hc = torch.zeros(n_img * S, dtype=f64, device=dev).index_add_(0, cell, hit).view(n_img, S)
        ratio = torch.where(seen, hc / cnt.clamp_min(1), torch.zeros_like(hc)).sum(0)
        per_pred = torch.where(n_seen > 0, ratio / n_seen.clamp_min(1), torch.zeros_like(ratio))
        mrecall[K] = per_pred[1:].mean()
    return {"recall": {K: float(v) for K, v in recall.items()}, "mrecall": {K: float(v) for K, v in mrecall.items()}}


def vg_recall_device(scores, table, modes=VG_MODES):
    """Recall@K and mean Recall@K of a split on the device: cpt_vg_recall_ranks, then the float64 reductions.  Only the 2 x len(modes)
    results leave the GPU.  Returns {"recall": {K: R@K}, "mrecall": {K: mR@K}, "ranks": (n_gt,) int32 on the device}."""
    ranks = vg_recall_ranks_device(scores, table)
    out = vg_recall_from_ranks(ranks, table, modes)
    out["ranks"] = ranks
    return out


def format_vg_recall(result):
    """The two-line string eval_vg returns (R@20/50/100, then mR@20/50/100)."""
    r, m = result["recall"], result["mrecall"]
    rst = "R@20: {:.4f}\tR@50: {:.4f}\tR@100: {:.4f}".format(r[20], r[50], r[100]) + "\n"
    rst += "mR@20: {:.4f}\tmR@50: {:.4f}\tmR@100: {:.4f}".format(m[20], m[50], m[100]) + "\n"
    return rst


def eval_vg_reference(predictions, gts, modes=VG_MODES, n_slots=51):
    """Torch restatement of eval_vg on the host, no device call: predictions {key: (C,) scores} in dict order, gts as vg_eval_table.  The
    image loop, argmax over predicates 1.., descending sort (stable: ties keep candidate order, NaN first), top-K matching, and the
    per-predicate means, written as the reference writes them but in float64.  Returns {"recall", "mrecall", "ranks" (n_gt,) int64
    (INT32_MAX = not predicted; triplets in ground-truth order), "string"}."""
    new_preds = {}
    for k, v in predictions.items():
        img, pair = _imkey_split(k)
        new_preds.setdefault(img, []).append((pair, v))
    C = next(iter(predictions.values())).numel() if predictions else n_slots
    for g in gts:
        if g["img_path"] not in new_preds:
            new_preds[g["img_path"]] = [([0, 0], torch.zeros(C, dtype=torch.float))]
    gts = [g for g in gts if g["img_path"] in new_preds]
    if len(new_preds) != len(gts):
        raise ValueError("cpt_amd: %d predicted images, %d ground-truth images" % (len(new_preds), len(gts)))
    big = 2 ** 31 - 1
    recall = {K: [] for K in modes}
    mrecall = {K: [[] for _ in range(n_slots)] for K in modes}
    all_ranks = []
    for g in gts:
        p_list = new_preds[g["img_path"]]
        pairs = torch.tensor([p for p, _ in p_list], dtype=torch.int64)
        prds = torch.stack([v.float().cpu() for _, v in p_list], 0)
        rels = prds[:, 1:].argmax(1) + 1
        scores = prds[torch.arange(len(prds)), rels]
        idxs = torch.sort(scores, descending=True, stable=True).indices
        trip = torch.cat([pairs[idxs], rels[idxs][:, None]], -1)
        gt_rels = torch.as_tensor(g["relations"]).long().reshape(-1, 3)
        if gt_rels.size(0) == 0:
            raise ValueError("cpt_amd: image %r has no ground-truth relation" % g["img_path"])
        eq = (gt_rels[:, None, :] == trip[None, :, :]).all(2)                  # (n_gt, n_cand) in rank order
        first = torch.where(eq.any(1), eq.float().argmax(1), torch.full((gt_rels.size(0),), big, dtype=torch.int64))
        all_ranks.append(first)
        for K in modes:
            rcl = first < K
            recall[K].append(float(rcl.sum()) / float(len(gt_rels)))
            tot, hit = {}, {}
            for r, c in zip(gt_rels[:, 2].tolist(), rcl.tolist()):
                tot[r] = tot.get(r, 0) + 1
                hit[r] = hit.get(r, 0) + int(c)
            for r in hit:
                mrecall[K][r].append(hit[r] / tot[r])
    out = {"recall": {K: float(np.mean(v)) for K, v in recall.items()},
           "mrecall": {K: float(np.mean([np.mean(v) if len(v) > 0 else 0 for v in vl[1:]])) for K, vl in mrecall.items()},
           "ranks": torch.cat(all_ranks) if all_ranks else torch.zeros(0, dtype=torch.int64)}
    if set(VG_MODES) <= set(modes):
        out["string"] = format_vg_recall(out)
    return out


# ---- VCR Q->AR (Oscar/oscar/fewshot/vcr_qar_nsp_cpt.py) ----------------------------------------------------------------------------------
def qar_choice_labels(ans_labels, rat_labels, n_ans, n_rats, device=None):
    """vcr_qar_nsp_cpt.py:462-472: class 0 at i * n_ans + ans_label of the Q->A block and at i * n_rats + rat_label of the QA->R block, 1 at every
    other sequence.  Returns (q_a_cls_labels (n_q * n_ans,), qa_r_cls_labels (n_q * n_rats,)) int64."""
    return nsp_choice_labels(ans_labels, n_ans, len(ans_labels) * n_ans, device), nsp_choice_labels(rat_labels, n_rats, len(rat_labels) * n_rats, device)


def choice_scores(rel):
    """evaluate()'s choice score (vcr_qar_nsp_cpt.py:641,650): 1 - softmax(rel)[:, 1]."""
    return 1 - (rel[:, :].softmax(-1)[:, 1].view(-1))


def vcr_qar_choose_reference(q_a_logits, qa_r_logits, ans_labels, rat_labels, n_ans, n_rats, q_ids=None):
    """Host restatement of evaluate()'s per-question loop (vcr_qar_nsp_cpt.py:657-676) on the choice scores: the answer argmax, the rationale
    argmax over all n_rats scores -- or, when n_rats > n_ans (16 rationales), over the slice [ans_label * n_ans, (ans_label + 1) * n_ans) of
    them, block width n_ans as written, with the GROUND-TRUTH answer --, correct = both right.  Returns the result dicts the reference
    pickles: questionId, answer [a, r], correct, gt [ans_label, rat_label], logits [q_a slice, qa_r slice]."""
    out = []
    n_q = len(ans_labels)
    for n in range(n_q):
        q_a_pred_logits = q_a_logits[n * n_ans:(n + 1) * n_ans]
        q_a_pred = q_a_pred_logits.argmax()
        ans_label = int(ans_labels[n])
        if n_rats > n_ans:
            qa_r_pred_logits = qa_r_logits[n * n_rats:(n + 1) * n_rats][ans_label * n_ans:(ans_label + 1) * n_ans]
        else:
            qa_r_pred_logits = qa_r_logits[n * n_rats:(n + 1) * n_rats]
        qa_r_pred = qa_r_pred_logits.argmax()
        rat_label = int(rat_labels[n])
        out.append({"questionId": int(q_ids[n]) if q_ids is not None else n, "answer": [int(q_a_pred), int(qa_r_pred)],
                    "correct": bool((ans_label == int(q_a_pred)) & (rat_label == int(qa_r_pred))), "gt": [ans_label, rat_label],
                    "logits": [q_a_pred_logits.cpu().numpy(), qa_r_pred_logits.cpu().numpy()]})
    return out


def vcr_qar_choose_device(q_a_scores, qa_r_scores, ans_labels, rat_labels, n_ans, n_rats, counts=None):
    """The same choice on the device, one launch (cpt_vcr_qar_choose): q_a_scores (n_q * n_ans,), qa_r_scores (n_q * n_rats,) fp32 device
    tensors, labels (n_q,).  Returns (preds (n_q, 2) int64, flags (n_q, 3) uint8 = Q->A, QA->R, Q->AR correct); ``counts`` (3,) int32 device
    tensor, optional: += the column sums of flags."""
    from . import _lib as L
    dev = q_a_scores.device
    n_q = len(ans_labels)
    qa = q_a_scores.contiguous().float()
    qr = qa_r_scores.contiguous().float()
    if qa.numel() != n_q * n_ans or qr.numel() != n_q * n_rats:
        raise ValueError("vcr_qar_choose_device: %d / %d scores for %d questions of %d answers and %d rationales"
                         % (qa.numel(), qr.numel(), n_q, n_ans, n_rats))
    al = torch.as_tensor(ans_labels, dtype=torch.int64).to(dev).contiguous()
    rl = torch.as_tensor(rat_labels, dtype=torch.int64).to(dev).contiguous()
    preds = torch.empty((n_q, 2), dtype=torch.int64, device=dev)
    flags = torch.empty((n_q, 3), dtype=torch.uint8, device=dev)
    if counts is not None and (counts.dtype != torch.int32 or counts.numel() != 3 or not counts.is_contiguous()):
        raise ValueError("vcr_qar_choose_device: counts must be a contiguous (3,) int32 tensor")
    L.check(L.lib().cpt_vcr_qar_choose(qa.data_ptr(), qr.data_ptr(), n_q, n_ans, n_rats, al.data_ptr(), rl.data_ptr(), preds.data_ptr(),
                                       flags.data_ptr(), L.ptr(counts), L.stream_ptr()), "cpt_vcr_qar_choose")
    return preds, flags


def vcr_qar_accuracy(results, n_examples):
    """vcr_qar_nsp_cpt.py:682-685: results de-duplicated by questionId (a dict: the LAST entry wins), acc = correct / len(eval_dataset)."""
    dic = {r["questionId"]: r for r in results}
    return sum([x["correct"] for x in dic.values()]) / n_examples


# ---- GQA-CPT (Oscar/oscar/fewshot/gqa_cpt.py evaluate(), :558-636) ------------------------------------------------------------------------
def gqa_first_pieces(labels, tokenizer):
    """gqa_cpt.py:566-568: per answer label its first word-piece -- (label_token_ids [its vocabulary id], answer_labels [the piece as a string])."""
    pieces = [tokenizer.tokenize(lb) for lb in labels]
    return [tokenizer.convert_tokens_to_ids(p)[0] for p in pieces], [p[0] for p in pieces]


def gqa_string_ids(labels, tokenizer):
    """The strings evaluate() compares (gqa_cpt.py:604-611) as integer ids, quirk kept: the PREDICTED string is the first word-piece of the chosen
    label (answer_labels[p]), the ground-truth strings are the WHOLE labels (labels[x]).  Returns (label_token_ids, label_sid, piece_sid), lists
    of len(labels): label_token_ids as gqa_first_pieces; label_sid[i] = one id per distinct label string (the index of its first occurrence);
    piece_sid[i] = the id of the label string equal to label i's first piece, -2 when no label is that string (the prediction is then never
    right)."""
    token_ids, answer_labels = gqa_first_pieces(labels, tokenizer)
    sid = {}
    for i, lb in enumerate(labels):
        sid.setdefault(lb, i)
    return token_ids, [sid[lb] for lb in labels], [sid.get(p, -2) for p in answer_labels]


def gqa_choose_reference(logits, labels, answer_labels, igts, q_ids=None):
    """Host restatement of evaluate()'s per-batch loop (gqa_cpt.py:600-612), no device call: logits (R, C) the label-order columns of the [MASK]
    rows, answer_labels the first-piece strings, igts per question its ground-truth label indices (eval_dic[str(qid)]).  Returns the result dicts
    the reference pickles: answer, question_id, gt, igt, correct, logits."""
    preds = logits.argmax(1)
    preds = [answer_labels[int(p)] for p in preds]
    out = []
    for i, (p, igt) in enumerate(zip(preds, igts)):
        gt = [labels[int(x)] for x in igt]
        correct = [x == p for x in gt]
        correct = max(correct)
        out.append({"answer": p, "question_id": int(q_ids[i]) if q_ids is not None else i, "gt": gt, "igt": list(igt), "correct": correct,
                    "logits": logits[i].cpu().numpy()})
    return out


def gqa_accuracy(results, n_examples):
    """gqa_cpt.py:619-620: results de-duplicated by question_id (a dict: the LAST entry wins), acc = correct / len(eval_dataset)."""
    dic = {r["question_id"]: r for r in results}
    return sum([x["correct"] for x in dic.values()]) / n_examples


def gqa_gt_table(igts, label_sid):
    """(R, G) int32 string ids of every question's ground-truth labels, padded with -1 (G = the longest list, at least 1)."""
    G = max(1, max((len(x) for x in igts), default=1))
    t = torch.full((len(igts), G), -1, dtype=torch.int32)
    for i, x in enumerate(igts):
        if len(x):
            t[i, :len(x)] = torch.tensor([label_sid[int(j)] for j in x], dtype=torch.int32)
    return t


def gqa_choose_device(scores, piece_sid, gt_sid, counts=None):
    """The same choice on the device, one launch (cpt_gqa_choose): scores (R, C) fp32 on the GPU, piece_sid (C,) and gt_sid (R, G) int32 (moved
    to the device when they are not there).  Returns (pred (R,) int64 = the argmax column, correct (R,) uint8); ``counts`` (1,) int32 device
    tensor, optional: += the number of correct rows."""
    from . import _lib as L
    if not scores.is_cuda:
        raise RuntimeError("cpt_amd: gqa_choose_device needs the logits on the GPU (no CPU fallback: gqa_choose_reference is the host form)")
    dev = scores.device
    sc = scores.contiguous().float()
    R, C = sc.shape
    ps = torch.as_tensor(piece_sid, dtype=torch.int32).to(dev).contiguous()
    gt = torch.as_tensor(gt_sid, dtype=torch.int32).to(dev).contiguous()
    if ps.numel() != C or gt.dim() != 2 or gt.size(0) != R:
        raise ValueError("gqa_choose_device: scores %s, piece_sid %s, gt_sid %s" % (tuple(sc.shape), tuple(ps.shape), tuple(gt.shape)))
    if counts is not None and (counts.dtype != torch.int32 or counts.numel() != 1 or not counts.is_cuda):
        raise ValueError("gqa_choose_device: counts must be a (1,) int32 device tensor")
    pred = torch.empty(R, dtype=torch.int64, device=dev)
    correct = torch.empty(R, dtype=torch.uint8, device=dev)
    L.check(L.lib().cpt_gqa_choose(sc.data_ptr(), R, C, ps.data_ptr(), gt.data_ptr(), gt.size(1), pred.data_ptr(), correct.data_ptr(), L.ptr(counts),
                                   L.stream_ptr()), "cpt_gqa_choose")
    return pred, correct


# ---- VCR Q->A (Oscar/oscar/fewshot/vcr_nsp_cpt.py evaluate(), :583-620) ---------------------------------------------------------------------
def nsp_choose_device(rel, interval, labels, counts=None):
    """nsp_choose on the device, one launch (cpt_nsp_choose): rel (N, n_rel) fp32 relation scores on the GPU, labels (N / interval,) the
    questions' answer labels.  Returns (scores (N,) = 1 - softmax(rel)[:, 1], preds (n_q,) int64, flags (n_q,) uint8 = pred == label);
    ``counts`` (1,) int32 device tensor, optional: += the number of correct questions.  N % interval != 0 raises (CPT_ERR_SHAPE)."""
    from . import _lib as L
    if not rel.is_cuda:
        raise RuntimeError("cpt_amd: nsp_choose_device needs the relation scores on the GPU (no CPU fallback: nsp_choose is the host form)")
    dev = rel.device
    x = rel.contiguous().float()
    N, n_rel = x.shape
    interval = int(interval)
    n_q = N // interval if interval > 0 else 0
    lb = torch.as_tensor(labels, dtype=torch.int64).to(dev).contiguous()
    if interval > 0 and N % interval == 0 and lb.numel() != n_q:
        raise ValueError("nsp_choose_device: %d labels for %d questions" % (lb.numel(), n_q))
    if counts is not None and (counts.dtype != torch.int32 or counts.numel() != 1 or not counts.is_cuda):
        raise ValueError("nsp_choose_device: counts must be a (1,) int32 device tensor")
    scores = torch.empty(N, dtype=torch.float32, device=dev)
    preds = torch.empty(n_q, dtype=torch.int64, device=dev)
    flags = torch.empty(n_q, dtype=torch.uint8, device=dev)
    L.check(L.lib().cpt_nsp_choose(x.data_ptr(), N, n_rel, interval, lb.data_ptr(), scores.data_ptr(), preds.data_ptr(), flags.data_ptr(),
                                   L.ptr(counts), L.stream_ptr()), "cpt_nsp_choose")
    return scores, preds, flags


def nsp_accuracy(results, n_examples):
    """vcr_nsp_cpt.py:619-620: results de-duplicated by questionId (the LAST entry wins), acc = correct / len(eval_dataset)."""
    dic = {r["questionId"]: r for r in results}
    return sum([x["correct"] for x in dic.values()]) / n_examples
