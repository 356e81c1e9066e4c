"""Device-resident evaluation sets: a split uploaded ONCE, each step's padded (or trimmed) batch gathered from it by one launch.

The evaluation loops are bound by the host: every step concatenates its items on the host and pushes the region features over PCIe, and the
few-shot protocol walks the same splits again and again.  Here a split becomes packed tables -- host side first (``tables``: numpy, no GPU),
then ``upload`` lays them into device memory -- and ``ResidentSet.gather`` builds what ``batching.trim(torch.cat(...))`` holds on the host with
cpt_gather_batch (include/cpt_hip.h), from a device list of sequence indices.  A pass uploads nothing but that list.

Layout.  The items (RefCOCO queries: ``from_queries``; GQA questions: ``from_questions``) become one flat list of sequences, item i owning
[seq_first[i], seq_first[i + 1]).  Per sequence: its padded text row (ids int32, segment ids uint8), its mask row (uint8), its [MASK] position
and ``feat_block``, the block that holds its region features.  A block is one (Li, D) array: a (Li, D) array expanded over the sequences of an
item is ONE block, and items that hand in the same array (same data pointer, shape, strides and dtype) share their blocks.  Only the rows up to
the last one with any non-zero BIT are stored (``block_rows``; -0.0 is not zero, a zero row in front of a non-zero one stays); the gather writes
the rows behind as +0.0, which is what they held.

Head tables.  The sets above hold ONE [MASK] position per sequence.  VG pairs (``from_pairs``), VCR questions (``from_vcr``, ``from_vcr_qar``) and
the few-shot training batches (``from_train_batches``) carry head tables beside it: per sequence its head rows (0, 1 or several positions in the
padded sequence, ``head_first`` / ``head_pos``), a label per head row (``head_label``, -1 = ignored) and a label per sequence (``seq_label``, the
relation heads).  cpt_gather_batch_heads writes, in the same single launch, the (n, 2) (sequence, position) head rows, their labels, the
(B, Lt' + Li') label grid of the MLM training loops and the sequence labels; ``row_first``, the prefix sum of the head counts of a batch, comes
from the host tables and goes up with the index lists.

Exactness.  The gathered batch equals the host batch element for element (features by their bits), and the forward is unchanged and repeats bit
for bit on equal inputs: a resident pass returns the host pass's results, not results inside a tolerance.  A bf16 store halves the memory and
the gather's read; it is exact only where the forward itself rounds the features to bf16 first (compute dtype "bf16"; rounding twice is
rounding once), so every other compute dtype refuses it (``ResidentSet.check_model``).
"""
import collections

import numpy as np

from . import batching
from . import dist as cdist

CHUNK_BYTES = 64 << 20          # features go up in chunks of at most this many fp32 bytes (one staging buffer of that size)
_ESIZE = {"fp32": 4, "bf16": 2}
HEAD_TABLES = ("head_first", "head_pos", "head_label", "seq_label")                 # cpt_resident_heads
HEAD_OUTPUTS = ("head_rows", "head_labels", "label_grid", "seq_label")              # the four outputs of cpt_gather_batch_heads
H2D = {"calls": collections.Counter(), "bytes": collections.Counter()}        # what h2d() moved, by name


def _np(x):
    """An array or a CPU tensor as an array (a tensor's memory is shared, not copied)."""
    if isinstance(x, np.ndarray):
        return x
    if hasattr(x, "detach"):
        x = x.detach()
        if str(x.dtype) == "torch.bfloat16":
            x = x.float()
        return x.numpy()
    return np.asarray(x)


def _key(x):
    """What makes two feature arrays the same array: data pointer, shape, strides and dtype."""
    if hasattr(x, "data_ptr"):
        return (x.data_ptr(), tuple(x.shape), tuple(x.stride()), str(x.dtype))
    a = np.asarray(x)
    return (a.__array_interface__["data"][0], a.shape, a.strides, a.dtype.str)


def _items(rows, heads=None, seq_labels=None, whole=False):
    n = len(rows)
    seq_first = np.zeros(n + 1, np.int64)
    for i, r in enumerate(rows):
        seq_first[i + 1] = seq_first[i] + r[0].shape[0]
    items = {"n_items": n, "seq_first": seq_first, "ids": [r[0] for r in rows], "seg": [r[1] for r in rows], "mask": [r[2] for r in rows],
             "mask_pos": [r[3] for r in rows], "feats": [r[4] for r in rows]}
    if heads is not None:               # per item (sequence, position, label or None) of its head rows, the sequence local to the item
        items["heads"] = heads
        items["seq_labels"] = seq_labels
        items["whole"] = whole          # (training sets: every rank stores the set it built, upload does not shard it)
    return items


def from_queries(queries):
    """RefCOCO queries (the layout drivers.val_queries takes: ``img_feats (P, Li, D)``, ``input_ids (P, Lt)``, ``segment_ids``,
    ``attention_mask (P, Lt + Li)``, ``mask_token_pos (P,)``) as items: one flat list of sequences plus ``seq_first``."""
    rows = []
    for q in queries:
        ids = _np(q["input_ids"])
        if ids.ndim != 2:
            raise ValueError("resident: a query's input_ids is (P, Lt), got %s" % (ids.shape,))
        rows.append((ids, _np(q["segment_ids"]), _np(q["attention_mask"]), _np(q["mask_token_pos"]).reshape(-1), q.get("img_feats")))
    return _items(rows)


def from_questions(questions):
    """GQA questions (prompts.assemble_gqa dicts: 1-D ``input_ids``, ``segment_ids``, ``input_mask``, ``img_feats (Li, D)``, and
    ``mask_token_pos`` whose first entry is the [MASK] position) as items of one sequence each."""
    rows = []
    for q in questions:
        ids = _np(q["input_ids"])
        if ids.ndim != 1:
            raise ValueError("resident: a question's input_ids is 1-D, got %s" % (ids.shape,))
        rows.append((ids[None], _np(q["segment_ids"])[None], _np(q["input_mask"])[None],
                     np.asarray([int(_np(q["mask_token_pos"]).reshape(-1)[0])], np.int64), q.get("img_feats")))
    return _items(rows)


def _head_rows(pos, n_seq, labels=None):
    """Head rows of one item as (sequence, position, labels or None): ``pos`` is (P,) -- one row per sequence, in order -- or (n, 2)
    (sequence, position) rows, which are brought into sequence order (stable)."""
    pos = _np(pos)
    if pos.dtype.kind not in "iu":
        raise ValueError("resident: mask_token_pos must be integers, got %s" % pos.dtype)
    pos = pos.astype(np.int64)
    if pos.ndim == 2 and pos.shape[1] == 2:
        seq, p = pos[:, 0], pos[:, 1]
    elif pos.reshape(-1).shape[0] == n_seq:
        seq, p = np.arange(n_seq, dtype=np.int64), pos.reshape(-1)
    else:
        raise ValueError("resident: mask_token_pos is (P,) or (n, 2), got %s for %d sequences" % (pos.shape, n_seq))
    if seq.size and (int(seq.min()) < 0 or int(seq.max()) >= n_seq):
        raise ValueError("resident: a head row names sequence %d of %d" % (int(seq.max() if seq.max() >= n_seq else seq.min()), n_seq))
    lab = None
    if labels is not None:
        lab = _np(labels).reshape(-1)
        if lab.dtype.kind not in "iu" or lab.shape[0] != seq.shape[0]:
            raise ValueError("resident: %d integer labels are needed for %d head rows, got %s %s" % (seq.shape[0], seq.shape[0], lab.dtype, lab.shape))
        lab = lab.astype(np.int64)
    order = np.argsort(seq, kind="stable")
    return seq[order], p[order], None if lab is None else lab[order]


def from_pairs(pairs):
    """VG pairs (prompts.assemble_vg_zsl / assemble_vg_train rows with ``img_feats`` (Li, D) or (P, Li, D), the layout drivers.val_vg takes) as
    items of 6 or 3 sequences.  ``mask_token_pos`` (n, 2) (sequence, position) gives the head rows -- in sequence order, as the prompts write
    them and scoring.vg_predicate_scores reads them -- and ``row_labels`` (n,), when present, their labels."""
    rows, heads = [], []
    for q in pairs:
        ids = _np(q["input_ids"])
        if ids.ndim != 2:
            raise ValueError("resident: a pair's input_ids is (P, Lt), got %s" % (ids.shape,))
        mask = _np(q["attention_mask"] if "attention_mask" in q else q["input_mask"])
        pos = _np(q["mask_token_pos"])
        if pos.ndim != 2 or pos.shape[1] != 2 or (pos.shape[0] > 1 and bool((np.diff(pos[:, 0]) < 0).any())):
            raise ValueError("resident: a pair's mask_token_pos is (n, 2) (sequence, position) rows in sequence order, got %s" % (pos.shape,))
        heads.append(_head_rows(pos, ids.shape[0], q.get("row_labels")))
        rows.append((ids, _np(q["segment_ids"]), mask, np.zeros(ids.shape[0], np.int64), q.get("img_feats")))
    if len({h[2] is None for h in heads}) > 1:
        raise ValueError("resident: either every pair carries row_labels or none does")
    return _items(rows, heads, None)


def _vcr_label(q):
    lb = q["label"]
    return int(lb[0] if isinstance(lb, (list, tuple)) else lb)


def from_vcr(questions, labels=True):
    """VCR Q->A questions (prompts.assemble_vcr dicts with ``img_feats`` (Li, D)) as items of one sequence per answer choice.  No head rows: the
    relation head reads [CLS].  labels: each sequence carries its class of scoring.nsp_choice_labels -- 0 for the question's correct choice, 1
    elsewhere -- as ``seq_label``."""
    rows, heads, slab = [], [], []
    for q in questions:
        ids = _np(q["input_ids"])
        if ids.ndim != 2:
            raise ValueError("resident: a VCR question's input_ids is (choices, Lt), got %s" % (ids.shape,))
        P = ids.shape[0]
        rows.append((ids, _np(q["segment_ids"]), _np(q["input_mask"]), np.zeros(P, np.int64), q.get("img_feats")))
        heads.append(_head_rows(np.zeros((0, 2), np.int64), P))
        if labels:
            lab = np.ones(P, np.int64)
            lab[_vcr_label(q)] = 0
            slab.append(lab)
    return _items(rows, heads, slab if labels else None)


def from_vcr_qar(questions, labels=True):
    """VCR Q->AR questions (prompts.assemble_vcr_qar dicts with ``img_feats`` (Li, D)) as items of n_ans + n_rats sequences, the Q->A block
    first.  A batch lists all Q->A sequences of its questions, then all QA->R sequences (``qar_order``): the layout drivers._qar_blocks builds
    and qar_forward runs.  labels: ``seq_label`` as scoring.qar_choice_labels gives it, per block."""
    rows, heads, slab = [], [], []
    for q in questions:
        a, r = q["q_a"], q["qa_r"]
        ids = np.concatenate([_np(a["input_ids"]), _np(r["input_ids"])], 0)
        n_ans, n_rats = _np(a["input_ids"]).shape[0], _np(r["input_ids"]).shape[0]
        if (n_ans, n_rats) != (q["n_ans"], q["n_rats"]):
            raise ValueError("resident: a Q->AR question holds %d + %d sequences and says %d + %d" % (n_ans, n_rats, q["n_ans"], q["n_rats"]))
        rows.append((ids, np.concatenate([_np(a["segment_ids"]), _np(r["segment_ids"])], 0),
                     np.concatenate([_np(a["input_mask"]), _np(r["input_mask"])], 0), np.zeros(ids.shape[0], np.int64), q.get("img_feats")))
        heads.append(_head_rows(np.zeros((0, 2), np.int64), ids.shape[0]))
        if labels:
            lab = np.ones(n_ans + n_rats, np.int64)
            lab[int(q["label"][0])] = 0
            lab[n_ans + int(q["label"][1])] = 0
            slab.append(lab)
    items = _items(rows, heads, slab if labels else None)
    items["n_ans"] = [int(q["n_ans"]) for q in questions]
    return items


def qar_order(seq_first, n_ans, group):
    """The index list of a Q->AR batch of the items ``group``: all Q->A sequences of the chunk, then all QA->R sequences."""
    qa = [np.arange(seq_first[i], seq_first[i] + n_ans) for i in group]
    qr = [np.arange(seq_first[i] + n_ans, seq_first[i + 1]) for i in group]
    return np.concatenate(qa + qr)


def from_train_batches(batches, labels=None):
    """Few-shot training batches as items, one per batch dict: the dicts drivers.train_batch / tune_soft_template take (``mask_token_pos`` (B,),
    ``colors`` (B,)) or the ones drivers.train_vg_batch takes (``mask_token_pos`` (n, 2), ``row_labels`` (n,)), each with ``input_ids``,
    ``segment_ids``, ``attention_mask`` and ``img_feats`` (B, Li, D).  labels: the key that holds the labels (default: ``colors`` for (B,)
    positions, ``row_labels`` for (n, 2) rows).  A negative position counts from the end of the padded sequence, as the index assignment of
    drivers._label_grid takes it.  The set is not sharded: every rank uploads the batches it trains on."""
    rows, heads = [], []
    for b in batches:
        ids = _np(b["input_ids"])
        if ids.ndim != 2:
            raise ValueError("resident: a training batch's input_ids is (B, Lt), got %s" % (ids.shape,))
        mask = _np(b["attention_mask"])
        pos = _np(b["mask_token_pos"])
        key = labels if labels is not None else ("row_labels" if pos.ndim == 2 else "colors")
        seq, p, lab = _head_rows(pos, ids.shape[0], b[key])
        p = np.where(p < 0, p + mask.shape[-1], p)
        first = np.zeros(ids.shape[0], np.int64)              # (mask_pos: the sequence's first head row, 0 without one)
        first[seq[::-1]] = p[::-1]
        rows.append((ids, _np(b["segment_ids"]), mask, first, b.get("img_feats")))
        heads.append((seq, p, lab))
    return _items(rows, heads, None, whole=True)


def _as_int(a, lo, hi, what):
    a = np.asarray(a)
    if a.dtype.kind not in "iub":
        raise ValueError("resident: %s must be integers, got %s" % (what, a.dtype))
    if a.size and (int(a.min()) < lo or int(a.max()) > hi):
        raise ValueError("resident: %s outside [%d, %d]" % (what, lo, hi))
    return a


def block_rows_of(block):
    """1 + the last row of a (Li, D) fp32 block that has any non-zero bit, 0 if there is none."""
    bits = np.ascontiguousarray(block, dtype=np.float32).view(np.uint32)
    live = np.flatnonzero((bits != 0).any(axis=1)) if bits.shape[1] else np.zeros(0, np.int64)
    return int(live[-1]) + 1 if live.size else 0


def tables(items, shard=None):
    """The host tables of the items [lo, hi) = ``shard`` (default: all) -- numpy only, nothing is uploaded.  Sequence indices stay GLOBAL:
    ``seq_first`` covers every item, the per-sequence arrays hold the sequences [seq_base, seq_base + n_seq) of the shard.
    Per sequence: ``text_len`` / ``regions`` (batching.extents of its mask row), ``mask_pos`` int32, ``feat_block`` int32, and the packed rows
    ``ids`` int32 (S, Lt), ``seg`` uint8 (S, Lt), ``mask`` uint8 (S, Lt + Li).  Per block: ``block_rows``, ``block_off`` (its first row in
    ``feats``, the concatenated fp32 rows that are kept).  Raises ValueError for a mask entry outside {0, 1}, an id or [MASK] position outside
    int32, a segment id outside uint8, and items whose Lt, Li or D differ."""
    n = items["n_items"]
    lo, hi = (0, n) if shard is None else (int(shard[0]), int(shard[1]))
    if not 0 <= lo <= hi <= n:
        raise ValueError("resident: shard [%d, %d) of %d items" % (lo, hi, n))
    seq_first = np.asarray(items["seq_first"], np.int64)
    Lt = Li = D = None
    ids, seg, mask, mpos, fblock = [], [], [], [], []
    blocks, seen = [], {}
    with_heads = items.get("heads") is not None
    hcount, hpos, hlab, slab = [], [], [], []
    for i in range(lo, hi):
        a, s, m, p, f = items["ids"][i], items["seg"][i], items["mask"][i], items["mask_pos"][i], items["feats"][i]
        P = a.shape[0]
        shape = (a.shape[1], m.shape[-1] - a.shape[1])
        if Lt is None:
            Lt, Li = shape
        if shape != (Lt, Li) or shape[1] < 0 or Lt < 1 or s.shape != a.shape or m.shape != (P, Lt + Li) or p.shape != (P,):
            raise ValueError("resident: item %d is padded %d + %d (segment ids %s, mask %s, positions %s), the set %d + %d"
                             % (i, shape[0], shape[1], s.shape, m.shape, p.shape, Lt, Li))
        ids.append(_as_int(a, -2 ** 31, 2 ** 31 - 1, "input_ids").astype(np.int32))
        seg.append(_as_int(s, 0, 255, "segment_ids").astype(np.uint8))
        mask.append(_as_int(m, 0, 1, "attention_mask entries").astype(np.uint8))
        mpos.append(_as_int(p, -2 ** 31, 2 ** 31 - 1, "mask_token_pos").astype(np.int32))
        if with_heads:
            hs, hp, hl = items["heads"][i]
            if hp.size and (int(hp.min()) < 0 or int(hp.max()) >= Lt + Li):
                raise ValueError("resident: item %d has a head row at position %d, outside the padded sequence of %d + %d"
                                 % (i, int(hp.max() if hp.max() >= Lt + Li else hp.min()), Lt, Li))
            if np.unique(hs * (Lt + Li) + hp).size != hp.size:
                raise ValueError("resident: item %d has two head rows of one sequence at the same position" % i)
            hcount.append(np.bincount(hs, minlength=P).astype(np.int64))
            hpos.append(hp.astype(np.int32))
            if hl is not None:
                hlab.append(_as_int(hl, -2 ** 31, 2 ** 31 - 1, "head row labels").astype(np.int32))
            if items.get("seq_labels") is not None:
                sl = np.asarray(items["seq_labels"][i])
                if sl.shape != (P,):
                    raise ValueError("resident: item %d has %s sequence labels for %d sequences" % (i, sl.shape, P))
                slab.append(_as_int(sl, -2 ** 31, 2 ** 31 - 1, "sequence labels").astype(np.int32))
        if f is None:
            if Li:
                raise ValueError("resident: item %d has %d region positions and no img_feats" % (i, Li))
            fblock.append(np.zeros(P, np.int32))
            continue
        key = _key(f)
        if key not in seen:
            arr = _np(f)
            if arr.ndim not in (2, 3) or arr.shape[-2] != Li or (arr.ndim == 3 and arr.shape[0] != P):
                raise ValueError("resident: item %d has img_feats %s for %d sequences of %d regions" % (i, arr.shape, P, Li))
            if D is None:
                D = arr.shape[-1]
            if arr.shape[-1] != D:
                raise ValueError("resident: item %d has img_feats of dimension %d, the set %d" % (i, arr.shape[-1], D))
            one = arr.ndim == 2 or arr.strides[0] == 0           # (Li, D), or that expanded over the sequences: ONE block
            arr = np.asarray(arr[0] if one and arr.ndim == 3 else arr, dtype=np.float32)
            seen[key] = (len(blocks), one, P)
            blocks.extend([arr] if one else list(arr))
        base, one, P0 = seen[key]
        if not one and P0 != P:
            raise ValueError("resident: item %d shares img_feats of %d sequences but has %d" % (i, P0, P))
        fblock.append(np.full(P, base, np.int32) if one else base + np.arange(P, dtype=np.int32))
    if Lt is None:                      # an empty shard: the shape from the first item, if there is one
        Lt, Li = (items["ids"][0].shape[1], items["mask"][0].shape[-1] - items["ids"][0].shape[1]) if n else (1, 0)
    D = 0 if D is None else D
    cat = lambda xs, shape, dt: np.concatenate(xs, 0) if xs else np.zeros(shape, dt)
    t = {"n_items": n, "seq_first": seq_first, "item_lo": lo, "item_hi": hi, "seq_base": int(seq_first[lo]),
         "n_seq": int(seq_first[hi] - seq_first[lo]), "Lt": int(Lt), "Li": int(Li), "D": int(D),
         "ids": cat(ids, (0, Lt), np.int32), "seg": cat(seg, (0, Lt), np.uint8), "mask": cat(mask, (0, Lt + Li), np.uint8),
         "mask_pos": cat(mpos, (0,), np.int32), "feat_block": cat(fblock, (0,), np.int32)}
    if t["ids"].shape[0] != t["n_seq"]:
        raise ValueError("resident: seq_first counts %d sequences in the shard, the items hold %d" % (t["n_seq"], t["ids"].shape[0]))
    t["text_len"], t["regions"] = batching.extents(t["mask"], Lt) if t["n_seq"] else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    rows = np.asarray([block_rows_of(b) for b in blocks], np.int32).reshape(-1)
    t["block_rows"] = rows
    t["block_off"] = (np.cumsum(rows, dtype=np.int64) - rows).astype(np.int64)
    t["feats"] = cat([np.ascontiguousarray(b[:r], dtype=np.float32) for b, r in zip(blocks, rows) if r], (0, D), np.float32)
    if with_heads:
        counts = cat(hcount, (0,), np.int64)
        if int(counts.sum()) > 2 ** 31 - 1:
            raise ValueError("resident: %d head rows do not fit int32" % int(counts.sum()))
        t["head_first"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        t["head_pos"] = cat(hpos, (0,), np.int32)
        t["n_heads"] = int(t["head_pos"].shape[0])
        labelled = [h[2] is not None for h in items["heads"]]
        if any(labelled) and not all(labelled):
            raise ValueError("resident: either every item carries head row labels or none does")
        labelled = any(labelled)
        t["head_label"] = cat(hlab, (0,), np.int32) if labelled else None
        t["seq_label"] = cat(slab, (0,), np.int32) if items.get("seq_labels") is not None else None
        t["whole"] = bool(items.get("whole"))
        if items.get("n_ans") is not None:
            t["n_ans"] = list(items["n_ans"])
    return t


def has_heads(t):
    return t.get("head_first") is not None


def row_first(t, seq_idx):
    """[B + 1] int32: the exclusive prefix sum of the head counts of the sequences ``seq_idx`` (global indices); its last entry is R."""
    idx = _local(t, seq_idx)
    hf = t["head_first"].astype(np.int64)
    return np.concatenate([[0], np.cumsum(hf[idx + 1] - hf[idx])]).astype(np.int32)


def _head_entries(t, idx):
    """(batch entry, table entry) of every head row of the batch of the store-local sequences ``idx``, in row order."""
    hf = t["head_first"].astype(np.int64)
    cnt = hf[idx + 1] - hf[idx]
    b = np.repeat(np.arange(idx.size, dtype=np.int64), cnt)
    first = np.cumsum(cnt) - cnt
    return b, hf[idx][b] + (np.arange(int(cnt.sum()), dtype=np.int64) - first[b])


def _local(t, seq_idx):
    idx = np.asarray(seq_idx, np.int64).reshape(-1) - t["seq_base"]
    if idx.size == 0 or int(idx.min()) < 0 or int(idx.max()) >= t["n_seq"]:
        raise ValueError("resident: sequence indices outside the stored [%d, %d) (or none)" % (t["seq_base"], t["seq_base"] + t["n_seq"]))
    return idx


def extent(t, seq_idx, head=True, labelled=False):
    """(Lt', Li') of the batch of the sequences ``seq_idx`` (global indices) from the per-sequence lengths: what
    batching.batch_extent(mask, Lt, mask_pos) gives on the concatenated batch (head=False: without the [MASK] positions).  A set with head
    tables counts the positions of its head rows -- all of them, or (labelled: the rule of batching.label_extent, for the training loops) those
    whose label is not -1; a set without head rows (the relation heads) gives the extent of the mask alone.  Host tables only: no device work,
    no synchronisation."""
    idx = _local(t, seq_idx)
    Lt, Li = t["Lt"], t["Li"]
    lt, li = max(1, int(t["text_len"][idx].max())), int(t["regions"][idx].max())
    if head:
        if has_heads(t):
            h = _head_entries(t, idx)[1]
            if labelled and t["head_label"] is not None:
                h = h[t["head_label"][h] != -1]
            p = t["head_pos"][h].astype(np.int64)
        else:
            p = t["mask_pos"][idx].astype(np.int64)
        text = (p >= 0) & (p < Lt)
        if text.any():
            lt = max(lt, int(p[text].max()) + 1)
        if p.size and not text.all():                  # a region position keeps the text whole; one outside the sequence keeps both parts whole
            lt = Lt
            rest = p[~text]
            inside = (rest >= Lt) & (rest < Lt + Li)
            li = Li if not inside.all() else max(li, int(rest.max()) - Lt + 1)
    return lt, li


def gather_reference(t, seq_idx, Lt_out, Li_out):
    """The numpy restatement of cpt_gather_batch: the batch of the sequences ``seq_idx`` (global indices) cut to (Lt_out, Li_out), as
    batching.trim of the concatenated host batch holds it -- ``input_ids`` / ``segment_ids`` (B, Lt_out) int64, ``attention_mask``
    (B, Lt_out + Li_out) int64, ``mask_token_pos`` (B,) int64, ``img_feats`` (B, Li_out, D) fp32.  Tables with head tables give what
    cpt_gather_batch_heads writes too, as the host path builds it: ``head_rows`` (R, 2) int64 (batch row, position), and where the set has the
    labels ``head_labels`` (R,), ``label_grid`` (B, Lt_out + Li_out) (drivers._label_grid / vg_label_grid, cut by batching.trim_grid) and
    ``seq_label`` (B,)."""
    idx = _local(t, seq_idx)
    Lt, Li, D = t["Lt"], t["Li"], t["D"]
    if not (1 <= Lt_out <= Lt and 0 <= Li_out <= Li):
        raise ValueError("resident: (%d, %d) does not fit the padded (%d, %d)" % (Lt_out, Li_out, Lt, Li))
    feats = np.zeros((idx.size, Li_out, D), np.float32)
    if Li_out:
        for b, blk in enumerate(t["feat_block"][idx].tolist()):
            r, o = min(int(t["block_rows"][blk]), Li_out), int(t["block_off"][blk])
            feats[b, :r] = t["feats"][o:o + r]
    out = {"input_ids": t["ids"][idx, :Lt_out].astype(np.int64), "segment_ids": t["seg"][idx, :Lt_out].astype(np.int64),
           "attention_mask": np.concatenate([t["mask"][idx, :Lt_out], t["mask"][idx, Lt:Lt + Li_out]], 1).astype(np.int64),
           "mask_token_pos": t["mask_pos"][idx].astype(np.int64), "img_feats": feats}
    if has_heads(t):            # cpt_gather_batch_heads: the head rows, their labels, the label grid and the sequence labels
        b, h = _head_entries(t, idx)
        out["head_rows"] = np.stack([b, t["head_pos"][h].astype(np.int64)], 1)
        if t["head_label"] is not None:
            out["head_labels"] = t["head_label"][h].astype(np.int64)
            grid = np.full((idx.size, Lt + Li), -1, np.int64)
            grid[b, out["head_rows"][:, 1]] = out["head_labels"]
            out["label_grid"] = np.concatenate([grid[:, :Lt_out], grid[:, Lt:Lt + Li_out]], 1)
        if t["seq_label"] is not None:
            out["seq_label"] = t["seq_label"][idx].astype(np.int64)
    return out


def item_keys(t):
    """The bucket key of every stored item: text_len + regions of its longest sequence (drivers._item_length, without a mask scan)."""
    total = t["text_len"] + t["regions"]
    first = t["seq_first"][t["item_lo"]:t["item_hi"] + 1] - t["seq_base"]
    return [int(total[a:b].max()) if b > a else 0 for a, b in zip(first[:-1].tolist(), first[1:].tolist())]


def pitch_of(D, feature_dtype):
    """Elements per stored feature row: D rounded up to 16 bytes, so that every stored row starts 16-byte aligned."""
    per = 16 // _ESIZE[feature_dtype]
    return (D + per - 1) // per * per


def store_bytes(t, feature_dtype="fp32"):
    """Device bytes of the tables ``t`` as a store of ``feature_dtype`` (the staging buffer of the upload not counted)."""
    if feature_dtype not in _ESIZE:
        raise ValueError("resident: feature_dtype must be 'fp32' or 'bf16'")
    small = sum(t[k].nbytes for k in ("ids", "seg", "mask", "mask_pos", "feat_block", "block_rows", "block_off"))
    small += sum(t[k].nbytes for k in HEAD_TABLES if t.get(k) is not None)
    return small + t["feats"].shape[0] * pitch_of(t["D"], feature_dtype) * _ESIZE[feature_dtype]


def h2d(array, device, what):
    """The one place a host array of this module (and of the resident paths of the drivers) goes to the device; counted by name in H2D."""
    import torch
    host = torch.as_tensor(array)
    H2D["calls"][what] += 1
    H2D["bytes"][what] += host.numel() * host.element_size()
    return host.to(device, non_blocking=True)


class ResidentSet(object):
    """An evaluation set on the device (``upload``).  ``tables`` keeps the small host tables (the features are dropped after the upload)."""

    def __init__(self, t, device, feature_dtype, dev, store, heads=None):
        self.tables, self.device, self.feature_dtype = t, device, feature_dtype
        self._dev, self._store, self._heads = dev, store, heads
        self.n_items, self.n_sequences = t["n_items"], int(t["seq_first"][-1])
        self.seq_first, self.item_lo, self.item_hi = t["seq_first"], t["item_lo"], t["item_hi"]
        self.Lt, self.Li, self.D = t["Lt"], t["Li"], t["D"]
        self.nbytes = sum(v.numel() * v.element_size() for v in dev.values())

    def free(self):
        """Drop the device tables; the set cannot gather afterwards."""
        self._dev, self._store, self._heads, self.nbytes = None, None, None, 0

    def batch_indices(self):
        """The grouping the set was built from: per stored item the global indices of its sequences (a training set: one list per batch)."""
        sf = self.seq_first
        return [np.arange(sf[i], sf[i + 1]) for i in range(self.item_lo, self.item_hi)]

    def check_items(self, n_items, n_sequences, lo, hi, what):
        if self._store is None:
            raise RuntimeError("%s: the resident set was freed" % what)
        if n_items != self.n_items or n_sequences != self.n_sequences:
            raise ValueError("%s: the resident set holds %d items of %d sequences, the pass %d of %d: it was built from other items"
                             % (what, self.n_items, self.n_sequences, n_items, n_sequences))
        if (lo, hi) != (self.item_lo, self.item_hi):
            raise ValueError("%s: this rank's shard is [%d, %d), the resident set stores [%d, %d)" % (what, lo, hi, self.item_lo, self.item_hi))

    def check_model(self, model, what):
        """A bf16 store is exact only where the forward rounds the features to bf16 itself."""
        mode = model._engine().dtype
        if self.feature_dtype == "bf16" and mode != "bf16":
            raise ValueError("%s: a bf16 feature store is exact only in compute dtype 'bf16' (the forward then rounds the features to bf16 "
                             "itself); this model runs in %r -- upload the set with feature_dtype='fp32'" % (what, mode))

    def gather(self, seq_idx, Lt_out, Li_out, mask_pos=True, out=None, row_first=None, R=0, heads=None):
        """One cpt_gather_batch on the current stream.  seq_idx: int32 device tensor of GLOBAL sequence indices (the caller validates them).
        Returns ``input_ids`` / ``segment_ids`` (B, Lt_out), ``attention_mask`` (B, Lt_out + Li_out), ``mask_token_pos`` (B,) (None without
        mask_pos) -- int64 -- and ``img_feats`` (B, Li_out, D) fp32.  out: a dict of those tensors to write into (contiguous, on the device, of
        exactly these shapes) instead of fresh ones; every element is written.
        heads: names out of HEAD_OUTPUTS -- ``head_rows`` (R, 2), ``head_labels`` (R,), ``label_grid`` (B, Lt_out + Li_out), ``seq_label`` (B,),
        int64 -- to write as well, by ONE cpt_gather_batch_heads instead (a set with head tables; () runs that launch with none of the four).
        row_first: the (B + 1,) int32 device tensor of resident.row_first for this batch and R its last entry, for the two row outputs."""
        import torch
        from . import _lib as L
        if self._store is None:
            raise RuntimeError("resident: the set was freed")
        if seq_idx.dtype != torch.int32 or not seq_idx.is_cuda or seq_idx.dim() != 1 or not seq_idx.is_contiguous():
            raise ValueError("resident: seq_idx must be a contiguous 1-D int32 tensor on the GPU")
        B, dev = seq_idx.numel(), seq_idx.device
        shapes = {"input_ids": (B, Lt_out), "segment_ids": (B, Lt_out), "attention_mask": (B, Lt_out + Li_out), "mask_token_pos": (B,),
                  "img_feats": (B, Li_out, self.D)}
        optional = {"mask_token_pos"}
        if heads is not None:
            heads = tuple(heads)
            if self._heads is None:
                raise ValueError("resident: this set has no head tables (from_pairs, from_vcr, from_vcr_qar and from_train_batches build them)")
            if any(k not in HEAD_OUTPUTS for k in heads):
                raise ValueError("resident: heads are names out of %s, got %s" % (HEAD_OUTPUTS, heads))
            R = int(R)
            if "head_rows" in heads or "head_labels" in heads:
                if row_first is None or row_first.dtype != torch.int32 or row_first.device != dev or row_first.dim() != 1 \
                        or row_first.numel() != B + 1 or not row_first.is_contiguous() or R < 0:
                    raise ValueError("resident: the head rows need row_first, a contiguous (B + 1,) int32 tensor on the GPU, and R >= 0")
            shapes.update({"head_rows": (R, 2), "head_labels": (R,), "label_grid": (B, Lt_out + Li_out), "seq_label": (B,)})
            optional |= set(HEAD_OUTPUTS)
        if out is None:
            out = {k: torch.empty(shape, dtype=torch.float32 if k == "img_feats" else torch.int64, device=dev) for k, shape in shapes.items()
                   if k not in HEAD_OUTPUTS or k in heads}
        else:
            for k, shape in shapes.items():
                v = out.get(k)
                if k in HEAD_OUTPUTS and k not in heads:
                    continue
                if v is None and k == "mask_token_pos":
                    continue
                if v is None or tuple(v.shape) != shape or v.dtype != (torch.float32 if k == "img_feats" else torch.int64) or v.device != dev \
                        or not v.is_contiguous():
                    raise ValueError("resident: out[%r] must be a contiguous %s tensor on %s" % (k, shape, dev))
            out = {k: v for k, v in out.items() if k not in HEAD_OUTPUTS or (heads is not None and k in heads)}
        if not mask_pos:
            out["mask_token_pos"] = None
        if heads is None:
            L.check(L.lib().cpt_gather_batch(self._store, seq_idx.data_ptr(), B, Lt_out, Li_out, out["input_ids"].data_ptr(),
                                             out["segment_ids"].data_ptr(), out["attention_mask"].data_ptr(), L.ptr(out.get("mask_token_pos")),
                                             out["img_feats"].data_ptr() if Li_out else None, L.stream_ptr()), "cpt_gather_batch")
            return out
        hp = lambda k: out[k].data_ptr() if k in heads and out[k].numel() else None
        L.check(L.lib().cpt_gather_batch_heads(self._store, self._heads, seq_idx.data_ptr(), L.ptr(row_first), B, R, Lt_out, Li_out,
                                               out["input_ids"].data_ptr(), out["segment_ids"].data_ptr(), out["attention_mask"].data_ptr(),
                                               L.ptr(out.get("mask_token_pos")), out["img_feats"].data_ptr() if Li_out else None,
                                               hp("head_rows"), hp("head_labels"), hp("label_grid"), hp("seq_label"), L.stream_ptr()),
                "cpt_gather_batch_heads")
        return out


def upload(items_or_tables, device, feature_dtype="fp32", max_bytes=None):
    """Items (``from_queries`` / ``from_questions`` / ``from_pairs`` / ``from_vcr`` / ``from_vcr_qar`` / ``from_train_batches``) or host tables (``tables``) -> ResidentSet on ``device``.  Items are cut to this rank's
    dist.shard_range first (data parallel: a rank stores its own items only; the indices stay global).  The features go up in chunks of at
    most CHUNK_BYTES and cpt_pad_cast lays each chunk into the store: rows padded to a pitch of D rounded up to 16 bytes, cast to fp32 or
    bf16 (``feature_dtype``).  max_bytes (default: half of the free device memory now): a set that needs more raises before anything is
    uploaded."""
    import torch
    from . import _lib as L
    if feature_dtype not in _ESIZE:
        raise ValueError("resident: feature_dtype must be 'fp32' or 'bf16'")
    t = items_or_tables
    if "block_rows" not in t:
        rank, world = cdist.rank_world()
        t = tables(t, None if t.get("whole") else cdist.shard_range(t["n_items"], rank, world))
    device = torch.device(device)
    need = store_bytes(t, feature_dtype)
    if max_bytes is None:
        max_bytes = torch.cuda.mem_get_info(device)[0] // 2
    if need > max_bytes:
        raise ValueError("resident: the set needs %d bytes (%.2f GB) with %s features, the limit is %d%s"
                         % (need, need / 1e9, feature_dtype, max_bytes,
                            "" if feature_dtype == "bf16" else "; feature_dtype='bf16' needs %d and is exact in compute dtype 'bf16'" % store_bytes(t, "bf16")))
    dev = {k: h2d(t[k], device, "tables") for k in ("ids", "seg", "mask", "mask_pos", "feat_block", "block_rows", "block_off")}
    R, D, esz = t["feats"].shape[0], t["D"], _ESIZE[feature_dtype]
    pitch = pitch_of(D, feature_dtype)
    dev["feats"] = torch.empty((R, pitch), dtype=torch.float32 if esz == 4 else torch.bfloat16, device=device)
    if R and D:
        rows = max(1, CHUNK_BYTES // (4 * D))
        with torch.cuda.device(device):
            for r0 in range(0, R, rows):
                stage = h2d(t["feats"][r0:r0 + rows], device, "features")
                L.check(L.lib().cpt_pad_cast(stage.data_ptr(), dev["feats"].data_ptr() + r0 * pitch * esz, L.CPT_F32 if esz == 4 else L.CPT_BF16,
                                             stage.size(0), D, pitch, L.stream_ptr()), "cpt_pad_cast(resident features)")
                del stage       # (freed in stream order: the next chunk's copy is queued behind this chunk's launch)
    store = L.ResidentStore(feats=L.ptr(dev["feats"]) if R else None, ids=dev["ids"].data_ptr(), seg=dev["seg"].data_ptr(), mask=dev["mask"].data_ptr(),
                            mask_pos=dev["mask_pos"].data_ptr(), feat_block=dev["feat_block"].data_ptr(),
                            block_rows=L.ptr(dev["block_rows"]) if len(t["block_rows"]) else None,
                            block_off=L.ptr(dev["block_off"]) if len(t["block_rows"]) else None, n_rows=R,
                            feat_dtype=L.CPT_F32 if esz == 4 else L.CPT_BF16, pitch=pitch, img_dim=D, Lt=t["Lt"], Li=t["Li"], n_seq=t["n_seq"],
                            seq_base=t["seq_base"], n_blocks=len(t["block_rows"]))
    heads = None
    if has_heads(t):
        for k in HEAD_TABLES:
            if t[k] is not None:
                dev[k] = h2d(t[k], device, "tables")
        heads = L.ResidentHeads(head_first=dev["head_first"].data_ptr(), head_pos=L.ptr(dev["head_pos"]) if t["n_heads"] else None,
                                head_label=L.ptr(dev["head_label"]) if t["head_label"] is not None and t["n_heads"] else None,
                                seq_label=L.ptr(dev.get("seq_label")), n_heads=t["n_heads"])
    small = {k: v for k, v in t.items() if k != "feats"}
    return ResidentSet(small, device, feature_dtype, dev, store, heads)
