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


def _items(rows):
    n = len(rows)
    seq_first = np.zeros(n + 1, np.int64)
    for i, r in enumerate(rows):
        seq_first[i + 1] = seq_first[i] + r[0].shape[0]
    return {"n_items": n, "seq_first": seq_first, "ids": [r[0] for r in rows], "seg": [r[1] for r in rows], "mask": [r[2] for r in rows],
            "mask_pos": [r[3] for r in rows], "feats": [r[4] for r in rows]}


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
    return t


def _local(t, seq_idx):
    idx = np.asarray(seq_idx, np.int64).reshape(-1) - t["seq_base"]
    if idx.size == 0 or int(idx.min()) < 0 or int(idx.max()) >= t["n_seq"]:
        raise ValueError("resident: sequence indices outside the stored [%d, %d) (or none)" % (t["seq_base"], t["seq_base"] + t["n_seq"]))
    return idx


def extent(t, seq_idx, head=True):
    """(Lt', Li') of the batch of the sequences ``seq_idx`` (global indices) from the per-sequence lengths: what
    batching.batch_extent(mask, Lt, mask_pos) gives on the concatenated batch (head=False: without the [MASK] positions).  Host tables only:
    no device work, no synchronisation."""
    idx = _local(t, seq_idx)
    Lt, Li = t["Lt"], t["Li"]
    lt, li = max(1, int(t["text_len"][idx].max())), int(t["regions"][idx].max())
    if head:
        p = t["mask_pos"][idx].astype(np.int64)
        text = (p >= 0) & (p < Lt)
        if text.any():
            lt = max(lt, int(p[text].max()) + 1)
        if not text.all():                  # a region position keeps the text whole; one outside the sequence keeps both parts whole
            lt = Lt
            rest = p[~text]
            inside = (rest >= Lt) & (rest < Lt + Li)
            li = Li if not inside.all() else max(li, int(rest.max()) - Lt + 1)
    return lt, li


def gather_reference(t, seq_idx, Lt_out, Li_out):
    """The numpy restatement of cpt_gather_batch: the batch of the sequences ``seq_idx`` (global indices) cut to (Lt_out, Li_out), as
    batching.trim of the concatenated host batch holds it -- ``input_ids`` / ``segment_ids`` (B, Lt_out) int64, ``attention_mask``
    (B, Lt_out + Li_out) int64, ``mask_token_pos`` (B,) int64, ``img_feats`` (B, Li_out, D) fp32."""
    idx = _local(t, seq_idx)
    Lt, Li, D = t["Lt"], t["Li"], t["D"]
    if not (1 <= Lt_out <= Lt and 0 <= Li_out <= Li):
        raise ValueError("resident: (%d, %d) does not fit the padded (%d, %d)" % (Lt_out, Li_out, Lt, Li))
    feats = np.zeros((idx.size, Li_out, D), np.float32)
    if Li_out:
        for b, blk in enumerate(t["feat_block"][idx].tolist()):
            r, o = min(int(t["block_rows"][blk]), Li_out), int(t["block_off"][blk])
            feats[b, :r] = t["feats"][o:o + r]
    return {"input_ids": t["ids"][idx, :Lt_out].astype(np.int64), "segment_ids": t["seg"][idx, :Lt_out].astype(np.int64),
            "attention_mask": np.concatenate([t["mask"][idx, :Lt_out], t["mask"][idx, Lt:Lt + Li_out]], 1).astype(np.int64),
            "mask_token_pos": t["mask_pos"][idx].astype(np.int64), "img_feats": feats}


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

    def __init__(self, t, device, feature_dtype, dev, store):
        self.tables, self.device, self.feature_dtype = t, device, feature_dtype
        self._dev, self._store = dev, store
        self.n_items, self.n_sequences = t["n_items"], int(t["seq_first"][-1])
        self.seq_first, self.item_lo, self.item_hi = t["seq_first"], t["item_lo"], t["item_hi"]
        self.Lt, self.Li, self.D = t["Lt"], t["Li"], t["D"]
        self.nbytes = sum(v.numel() * v.element_size() for v in dev.values())

    def free(self):
        """Drop the device tables; the set cannot gather afterwards."""
        self._dev, self._store, self.nbytes = None, None, 0

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

    def gather(self, seq_idx, Lt_out, Li_out, mask_pos=True, out=None):
        """One cpt_gather_batch on the current stream.  seq_idx: int32 device tensor of GLOBAL sequence indices (the caller validates them).
        Returns ``input_ids`` / ``segment_ids`` (B, Lt_out), ``attention_mask`` (B, Lt_out + Li_out), ``mask_token_pos`` (B,) (None without
        mask_pos) -- int64 -- and ``img_feats`` (B, Li_out, D) fp32.  out: a dict of those tensors to write into (contiguous, on the device, of
        exactly these shapes) instead of fresh ones; every element is written."""
        import torch
        from . import _lib as L
        if self._store is None:
            raise RuntimeError("resident: the set was freed")
        if seq_idx.dtype != torch.int32 or not seq_idx.is_cuda or seq_idx.dim() != 1 or not seq_idx.is_contiguous():
            raise ValueError("resident: seq_idx must be a contiguous 1-D int32 tensor on the GPU")
        B, dev = seq_idx.numel(), seq_idx.device
        shapes = {"input_ids": (B, Lt_out), "segment_ids": (B, Lt_out), "attention_mask": (B, Lt_out + Li_out), "mask_token_pos": (B,),
                  "img_feats": (B, Li_out, self.D)}
        if out is None:
            out = {k: torch.empty(shape, dtype=torch.float32 if k == "img_feats" else torch.int64, device=dev) for k, shape in shapes.items()}
        else:
            for k, shape in shapes.items():
                v = out.get(k)
                if v is None and k == "mask_token_pos":
                    continue
                if v is None or tuple(v.shape) != shape or v.dtype != (torch.float32 if k == "img_feats" else torch.int64) or v.device != dev \
                        or not v.is_contiguous():
                    raise ValueError("resident: out[%r] must be a contiguous %s tensor on %s" % (k, shape, dev))
            out = dict(out)
        if not mask_pos:
            out["mask_token_pos"] = None
        L.check(L.lib().cpt_gather_batch(self._store, seq_idx.data_ptr(), B, Lt_out, Li_out, out["input_ids"].data_ptr(),
                                         out["segment_ids"].data_ptr(), out["attention_mask"].data_ptr(), L.ptr(out.get("mask_token_pos")),
                                         out["img_feats"].data_ptr() if Li_out else None, L.stream_ptr()), "cpt_gather_batch")
        return out


def upload(items_or_tables, device, feature_dtype="fp32", max_bytes=None):
    """Items (``from_queries`` / ``from_questions``) or host tables (``tables``) -> ResidentSet on ``device``.  Items are cut to this rank's
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
        t = tables(t, cdist.shard_range(t["n_items"], rank, world))
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
    small = {k: v for k, v in t.items() if k != "feats"}
    return ResidentSet(small, device, feature_dtype, dev, store)
