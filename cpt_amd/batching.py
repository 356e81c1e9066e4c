"""Length-aware evaluation, host side: how far a padded batch is attended to, trimming it, walking a data set by length and packing
whole queries into batches; for training, the extent of a mask with its label grid and the cut of that grid.  Pure numpy / python (torch CPU tensors are accepted wherever an array is): nothing here touches the GPU.

The collate functions pad every sequence to a fixed shape (RefCOCO 70 + 50, GQA / VCR 165 + 45) because eager PyTorch needs rectangular
tensors.  A position whose attention-mask column is 0 in EVERY sequence of a batch is never a key, and its own row is read by no head-row
output ([MASK] rows, the [CLS] row): ``(1 - m) * -10000`` underflows to exactly 0 after the row-max subtraction, in fp32 and in float64.
Dropping such positions changes only the order of the sums.  The device counterparts are cpt_batch_extents / cpt_trim_batch
(include/cpt_hip.h); both sides follow the same rules, stated on ``batch_extent``.
"""
import numpy as np


def _last_set(part):
    """(B, n) -> (B,) int64: 1 + the last index whose entry is non-zero, 0 where a row has none."""
    part = np.asarray(part)
    if part.shape[1] == 0:
        return np.zeros(part.shape[0], np.int64)
    return np.where(part != 0, np.arange(1, part.shape[1] + 1, dtype=np.int64), 0).max(axis=1)


def extents(attention_mask, Lt):
    """(text_len[B], regions[B]) of a (B, Lt + Li) mask: per part, 1 + the last index whose mask is set, 0 if none.  No prefix form is
    assumed: a hole in the mask stays inside the extent, so trimming to it never drops an attended position."""
    m = np.asarray(attention_mask)
    if m.ndim != 2 or not 0 < Lt <= m.shape[1]:
        raise ValueError("extents: a (B, Lt + Li) mask and 0 < Lt <= its width are needed, got %s and Lt = %d" % (m.shape, Lt))
    return _last_set(m[:, :Lt]), _last_set(m[:, Lt:])


def batch_extent(attention_mask, Lt, mask_token_pos=None):
    """(Lt', Li'): the maxima of ``extents`` over the batch, Lt' >= 1 (the [CLS] row stays), Li' possibly 0.
    mask_token_pos (head-row positions: (B,), or (n, 2) (sequence, position) pairs): a text position p gives Lt' >= p + 1; a region position
    keeps the text whole (Lt' = Lt, so that the position does not move relative to the text) and gives Li' >= p - Lt + 1; a position
    outside [0, Lt + Li) keeps both parts whole."""
    m = np.asarray(attention_mask)
    t, r = extents(m, Lt)
    Li = m.shape[1] - Lt
    lt, li = max(1, int(t.max(initial=0))), int(r.max(initial=0))
    if mask_token_pos is not None:
        pos = np.asarray(mask_token_pos)
        pos = (pos[:, 1] if pos.ndim == 2 else pos.reshape(-1)).astype(np.int64)
        for p in pos.tolist():
            if 0 <= p < Lt:
                lt = max(lt, p + 1)
            else:
                lt = Lt
                li = max(li, p - Lt + 1) if Lt <= p < Lt + Li else Li
    return lt, li


def trim(batch, Lt2, Li2):
    """A copy of the batch dict with ``input_ids``, ``segment_ids``, ``position_ids`` (when present) cut to (B, Lt'), ``img_feats`` (when
    present) to (B, Li', D), and ``attention_mask`` rebuilt as (B, Lt' + Li') from its text and region parts.  Every other entry is passed
    through.  Arrays and CPU tensors alike: only slicing and one concatenation are used."""
    ids = batch["input_ids"]
    Lt = ids.shape[1]
    mask = batch["attention_mask"]
    Li = mask.shape[1] - Lt
    if not (1 <= Lt2 <= Lt and 0 <= Li2 <= Li):
        raise ValueError("trim: (%d, %d) does not fit the padded (%d, %d)" % (Lt2, Li2, Lt, Li))
    out = dict(batch)
    for k in ("input_ids", "segment_ids", "position_ids"):
        if batch.get(k) is not None:
            out[k] = batch[k][:, :Lt2]
    if batch.get("img_feats") is not None:
        out["img_feats"] = batch["img_feats"][:, :Li2]
    parts = (mask[:, :Lt2], mask[:, Lt:Lt + Li2])
    if isinstance(mask, np.ndarray):
        out["attention_mask"] = np.concatenate(parts, 1)
    else:
        import torch
        out["attention_mask"] = torch.cat(parts, 1)
    return out


def label_extent(attention_mask, Lt, label_grid=None):
    """(Lt', Li') of a training batch: ``batch_extent`` of the (B, Lt + Li) mask, widened so that every labelled position of the (B, Lt + Li)
    ``label_grid`` (-1 = no label: drivers.gqa_label_grid, vg_label_grid, _label_grid) stays -- a labelled column is a head-row position of
    ``batch_extent``: Lt' > every labelled text position, a labelled region column keeps the text whole.  Without a grid (the relation heads
    read [CLS] only) the extent comes from the mask alone.  The device counterpart is cpt_train_extents."""
    m = np.asarray(attention_mask)
    if label_grid is None:
        return batch_extent(m, Lt)
    g = np.asarray(label_grid)
    if g.shape != m.shape:
        raise ValueError("label_extent: the label grid is %s, the mask %s" % (g.shape, m.shape))
    return batch_extent(m, Lt, np.unique(np.nonzero(g != -1)[1]))


def trim_grid(label_grid, Lt, Lt2, Li2):
    """The (B, Lt + Li) label grid cut as ``trim`` cuts the mask: text columns [0, Lt') then region columns [Lt, Lt + Li') -> (B, Lt' + Li').
    An array or a CPU tensor."""
    Li = label_grid.shape[1] - Lt
    if not (1 <= Lt2 <= Lt and 0 <= Li2 <= Li):
        raise ValueError("trim_grid: (%d, %d) does not fit the padded (%d, %d)" % (Lt2, Li2, Lt, Li))
    parts = (label_grid[:, :Lt2], label_grid[:, Lt:Lt + Li2])
    if isinstance(label_grid, np.ndarray):
        return np.concatenate(parts, 1)
    import torch
    return torch.cat(parts, 1)


def length_order(text_len, regions):
    """(order, inverse): ``order`` walks the sequences by ascending text_len + regions, stable (equal lengths keep their order);
    inverse[order[i]] = i, so ``x[order][inverse]`` is ``x``."""
    key = np.asarray(text_len, dtype=np.int64) + np.asarray(regions, dtype=np.int64)
    order = np.argsort(key, kind="stable")
    inverse = np.empty_like(order)
    inverse[order] = np.arange(order.size)
    return order, inverse


def pack_queries(counts, max_sequences):
    """Consecutive groups (lists of query indices) of WHOLE queries with sum(counts) <= max_sequences per group; a query larger than the
    cap forms a group of its own.  The groups concatenated are range(len(counts))."""
    if max_sequences < 1:
        raise ValueError("pack_queries: max_sequences must be at least 1")
    groups, cur, total = [], [], 0
    for i, c in enumerate(counts):
        c = int(c)
        if cur and total + c > max_sequences:
            groups.append(cur)
            cur, total = [], 0
        cur.append(i)
        total += c
    if cur:
        groups.append(cur)
    return groups
