"""Driver-side hot loops on the HIP path: counterparts of the reference's ``val`` and ``train_batch``.

  * ``val_queries``  <- Oscar/oscar/zeroshot/refcoco_cpt.py:208-288 (and the few-shot
    variant fewshot/refcoco_cpt.py:258-315): per query, score every proposal sequence at its [MASK]
    slot, gather the colour logits, argmax -> chosen rectangle; queries are sharded across ranks and
    the chosen indices are gathered with one fixed-shape all_gather.
  * ``val_rec``      <- the same two val() functions to their end: selection, IoU against the annotation and
    the accuracy they return, in one launch per batch against tables uploaded once (cpt_rec_choose).
  * ``train_batch``  <- fewshot/refcoco_cpt.py:225-255: label grid, LR schedule, zero_grad / loss /
    backward / step, RuntimeError per step logged and skipped.
Datasets, tokeniser and TSV decoding stay outside: a *query* here is already
tensors, in the layout ``test_collate`` (zeroshot/refcoco_cpt.py:159-172) produces.
"""
import logging

import numpy as np
import torch

from . import batching
from . import dist as cdist
from . import resident as rsd
from . import scoring
from .train import get_lr_sched

logger = logging.getLogger(__name__)


# ---- the evaluation pass every val_* driver runs (_eval_pass) --------------------------------------------------------------------------------
#   Items (queries, pairs, questions) are sharded over ranks, whole items per rank (dist.shard_range); each rank walks ITS shard in groups
#   (_walk), the driver's ``step`` scores one group -- batch, one forward, one choice kernel -- and the results go into fixed-shape shard-local
#   tensors that one all_gather per output brings to every rank (dist.gather_fixed).  A driver holds its constants, its ``step`` and what it
#   makes of the gathered tensors.  Length-aware evaluation (batching.py), all off by default:
#   trim    the host arrays of every batch are cut to the part some sequence attends to BEFORE the H2D copy (batching.trim: no device copy, fewer
#           PCIe bytes); the encoder then runs on (B, Lt' + Li').  Head-row outputs only, which is all these drivers read.
#   bucket  each rank walks ITS shard by ascending length (batching.length_order; an item of several sequences -- a query, a VCR question, a VG
#           pair -- stays whole and counts by its longest sequence) and writes every result back at the item's own index.
#   Length-aware training: the six training loops below take trim=False too.  With trim=True the label grid of each micro-batch is built on the
#   host, the extent comes from the mask AND the grid (batching.label_extent: every labelled position stays; the relation heads' extent from the
#   mask alone, both Q->AR blocks sharing one), and the host arrays and the grid are cut before the H2D copy: no device work, no synchronisation.
#   The trimmed rows contribute exact zeros to the loss's gradient, so only the order of the sums changes; with dropout on, the masks are drawn
#   for the shape that runs, so a trimmed step draws other masks than the padded one would (README "Length-aware training").
#   Device-resident sets (resident.py; val_queries, val_rec and val_gqa take resident=None): with a ResidentSet the walk is computed up front
#   from the set's host tables (bucket keys from text_len + regions, max_sequences from seq_first: no mask is scanned), the sequence indices of
#   ALL steps go up in one copy per pass, and a step is resident.extent (trim) or the padded shape, ONE cpt_gather_batch, the unchanged forward
#   and the unchanged choice launch.  No tensor of the items is read; the returns are the host path's, field for field and bit for bit.
#   val_vg, val_vcr and val_vcr_qar take resident= too (sets with head tables: resident.from_pairs / from_vcr / from_vcr_qar).  VG sequences hold
#   1, 2 or 3 [MASK] rows, so a VG step is ONE cpt_gather_batch_heads, which also writes the (n, 2) head rows; their prefix sums (row_first) go up
#   with the index lists, still one copy per pass.  A Q->AR step gathers both blocks in one launch (all Q->A sequences, then all QA->R).
#   Training: train_batch, train_vg_batch and tune_soft_template take resident= (resident.from_train_batches); ``batches`` is then an iterable of
#   1-D arrays of global sequence indices -- any grouping, so an epoch's reshuffle costs an index list -- and a step's batch AND its label grid
#   come from one cpt_gather_batch_heads (trim=True: cut to resident.extent of that batch, the rule of batching.label_extent).
def _item_length(mask, Lt):
    """The length key of one item: text_len + regions of its longest sequence."""
    t, r = batching.extents(mask, Lt)
    return int((t + r).max())


def _walk(n, size, keys=None, counts=None, cap=None):
    """Lists of shard-local item indices: in data set order, or (keys: bucket) by ascending length key, stable.  ``size`` items per list -- or
    (cap: max_sequences) whole items of counts[i] sequences each, consecutive in that order, at most cap sequences per list
    (batching.pack_queries)."""
    order = list(range(n)) if keys is None else batching.length_order(keys, 0)[0].tolist()
    if cap is None:
        return [order[i:i + size] for i in range(0, n, size)]
    return [[order[i] for i in g] for g in batching.pack_queries([counts[i] for i in order], cap)]


def _upload_lists(lists, device):
    """int32 lists -> their device tensors, slices of ONE copy."""
    flat = rsd.h2d(np.concatenate(lists).astype(np.int32), device, "seq_idx")
    out, o = [], 0
    for x in lists:
        out.append(flat[o:o + x.size])
        o += x.size
    return out


def _resident_walk(res, model, n_items, n_sequences, lo, hi, size, bucket, cap, trim, device, what, heads=False, order=None):
    """The walk of this rank's shard [lo, hi) over a ResidentSet: (groups as _walk gives them, {first item of a group: (its sequence indices
    on the device, Lt', Li')}).  Everything comes from the set's host tables; the index lists of all groups go up in ONE copy.
    heads: a plan is (sequence indices, Lt', Li', row_first on the device, R) -- the prefix sums of the head counts of every group ride in the
    same copy.  order(group) -> the group's sequence indices, where they are not the items' sequences one item after the other (Q->AR)."""
    res.check_items(n_items, n_sequences, lo, hi, what)
    res.check_model(model, what)
    sf = res.seq_first
    counts = (sf[lo + 1:hi + 1] - sf[lo:hi]).tolist() if cap is not None else None
    groups = _walk(hi - lo, size, rsd.item_keys(res.tables) if bucket else None, counts, cap)
    if heads and not rsd.has_heads(res.tables):
        raise ValueError("%s: the resident set has no head tables (it was built for another driver)" % what)
    if order is None:
        order = lambda g: np.concatenate([np.arange(sf[lo + i], sf[lo + i + 1]) for i in g])
    seqs = [order(g) for g in groups]
    plans = {}
    if seqs:
        firsts = [rsd.row_first(res.tables, s) for s in seqs] if heads else []
        dev = _upload_lists(seqs + firsts, device)
        for k, (g, s) in enumerate(zip(groups, seqs)):
            lt, li = rsd.extent(res.tables, s) if trim else (res.Lt, res.Li)
            plans[g[0]] = (dev[k], lt, li) + ((dev[len(seqs) + k], int(firsts[k][-1])) if heads else ())
    return groups, plans


def _sel(idx, device, bucket):
    """Where the results of the items ``idx`` go in a shard-local result tensor: a slice in data set order, an index tensor under bucket."""
    return torch.as_tensor(idx, device=device) if bucket else slice(idx[0], idx[-1] + 1)


def _eval_pass(n_items, groups_of, outputs, step, device, bucket):
    """One sharded evaluation pass over n_items.  outputs: one (trailing shape, dtype, fill) per result tensor; groups_of(lo, hi) -> the lists
    of shard-local indices of this rank's shard [lo, hi) (_walk); step(idx_local, lo) -> one tensor per output for those items, run under
    no_grad.  Returns the (n_items, ...) tensors gathered to every rank, on the device, in the order of ``outputs``."""
    rank, world = cdist.rank_world()
    lo, hi = cdist.shard_range(n_items, rank, world)
    local = [torch.full((hi - lo,) + tuple(shape), fill, dtype=dtype, device=device) for shape, dtype, fill in outputs]
    for idx in groups_of(lo, hi):
        with torch.no_grad():
            res = step(idx, lo)
        if local:       # (a step that writes its results itself, at the items' global indices, returns nothing: val_rec)
            sel = _sel(idx, device, bucket)
            for t, r in zip(local, res):
                t[sel] = r
    return tuple(cdist.gather_fixed(t, n_items, fill=o[2]) for t, o in zip(local, outputs))


def _dedup_accuracy(flags, q_ids, n):
    """The reference's accuracy over results keyed by question id (results_dic = {k["questionId"]: k ...}: the last entry of an id wins;
    vcr_qar_nsp_cpt.py:682, gqa_cpt.py:619, vcr_nsp_cpt.py:619): the flags of the kept entries summed, divided by the number of questions n.
    flags (len(q_ids),) -> float; (len(q_ids), k) -> k floats, one per column."""
    last = {}
    for i, qid in enumerate(q_ids):
        last[qid] = i
    kept = flags[sorted(last.values())].sum(0)
    return [float(v) / n for v in kept.tolist()] if kept.dim() else float(kept.item()) / n


def _seq_feats(f, n, device, li=None):
    """img_feats of one item on the device: the first li regions (all of them without li) are moved, and (Li, D) is expanded to the item's n
    sequences there (the collate functions stack it per sequence)."""
    f = torch.as_tensor(f)[..., :li, :].to(device, non_blocking=True)
    return f.unsqueeze(0).expand(n, -1, -1) if f.dim() == 2 else f


def _trim_host(b, head_pos=None):
    """batching.trim of a host batch to its own batch extent -> (batch, Li')."""
    lt, li = batching.batch_extent(b["attention_mask"], b["input_ids"].shape[1], head_pos)
    return batching.trim(b, lt, li), li


def _trim_train_host(host, grid):
    """A host batch (CPU tensors) and its (B, Lt + Li) label grid, both cut to batching.label_extent of the two."""
    Lt = host["input_ids"].shape[1]
    lt, li = batching.label_extent(host["attention_mask"], Lt, grid)
    return batching.trim(host, lt, li), batching.trim_grid(grid, Lt, lt, li)


def val_queries(model, queries, none_id, device, few_shot=False, batch_queries=4, colour_columns_only=True, trim=False, bucket=False,
                max_sequences=None, resident=None):
    """queries: list of dicts with tensors ``img_feats (P,Li,D)``, ``input_ids (P,Lt)``,
    ``segment_ids``, ``attention_mask (P,Lt+Li)``, ``mask_token_pos (P,)`` and python lists
    ``colors`` (per proposal sequence: colour-token ids) and ``rects`` (per sequence: rectangles).
    Returns {global query index: (max_idx, rect)} on every rank.
    colour_columns_only (default): the decoder scores only the vocabulary columns the selection reads -- every colour id of the queries + ``none_id``
    (zeroshot/refcoco_cpt.py:219 gathers exactly those out of the (P, V) scores) -- instead of all V; same chosen indices.
    trim / bucket: length-aware evaluation, see the top of this module.  max_sequences: batches are consecutive groups of whole queries with at
    most that many proposal sequences (batching.pack_queries) instead of ``batch_queries`` queries each -- even launches for ragged queries.
    resident: a ResidentSet of these queries (resident.upload(resident.from_queries(queries), device)): the batches are gathered on the
    device, only ``colors`` and ``rects`` of the queries are read; see the top of this module."""
    model.eval()
    plans = {}
    col_ids, col_of, cols_dev = None, None, None
    if colour_columns_only:
        col_ids = sorted({int(c) for q in queries for s in q["colors"] for c in s} | {int(none_id)})
        col_of = {c: i for i, c in enumerate(col_ids)}
        cols_dev = torch.tensor(col_ids, dtype=torch.int64, device=device)

    def groups_of(lo, hi):
        if resident is not None:
            groups, found = _resident_walk(resident, model, len(queries), sum(len(q["colors"]) for q in queries), lo, hi, batch_queries, bucket,
                                           max_sequences, trim, device, "val_queries")
            plans.update(found)
            return groups
        shard = queries[lo:hi]
        keys = [_item_length(q["attention_mask"], q["input_ids"].shape[1]) for q in shard] if bucket else None
        counts = [q["input_ids"].size(0) for q in shard] if max_sequences is not None else None
        return _walk(hi - lo, batch_queries, keys, counts, max_sequences)

    def step(idx_local, lo):
        chunk = [queries[lo + i] for i in idx_local]
        if resident is not None:
            cat = resident.gather(*plans[idx_local[0]])
        else:
            cat = {k: torch.cat([q[k] for q in chunk], 0) for k in ("img_feats", "input_ids", "segment_ids", "attention_mask", "mask_token_pos")}
            if trim:
                cat = _trim_host(cat, cat["mask_token_pos"])[0]
            cat = {k: v.to(device, non_blocking=True) for k, v in cat.items()}
        scores = model(cat["input_ids"], cat["segment_ids"], cat["attention_mask"], img_feats=cat["img_feats"],
                       mask_token_pos=cat["mask_token_pos"], vocab_columns=cols_dev)[0]      # (None: all V columns)
        # colour gather + per-query argmax run on the device (cpt_select_regions): only indices leave the GPU
        sets = [list(s) for q in chunk for s in q["colors"]]
        if col_of is not None:      # (ids -> positions in the column list the scores were computed for)
            sets = [[col_of[int(c)] for c in s] for s in sets]
        first = [0]
        for q in chunk:
            first.append(first[-1] + (q["input_ids"].size(0) if resident is None else len(q["colors"])))   # (one colour list per sequence)
        return (scoring.select_regions_device(scores, sets, first, none_id if col_of is None else col_of[int(none_id)], few_shot=few_shot),)

    chosen, = _eval_pass(len(queries), groups_of, [((), torch.int64, -1)], step, device, bucket)
    allc = chosen.cpu().tolist()
    out = {}
    for gi, idx in enumerate(allc):
        rects = [r for rs in queries[gi]["rects"] for r in rs]
        # a query none of whose proposal sequences carries a colour has no prediction (idx -1): never index rects[-1]
        out[gi] = (idx, rects[idx] if 0 <= idx < len(rects) else None)
    return out


def _gather_ranges(buf, bounds):
    """buf (n_total, ...) holds this rank's range [bounds[rank], bounds[rank + 1]) of a ragged split; every rank gets the whole tensor: one
    fixed-shape all_gather, padded to the longest range."""
    rank, world = cdist.rank_world()
    if world == 1:
        return buf
    mx = max(max(bounds[r + 1] - bounds[r] for r in range(world)), 1)
    pad = torch.zeros((mx,) + tuple(buf.shape[1:]), dtype=buf.dtype, device=buf.device)
    pad[:bounds[rank + 1] - bounds[rank]] = buf[bounds[rank]:bounds[rank + 1]]
    bufs = [torch.empty_like(pad) for _ in range(world)]
    torch.distributed.all_gather(bufs, pad)
    return torch.cat([bufs[r][:bounds[r + 1] - bounds[r]] for r in range(world)], 0)


def val_rec(model, queries, gts, none_id, device, few_shot=False, batch_queries=4, colour_columns_only=True, trim=False, bucket=False,
            max_sequences=None, table=None, return_candidate_scores=False, resident=None):
    """The whole of val() (zeroshot/refcoco_cpt.py:208-288, fewshot/refcoco_cpt.py:258-315) with the evaluation on the device: the pass of
    val_queries -- same queries, sharding, walking and trim / bucket / max_sequences -- whose step is concatenate, one forward, ONE launch
    (cpt_rec_choose): selection, the chosen box's float64 IoU against the annotation, correct = IoU > 0.5 and the counts, against tables
    uploaded once (scoring.rec_eval_table; pass ``table`` to reuse one over several passes of a split).  Per step only the batch's query
    indices are uploaded and nothing is read back.  gts: per query its annotation [x, y, w, h] or None.
    Returns {"accuracy": percent = correct / evaluated, the number val() returns, "n_evaluated", "n_unpredicted" (queries without a colour),
    "predictions": {query index: (idx, rect)} as val_queries returns, "correct" (Q,) uint8, "iou" (Q,) float64, "score" (Q,) fp32 host arrays,
    and with return_candidate_scores "candidate_scores" (R_total,) fp32: every candidate's score, val()'s to_save_predictions[k]["scores"]
    concatenated} on every rank.  A query without a colour or without an annotation is counted in neither sum.
    resident: a ResidentSet of these queries, as val_queries takes it; the batches are then gathered on the device."""
    model.eval()
    plans = {}
    if table is None:
        col_ids = sorted({int(c) for q in queries for s in q["colors"] for c in s} | {int(none_id)}) if colour_columns_only else None
        table = scoring.rec_eval_table(queries, gts, none_id, col_ids)
    if table["n_queries"] != len(queries) or (table["col_ids"] is None) == bool(colour_columns_only) or table["none_id"] != int(none_id):
        raise ValueError("val_rec: the table was built for other queries, another none_id or another colour_columns_only")
    cols_dev = None if table["col_ids"] is None else torch.tensor(table["col_ids"], dtype=torch.int64, device=device)
    scoring.rec_table_device(table, device)
    out = scoring.rec_eval_buffers(table, device, return_candidate_scores)

    def groups_of(lo, hi):
        if resident is not None:
            groups, found = _resident_walk(resident, model, len(queries), int(table["seq_first"][-1]), lo, hi, batch_queries, bucket,
                                           max_sequences, trim, device, "val_rec")
            plans.update(found)
            return groups
        shard = queries[lo:hi]
        keys = [_item_length(q["attention_mask"], q["input_ids"].shape[1]) for q in shard] if bucket else None
        counts = [q["input_ids"].size(0) for q in shard] if max_sequences is not None else None
        return _walk(hi - lo, batch_queries, keys, counts, max_sequences)

    def step(idx_local, lo):
        if resident is not None:
            cat = resident.gather(*plans[idx_local[0]])
        else:
            cat = {k: torch.cat([queries[lo + i][k] for i in idx_local], 0)
                   for k in ("img_feats", "input_ids", "segment_ids", "attention_mask", "mask_token_pos")}
            if trim:
                cat = _trim_host(cat, cat["mask_token_pos"])[0]
            cat = {k: v.to(device, non_blocking=True) for k, v in cat.items()}
        scores = model(cat["input_ids"], cat["segment_ids"], cat["attention_mask"], img_feats=cat["img_feats"],
                       mask_token_pos=cat["mask_token_pos"], vocab_columns=cols_dev)[0]
        scoring.rec_choose_device(scores, [lo + i for i in idx_local], table, few_shot, out)
        return ()

    n = len(queries)
    _eval_pass(n, groups_of, [], step, device, bucket)
    rank, world = cdist.rank_world()
    lo, hi = cdist.shard_range(n, rank, world)
    idx, score, iou, correct = (cdist.gather_fixed(out[k][lo:hi], n) for k in ("idx", "score", "iou", "correct"))
    counts = out["counts"]
    if world > 1:       # (the counts of every rank's shard, summed)
        every = [torch.empty_like(counts) for _ in range(world)]
        torch.distributed.all_gather(every, counts)
        counts = torch.stack(every).sum(0)
    n_correct, n_eval = counts.cpu().tolist()
    chosen = idx.cpu().tolist()
    res = {"accuracy": n_correct / max(n_eval, 1) * 100, "n_evaluated": n_eval, "n_unpredicted": sum(1 for i in chosen if i < 0),
           "correct": correct.cpu().numpy(), "iou": iou.cpu().numpy(), "score": score.cpu().numpy()}
    if return_candidate_scores:
        cf = table["cand_first"].tolist()
        bounds = [cf[cdist.shard_range(n, r, world)[0]] for r in range(world)] + [cf[n]]
        res["candidate_scores"] = _gather_ranges(out["cand_score"], bounds).cpu().numpy()
    preds = {}
    for gi, i in enumerate(chosen):
        rects = [r for rs in queries[gi]["rects"] for r in rs]
        preds[gi] = (i, rects[i] if 0 <= i < len(rects) else None)
    res["predictions"] = preds
    return res


def _label_grid(batch):
    """(B, L) grid of -1 with each sequence's colour id at its [MASK] slot: what CrossEntropyLoss(ignore_index=-1) of
    modeling_rec.py:147-150 wants (fewshot/refcoco_cpt.py:231-233)."""
    grid = batch["attention_mask"].new_full(batch["attention_mask"].shape, -1, dtype=torch.long)
    # index assignment as the reference writes it: any integer dtype and negative (from-the-end) positions are accepted
    grid[torch.arange(grid.size(0), device=grid.device), batch["mask_token_pos"].long().view(-1)] = batch["colors"].long().view(-1)
    return grid


def _apply_lr(optimizer, lr, head_multiplier):
    """The reference's parameter groups (fewshot/refcoco_cpt.py:236-243, 318-343): groups 0-1 take lr x lr_mul, groups 2-3 the plain
    rate; like the reference, an optimizer with fewer groups trains and only a fifth group raises."""
    groups = optimizer.param_groups
    if len(groups) > 4:
        raise ValueError("at most the four parameter groups of build_optimizer are scheduled, got %d" % len(groups))
    for g in groups[:2]:
        g["lr"] = lr * head_multiplier
    for g in groups[2:]:
        g["lr"] = lr


def _device_batch(host_batch, grid_fn, device, trim):
    """(batch on the device, its label grid on the device).  trim: the grid is built on the host and both are cut there first."""
    if not trim:
        batch = {name: torch.as_tensor(t).to(device) for name, t in host_batch.items()}
        return batch, grid_fn(batch)
    host = {name: torch.as_tensor(t) for name, t in host_batch.items()}
    host, grid = _trim_train_host(host, grid_fn(host))
    batch = {name: t.to(device) for name, t in host.items()}
    if batch.get("img_feats") is not None and batch["img_feats"].size(1) == 0:
        batch["img_feats"] = None          # Li' = 0: the step runs text-only, as it does without regions
    return batch, grid.to(device)


def _resident_batches(res, model, batches, device, trim, what):
    """The training steps of a pass over a ResidentSet (resident.from_train_batches): ``batches`` is an iterable of 1-D integer arrays of global
    sequence indices.  The lists are materialised once and go up in ONE copy; yields per step (batch, label grid), both written by one
    cpt_gather_batch_heads.  trim: every batch is cut to resident.extent of its sequences (labelled positions kept)."""
    if res._store is None:
        raise RuntimeError("%s: the resident set was freed" % what)
    t = res.tables
    if not rsd.has_heads(t) or t["head_label"] is None:
        raise ValueError("%s: the resident set has no labelled head rows (build it with resident.from_train_batches)" % what)
    res.check_model(model, what)
    lists = []
    for b in batches:
        b = np.asarray(b.cpu() if hasattr(b, "cpu") else b)
        if b.ndim != 1 or b.dtype.kind not in "iu" or b.size == 0:
            raise ValueError("%s: with a resident set a batch is a non-empty 1-D integer array of sequence indices, got %s %s" % (what, b.dtype, b.shape))
        rsd._local(t, b)                                   # (raises for an index outside the stored sequences)
        lists.append(b.astype(np.int64))
    dev = _upload_lists(lists, device) if lists else []

    def steps():
        for seq, idx in zip(dev, lists):
            lt, li = rsd.extent(t, idx, labelled=True) if trim else (res.Lt, res.Li)
            b = res.gather(seq, lt, li, mask_pos=False, heads=("label_grid",))
            if li == 0:
                b["img_feats"] = None                      # Li' = 0: the step runs text-only, as it does without regions
            yield b, b["label_grid"]
    return steps()


def _scheduled_pass(model, optimizer, batches, opts, device, global_step, grid_fn, trim=False, resident=None, what="train_batch"):
    """The loop train_batch and train_vg_batch share: per batch the scheduled learning rate, then zero_grad / forward with
    masked_lm_labels=grid_fn(batch) / backward / step; a step that raises RuntimeError is logged and skipped without advancing the schedule.
    Returns (global_step, [loss tensors]).  resident: the batches and their grids are gathered on the device (_resident_batches)."""
    model.train()
    losses = []
    if resident is not None:
        steps = _resident_batches(resident, model, batches, device, trim, what)
    else:
        steps = (_device_batch(host_batch, grid_fn, device, trim) for host_batch in batches)
    for index, (batch, grid) in enumerate(steps):
        _apply_lr(optimizer, get_lr_sched(global_step, opts), getattr(opts, "lr_mul", 1.0))
        try:
            optimizer.zero_grad()
            loss = model(batch["input_ids"], batch["segment_ids"], batch["attention_mask"], img_feats=batch["img_feats"],
                         masked_lm_labels=grid)[0]
            loss.backward()
            optimizer.step()
        except RuntimeError as err:
            logger.info("step %d of this pass skipped: %s", index, err)
            continue
        global_step += 1
        losses.append(loss.detach())
    return global_step, losses


def train_batch(model, optimizer, batches, opts, device, global_step=0, trim=False, resident=None):
    """One pass over ``batches`` (dicts with img_feats, input_ids, attention_mask, segment_ids, mask_token_pos, colors): the few-shot
    step of fewshot/refcoco_cpt.py:225-255 -- label grid, scheduled learning rate, zero_grad / forward / backward / step; a step that
    raises RuntimeError is logged and skipped without advancing the schedule (_scheduled_pass).  Returns (global_step, [loss tensors]).
    trim: length-aware training, see the top of this module.
    resident: a ResidentSet of the training batches (resident.upload(resident.from_train_batches(batch dicts), device)); ``batches`` is then an
    iterable of 1-D integer arrays of global sequence indices into it (resident.batch_indices(): the grouping it was built from; any other
    grouping is allowed) and every step's batch and label grid are gathered on the device by one launch."""
    return _scheduled_pass(model, optimizer, batches, opts, device, global_step, _label_grid, trim, resident, "train_batch")


def tune_soft_template(model, optimizer, batches, device, trim=False, resident=None):
    """The template-tuning loop of explore/sgd_to_explore_template.py:396-412 on a model with a soft template attached
    (cpt_amd/soft_prompt.py attach; ``optimizer`` is any torch optimizer over that one tensor -- the reference builds
    ``AdamW([template], lr=0.02, eps=1e-8)``): per batch the label grid with the colour id at the [MASK] position, the loss divided
    ADDITIONALLY by the batch size (:409), zero_grad / backward / step.  Returns the list of (divided) loss tensors.
    The reference runs this loop on BertImgForPreTraining with next_sentence_label=0, so its loss also carries the contrastive term;
    here it is REC_MLM_CPT's MLM loss alone.  trim: length-aware training, see the top of this module.  resident: as train_batch takes it."""
    model.train()
    losses = []
    if resident is not None:
        steps = _resident_batches(resident, model, batches, device, trim, "tune_soft_template")
    else:
        steps = (_device_batch(host_batch, _label_grid, device, trim) for host_batch in batches)
    for batch, grid in steps:
        optimizer.zero_grad()
        loss = model(batch["input_ids"], batch["segment_ids"], batch["attention_mask"], img_feats=batch["img_feats"],
                     masked_lm_labels=grid)[0]
        loss = loss / batch["input_ids"].size(0)
        loss.backward()
        optimizer.step()
        losses.append(loss.detach())
    return losses


# ---- VG-CPT (Oscar/oscar/fewshot/vg_cpt.py; launched by cmds/vg/_fsl.sh with 16 pairs per GPU) ------------------------------------
def _vg_cat(chunk, device, per_pair, trim=False):
    """Concatenate pairs (dicts of prompts.assemble_vg_* arrays + img_feats) into one batch; mask_token_pos gets the pair's sequence
    offset.  img_feats (Li, D) is repeated per sequence on the device (the reference stacks it per sequence).  trim: the host arrays are cut
    to the batch extent first (the head rows kept), and only the first Li' regions of every image are moved."""
    t = lambda x: torch.as_tensor(x)
    out = {k: torch.cat([t(q[k]) for q in chunk], 0) for k in ("input_ids", "segment_ids", "attention_mask")}
    pos = torch.cat([t(q["mask_token_pos"]).long() + torch.tensor([per_pair * i, 0]) for i, q in enumerate(chunk)], 0)
    li = None
    if trim:
        out, li = _trim_host(out, pos)
    out = {k: v.to(device, non_blocking=True) for k, v in out.items()}
    out["img_feats"] = torch.cat([_seq_feats(q["img_feats"], per_pair, device, li) for q in chunk], 0).contiguous()
    out["mask_token_pos"] = pos.to(device)
    return out


def val_vg(model, pairs, idx2pred, device, batch_pairs=16, trim=False, bucket=False, resident=None):
    """Zero-shot / evaluation pass of vg_cpt.py:255-305.  pairs: one dict per TSV row -- ``img_key`` (the image name), ``input_ids``
    (6, Lt), ``segment_ids``, ``attention_mask`` (6, Lt + Li), ``mask_token_pos`` (12, 2) as prompts.assemble_vg_zsl gives them, and
    ``img_feats`` (Li, D) or (6, Li, D).  Pairs are sharded across ranks as val_queries shards queries; each batch is scored on the
    device (scoring.vg_predicate_scores) and the fixed-shape (pairs, 2, C) scores are gathered with one all_gather.
    Returns (scores (pairs, 2, C) fp32 on the device, keys): keys[2 i] = pair i's key, keys[2 i + 1] = its reverse_imkey -- the rows of
    scores.view(-1, C), in dataset order, as scoring.vg_eval_table takes them.  trim / bucket: see the top of this module.
    resident: a ResidentSet of these pairs (resident.upload(resident.from_pairs(pairs), device)): every batch and its head rows are gathered on
    the device by one launch, only ``img_key`` of the pairs is read."""
    model.eval()
    C = max(int(i) for i in idx2pred) + 1
    plans = {}

    def groups_of(lo, hi):
        if resident is not None:
            groups, found = _resident_walk(resident, model, len(pairs), 6 * len(pairs), lo, hi, batch_pairs, bucket, None, trim, device, "val_vg",
                                           heads=True)
            plans.update(found)
            return groups
        return _walk(hi - lo, batch_pairs,
                     [_item_length(q["attention_mask"], np.asarray(q["input_ids"]).shape[1]) for q in pairs[lo:hi]] if bucket else None)

    def step(idx, lo):
        if resident is not None:
            seq, lt, li, first, R = plans[idx[0]]
            b = resident.gather(seq, lt, li, mask_pos=False, row_first=first, R=R, heads=("head_rows",))
            b["mask_token_pos"] = b["head_rows"]
        else:
            b = _vg_cat([pairs[lo + i] for i in idx], device, 6, trim)
        return (scoring.vg_predicate_scores(model, b["input_ids"], b["segment_ids"], b["attention_mask"], b["img_feats"], b["mask_token_pos"],
                                            idx2pred),)

    scores, = _eval_pass(len(pairs), groups_of, [((2, C), torch.float32, 0)], step, device, bucket)
    keys = []
    for q in pairs:
        keys += [q["img_key"], scoring.reverse_imkey(q["img_key"])]
    return scores, keys


def vg_label_grid(batch):
    """vg_cpt.py:227-229: a (B, L) grid of -1 with row_labels at the (sequence, position) rows of mask_token_pos (n, 2)."""
    grid = batch["attention_mask"].new_full(batch["attention_mask"].shape, -1, dtype=torch.long)
    pos = batch["mask_token_pos"].long()
    grid[pos[:, 0], pos[:, 1]] = batch["row_labels"].long().view(-1)
    return grid


def vg_schedule(opts, num_train_epochs):
    """vg_cpt.py:532-533, quirk kept: num_train_steps = num_train_epochs and warmup_steps = int(num_train_epochs / 10), so the rate
    reaches its 1e-8 floor after num_train_epochs STEPS whatever the data set size.  Sets them on opts and returns it."""
    opts.num_train_steps = num_train_epochs
    opts.warmup_steps = int(num_train_epochs / 10)
    return opts


def train_vg_batch(model, optimizer, batches, opts, device, global_step=0, trim=False, resident=None):
    """One pass of vg_cpt.py:217-252 (train_batch) over ``batches``: dicts with img_feats, input_ids, attention_mask, segment_ids,
    mask_token_pos (n, 2) (sequence, position) and row_labels (n,) -- prompts.assemble_vg_train rows concatenated, 6 labelled rows per
    pair.  The label grid holds several labelled positions per sequence (the multi-row training path of REC_MLM_CPT.forward); LR
    schedule (opts from vg_schedule), zero_grad / forward / backward / step and the skipped-step rule as train_batch (_scheduled_pass).
    Returns (global_step, [loss tensors]).  trim: length-aware training, see the top of this module.  resident: as train_batch takes it (the
    set built from these batch dicts: every sequence owns its labelled rows)."""
    return _scheduled_pass(model, optimizer, batches, opts, device, global_step, vg_label_grid, trim, resident, "train_vg_batch")


# ---- VCR Q->AR (Oscar/oscar/fewshot/vcr_qar_nsp_cpt.py; launched by cmds/vcr/qar_cpt_fsl.sh) ----------------------------------------------
def _qar_blocks(chunk, device, trim=False):
    """Concatenate questions (prompts.assemble_vcr_qar dicts + ``img_feats`` (Li, D)) into the Q->A block and the QA->R block of one batch, in
    the reference's inputs-dict layout; img_feats is expanded per sequence on the device (vcr_collate_fn stacks it per sequence).  trim: both
    blocks are cut on the host to ONE extent, the larger of the two (they run as one batch), and only the first Li' regions are moved."""
    t = lambda x: torch.as_tensor(x)
    host = [{"input_ids": torch.cat([t(q[part]["input_ids"]) for q in chunk], 0),
             "attention_mask": torch.cat([t(q[part]["input_mask"]) for q in chunk], 0),
             "segment_ids": torch.cat([t(q[part]["segment_ids"]) for q in chunk], 0)} for part in ("q_a", "qa_r")]
    li = None
    if trim:
        ext = [batching.batch_extent(b["attention_mask"], b["input_ids"].shape[1]) for b in host]
        lt, li = max(e[0] for e in ext), max(e[1] for e in ext)
        host = [batching.trim(b, lt, li) for b in host]
    blocks = []
    for part, b in zip(("q_a", "qa_r"), host):
        feats = [_seq_feats(q["img_feats"], q[part]["input_ids"].shape[0], device, li) for q in chunk]
        blocks.append({"input_ids": b["input_ids"].to(device, non_blocking=True),
                       "attention_mask": b["attention_mask"].to(device, non_blocking=True),
                       "token_type_ids": b["segment_ids"].to(device, non_blocking=True),
                       "img_feats": torch.cat(feats, 0).float().contiguous()})
    return blocks


def _qar_layout(questions):
    n_ans, n_rats = questions[0]["n_ans"], questions[0]["n_rats"]
    if any(q["n_ans"] != n_ans or q["n_rats"] != n_rats for q in questions):
        raise ValueError("VCR Q->AR: every question of a pass needs the same numbers of answers and rationales")
    return n_ans, n_rats


def val_vcr_qar(model, questions, device, batch_questions=4, trim=False, bucket=False, resident=None):
    """Evaluation pass of vcr_qar_nsp_cpt.py:605-703 (evaluate) on VCRQAR_NSPCPT.  questions: prompts.assemble_vcr_qar dicts with ``img_feats``
    (Li, D).  Questions are sharded over ranks (whole questions per rank); per batch ONE encoder pass runs over both blocks (qar_forward) and the
    choice runs on the device (cpt_vcr_qar_choose); the fixed-shape (n_q, 2) predictions, (n_q, 3) flags and (n_q, n_ans + n_rats) choice scores
    are gathered to every rank.  Accuracies follow the reference: results de-duplicated by questionId (last wins), divided by the number of
    questions; "q_ar" is the reference's "Eval Accuracy".  Returns {"preds", "flags", "scores", "q_ids", "acc": {"q_a", "qa_r", "q_ar"}}.
    trim / bucket: see the top of this module.
    resident: a ResidentSet of these questions (resident.upload(resident.from_vcr_qar(questions), device)): both blocks of a batch are gathered on
    the device by one launch, only ``n_ans``, ``n_rats``, ``label`` and ``q_id`` of the questions are read."""
    model.eval()
    n_ans, n_rats = _qar_layout(questions)
    plans = {}

    def groups_of(lo, hi):
        if resident is not None:
            sf = resident.seq_first
            if resident.tables.get("n_ans") != [n_ans] * len(questions):
                raise ValueError("val_vcr_qar: the resident set was not built from Q->AR questions of %d answers (resident.from_vcr_qar)" % n_ans)
            groups, found = _resident_walk(resident, model, len(questions), len(questions) * (n_ans + n_rats), lo, hi, batch_questions, bucket, None,
                                           trim, device, "val_vcr_qar", order=lambda g: rsd.qar_order(sf, n_ans, [lo + i for i in g]))
            plans.update(found)
            return groups
        keys = None
        if bucket:
            keys = [max(_item_length(q[part]["input_mask"], q[part]["input_ids"].shape[1]) for part in ("q_a", "qa_r")) for q in questions[lo:hi]]
        return _walk(hi - lo, batch_questions, keys)

    def step(idx, lo):
        chunk = [questions[lo + i] for i in idx]
        if resident is not None:                # one launch for both blocks: rows [0, B0) are the Q->A block, the others the QA->R block
            b = resident.gather(*plans[idx[0]], mask_pos=False)
            B0 = len(chunk) * n_ans
            qa, qr = ({"input_ids": b["input_ids"][r], "attention_mask": b["attention_mask"][r], "token_type_ids": b["segment_ids"][r],
                       "img_feats": b["img_feats"][r]} for r in (slice(0, B0), slice(B0, None)))
        else:
            qa, qr = _qar_blocks(chunk, device, trim)
        _, _, sc = model.qar_forward(qa, qr, return_scores=True)
        nq = len(chunk)
        B0 = nq * n_ans
        p, f = scoring.vcr_qar_choose_device(sc[:B0], sc[B0:], [q["label"][0] for q in chunk], [q["label"][1] for q in chunk], n_ans, n_rats)
        return p, f, torch.cat([sc[:B0].view(nq, n_ans), sc[B0:].view(nq, n_rats)], 1)

    n = len(questions)
    outputs = [((2,), torch.int64, -1), ((3,), torch.uint8, 0), ((n_ans + n_rats,), torch.float32, 0)]
    preds, flags, scores = (t.cpu() for t in _eval_pass(n, groups_of, outputs, step, device, bucket))
    q_ids = [q["q_id"] for q in questions]
    acc = dict(zip(("q_a", "qa_r", "q_ar"), _dedup_accuracy(flags, q_ids, n)))
    return {"preds": preds, "flags": flags, "scores": scores, "q_ids": q_ids, "acc": acc}


def qar_accumulation(n_examples, per_gpu_train_batch_size, world_size, n_batches, num_train_epochs=1, max_steps=0):
    """vcr_qar_nsp_cpt.py:399-407 and gqa_cpt.py:328-334: gradient_accumulation_steps = max(1, len(dataset) // (per_gpu_bs * world)) -- one
    optimizer step per epoch -- and t_total (max_steps, else len(dataloader) // gradient_accumulation_steps * num_train_epochs).  Returns
    (gradient_accumulation_steps, t_total)."""
    gas = max(1, n_examples // (per_gpu_train_batch_size * world_size))
    t_total = max_steps if max_steps > 0 else n_batches // gas * num_train_epochs
    return gas, t_total


gqa_accumulation = qar_accumulation


def train_vcr_qar_batch(model, optimizer, scheduler, batches, opts, device, global_step=0, trim=False):
    """One epoch of vcr_qar_nsp_cpt.py:453-525 over ``batches`` (lists of prompts.assemble_vcr_qar dicts with img_feats, one list per micro-step):
    class-0 labels of both blocks (qar_choice_labels), loss = q_a_loss + qa_r_loss from ONE encoder pass (qar_forward), divided by
    opts.gradient_accumulation_steps when that is > 1, backward, torch.nn.utils.clip_grad_norm_(model.parameters(), opts.max_grad_norm) on EVERY
    micro-step (in place on the accumulated gradient, as the reference), and every gradient_accumulation_steps micro-steps scheduler.step() BEFORE
    optimizer.step(), then model.zero_grad() (_accumulate, with the host clip).  Micro-steps that do not complete a window take no optimizer step
    and their gradient is kept (the reference zeroes only after a step).  Returns (global_step, [loss tensors, as divided]).
    trim: length-aware training (both blocks of a micro-step cut to ONE extent, _qar_blocks), see the top of this module."""
    model.train()

    def micro():
        for chunk in batches:
            n_ans, n_rats = _qar_layout(chunk)
            qa, qr = _qar_blocks(chunk, device, trim)
            la, lr_ = scoring.qar_choice_labels([q["label"][0] for q in chunk], [q["label"][1] for q in chunk], n_ans, n_rats)
            yield model.qar_forward(qa, qr, la, lr_)[0]
    global_step, losses, _ = _accumulate(model, optimizer, scheduler, micro(), opts, global_step, use_device_clip=False)
    return global_step, losses


# ---- GQA-CPT (Oscar/oscar/fewshot/gqa_cpt.py; BASELINE config 4) and VCR Q->A (fewshot/vcr_nsp_cpt.py; config 5) -----------------------------
def val_gqa(model, questions, labels, tokenizer, device, batch_questions=256, trim=False, bucket=False, resident=None):
    """Evaluation pass of gqa_cpt.py:558-636 (evaluate) on REC_MLM_CPT.  questions: prompts.assemble_gqa dicts with ``img_feats`` (Li, D) and
    ``igt``, the question's ground-truth label indices (eval_dic[str(q_id)]); labels: the data set's answer strings.  Questions are sharded over
    ranks; per batch ONE forward scores the label columns only (vocab_columns = every label's first word-piece id, duplicates kept) at the first
    [MASK] slot, and the argmax, the multi-ground-truth correctness and their count run in one launch (cpt_gqa_choose); the fixed-shape
    predictions, flags and (n, C) logits are gathered to every rank.  Accuracy as the reference: results de-duplicated by question_id (last
    wins), divided by the number of questions.  Returns {"preds" (n,) label columns, "answers" [the first-piece strings the reference reports],
    "correct" (n,) uint8, "logits" (n, C), "q_ids", "acc"}.  trim / bucket: see the top of this module.
    resident: a ResidentSet of these questions (resident.upload(resident.from_questions(questions), device)): the batches are gathered on the
    device, only ``igt`` and ``q_id`` of the questions are read."""
    model.eval()
    plans = {}
    token_ids, label_sid, piece_sid = scoring.gqa_string_ids(labels, tokenizer)
    _, answer_labels = scoring.gqa_first_pieces(labels, tokenizer)
    C = len(labels)
    cols = torch.tensor(token_ids, dtype=torch.int64, device=device)
    piece = torch.tensor(piece_sid, dtype=torch.int32, device=device)
    gt_all = scoring.gqa_gt_table([q["igt"] for q in questions], label_sid)
    t = lambda x: torch.as_tensor(x)

    def groups_of(lo, hi):
        if resident is not None:
            groups, found = _resident_walk(resident, model, len(questions), len(questions), lo, hi, batch_questions, bucket, None, trim, device,
                                           "val_gqa")
            plans.update(found)
            return groups
        return _walk(hi - lo, batch_questions, [_item_length(np.asarray(q["input_mask"])[None], np.asarray(q["input_ids"]).shape[0])
                                                for q in questions[lo:hi]] if bucket else None)

    def step(idx, lo):
        if resident is not None:
            b = resident.gather(*plans[idx[0]])
            sc = model(b["input_ids"], b["segment_ids"], b["attention_mask"], img_feats=b["img_feats"], mask_token_pos=b["mask_token_pos"],
                       vocab_columns=cols)[0]
            p, c = scoring.gqa_choose_device(sc, piece, gt_all[torch.as_tensor(idx) + lo])
            return p, c, sc
        chunk = [questions[lo + i] for i in idx]
        b = {"input_ids": torch.stack([t(q["input_ids"]) for q in chunk]), "segment_ids": torch.stack([t(q["segment_ids"]) for q in chunk]),
             "attention_mask": torch.stack([t(q["input_mask"]) for q in chunk]), "img_feats": torch.stack([t(q["img_feats"]) for q in chunk])}
        mpos = torch.tensor([int(q["mask_token_pos"][0]) for q in chunk], dtype=torch.int64)    # raw_batch[-1][0]
        if trim:
            b = _trim_host(b, mpos)[0]
        ids, seg, msk = (b[k].to(device, non_blocking=True) for k in ("input_ids", "segment_ids", "attention_mask"))
        feats = b["img_feats"].to(device, non_blocking=True).float()
        mpos = mpos.to(device, non_blocking=True)
        sc = model(ids, seg, msk, img_feats=feats, mask_token_pos=mpos, vocab_columns=cols)[0]
        p, c = scoring.gqa_choose_device(sc, piece, gt_all[torch.as_tensor(idx) + lo])
        return p, c, sc

    n = len(questions)
    outputs = [((), torch.int64, -1), ((), torch.uint8, 0), ((C,), torch.float32, 0)]
    preds, correct, logits = (r.cpu() for r in _eval_pass(n, groups_of, outputs, step, device, bucket))
    q_ids = [int(t(q["q_id"]).reshape(-1)[0]) for q in questions]
    acc = _dedup_accuracy(correct, q_ids, n)
    return {"preds": preds, "answers": [answer_labels[int(p)] for p in preds.tolist()], "correct": correct, "logits": logits, "q_ids": q_ids,
            "acc": acc}


def gqa_label_grid(input_ids, attention_mask, label_id, label_token_ids):
    """gqa_cpt.py:428-435: a grid of -1 shaped like attention_mask (B, Lt + Li) with label_token_ids[label] at EVERY input_ids == 103 slot
    ([MASK]); label_id (B,) or (B, 1) the first ground-truth label of each question.  The slots are taken in row-major order and the labels in
    batch order, as the reference's index assignment pairs them: a batch whose sequences do not hold exactly one [MASK] each raises, as the
    assignment does there."""
    grid = torch.full(attention_mask.shape, -1, dtype=torch.long, device=input_ids.device)
    want = label_token_ids.to(input_ids.device)[label_id.to(input_ids.device).long().reshape(-1)]
    idx = (input_ids == 103).nonzero(as_tuple=False)
    if idx.size(0) != want.numel():
        raise RuntimeError("GQA label grid: %d [MASK] slots for %d labels" % (idx.size(0), want.numel()))
    grid[idx[:, 0], idx[:, 1]] = want
    return grid


def set_dropout(model, p):
    """The adjust_dp switch of gqa_cpt.py:403-412 (0.3 from epoch 3 on): the reference sets ``p`` of model.dropout, model.bert.dropout and
    model.bert.embeddings.dropout.  Here the training step draws its masks from config.hidden_dropout_prob (train.dropout_for), one rate for
    every hidden dropout of the step, so that is set too: the next training forward's cpt_dropout carries it."""
    model.config.hidden_dropout_prob = float(p)
    for owner in (model, getattr(model, "bert", None), getattr(getattr(model, "bert", None), "embeddings", None)):
        d = getattr(owner, "dropout", None)
        if isinstance(d, torch.nn.Dropout):
            d.p = float(p)


def _accumulate(model, optimizer, scheduler, micro_losses, opts, global_step, use_device_clip=None):
    """The accumulation loop of train_gqa_batch, train_vcr_batch and train_vcr_qar_batch (gqa_cpt.py:445-462, vcr_nsp_cpt.py:452-473,
    vcr_qar_nsp_cpt.py:453-525).  micro_losses yields one loss per micro-step; it is
    divided by gradient_accumulation_steps when that is > 1, backward and the global-norm clip run on EVERY micro-step (in place on the
    accumulated gradient), and every gradient_accumulation_steps micro-steps scheduler.step() runs BEFORE optimizer.step(), then
    model.zero_grad().  The clip is optimizer.clip_grad_norm_device (no host synchronisation) when the optimizer has it -- use_device_clip=False
    forces torch.nn.utils.clip_grad_norm_.  Returns (global_step, [loss tensors, as divided], [gradient norms before each clip])."""
    gas = max(1, int(getattr(opts, "gradient_accumulation_steps", 1)))
    max_norm = float(getattr(opts, "max_grad_norm", 1.0))
    if use_device_clip is None:
        use_device_clip = hasattr(optimizer, "clip_grad_norm_device")
    losses, norms = [], []
    for step, loss in enumerate(micro_losses):
        if gas > 1:
            loss = loss / gas
        loss.backward()
        if use_device_clip:
            norms.append(optimizer.clip_grad_norm_device(max_norm))
        else:
            norms.append(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm))
        losses.append(loss.detach())
        if (step + 1) % gas == 0:
            scheduler.step()
            optimizer.step()
            model.zero_grad()
            global_step += 1
    return global_step, losses, norms


def train_gqa_batch(model, optimizer, scheduler, batches, opts, device, label_token_ids, global_step=0, use_device_clip=None, trim=False):
    """One epoch of gqa_cpt.py:423-462 over ``batches``: dicts with input_ids (B, Lt), attention_mask (B, Lt + Li), segment_ids, img_feats
    (B, Li, D) and label_id (B,) or (B, 1).  Label grid of gqa_label_grid, loss / gradient_accumulation_steps, backward and clip on every
    micro-step, scheduler before optimizer, model.zero_grad() after (_accumulate).  use_device_clip: None = optimizer.clip_grad_norm_device when
    the optimizer has it, False = torch.nn.utils.clip_grad_norm_.  Returns (global_step, [loss tensors, as divided]).
    trim: length-aware training, see the top of this module."""
    global_step, losses, _ = _gqa_pass(model, optimizer, scheduler, batches, opts, device, label_token_ids, global_step, use_device_clip, trim)
    return global_step, losses


def _gqa_pass(model, optimizer, scheduler, batches, opts, device, label_token_ids, global_step, use_device_clip, trim=False):
    model.train()
    # the label grid is built where the batch is when grid_fn runs (_device_batch): on the host with trim, on the device without -- the token
    # table the lambda below closes over lives on that side
    label_token_ids = torch.as_tensor(label_token_ids, dtype=torch.long)
    if not trim:
        label_token_ids = label_token_ids.to(device)

    def micro():
        for host_batch in batches:
            b, grid = _device_batch(host_batch, lambda x: gqa_label_grid(x["input_ids"], x["attention_mask"], x["label_id"], label_token_ids),
                                    device, trim)
            yield model(b["input_ids"], b["segment_ids"], b["attention_mask"], img_feats=None if b["img_feats"] is None else b["img_feats"].float(),
                        masked_lm_labels=grid)[0]
    return _accumulate(model, optimizer, scheduler, micro(), opts, global_step, use_device_clip)


def _vcr_block(chunk, device, trim=False):
    """Questions (prompts.assemble_vcr dicts + ``img_feats`` (Li, D)) concatenated in vcr_collate_fn's layout: one row per answer choice.
    trim: the host arrays are cut to the batch extent first, and only the first Li' regions of every image are moved."""
    t = lambda x: torch.as_tensor(x)
    interval = chunk[0]["input_ids"].shape[0]
    if any(q["input_ids"].shape[0] != interval for q in chunk):
        raise ValueError("VCR Q->A: every question of a pass needs the same number of answer choices")
    b = {"input_ids": torch.cat([t(q["input_ids"]) for q in chunk], 0), "attention_mask": torch.cat([t(q["input_mask"]) for q in chunk], 0),
         "segment_ids": torch.cat([t(q["segment_ids"]) for q in chunk], 0)}
    li = None
    if trim:
        b, li = _trim_host(b)
    return {"input_ids": b["input_ids"].to(device, non_blocking=True),
            "attention_mask": b["attention_mask"].to(device, non_blocking=True),
            "token_type_ids": b["segment_ids"].to(device, non_blocking=True),
            "img_feats": torch.cat([_seq_feats(q["img_feats"], interval, device, li) for q in chunk], 0).float().contiguous()}, interval


def _vcr_label(q):
    lb = q["label"]
    return int(lb[0] if isinstance(lb, (list, tuple)) else lb)


def val_vcr(model, questions, device, batch_questions=8, trim=False, bucket=False, resident=None):
    """Evaluation pass of vcr_nsp_cpt.py:583-620 (evaluate) on NSPCPT.  questions: prompts.assemble_vcr dicts with ``img_feats`` (Li, D).
    Questions are sharded over ranks (whole questions per rank); per batch one forward gives the relation scores and ONE launch
    (cpt_nsp_choose) the choice scores 1 - softmax(rel)[:, 1], each question's argmax and its correctness; the fixed-shape predictions, flags
    and (n_q, interval) choice scores are gathered to every rank.  Accuracy as the reference: results de-duplicated by questionId (last wins),
    divided by the number of questions.  Returns {"preds" (n_q,), "correct" (n_q,) uint8, "scores" (n_q, interval), "q_ids", "acc"}.
    trim / bucket: see the top of this module.
    resident: a ResidentSet of these questions (resident.upload(resident.from_vcr(questions), device)): the batches are gathered on the device,
    only ``label`` and ``q_id`` of the questions are read (and the number of choices comes from the set)."""
    model.eval()
    plans = {}
    if resident is not None:
        counts = np.diff(resident.seq_first)
        interval = int(counts[0]) if counts.size else 0
        if bool((counts != interval).any()):
            raise ValueError("VCR Q->A: every question of a pass needs the same number of answer choices")
    else:
        interval = questions[0]["input_ids"].shape[0]

    def groups_of(lo, hi):
        if resident is not None:
            groups, found = _resident_walk(resident, model, len(questions), len(questions) * interval, lo, hi, batch_questions, bucket, None, trim,
                                           device, "val_vcr")
            plans.update(found)
            return groups
        return _walk(hi - lo, batch_questions, [_item_length(q["input_mask"], q["input_ids"].shape[1]) for q in questions[lo:hi]] if bucket else None)

    def step(idx, lo):
        chunk = [questions[lo + i] for i in idx]
        if resident is not None:
            b = resident.gather(*plans[idx[0]], mask_pos=False)
            b["token_type_ids"] = b["segment_ids"]
        else:
            b, iv = _vcr_block(chunk, device, trim)
            if iv != interval:
                raise ValueError("VCR Q->A: every question of a pass needs the same number of answer choices")
        rel = model(b["input_ids"], b["token_type_ids"], b["attention_mask"], img_feats=b["img_feats"])[0]
        sc, p, c = scoring.nsp_choose_device(rel, interval, [_vcr_label(q) for q in chunk])
        return p, c, sc.view(len(chunk), interval)

    n = len(questions)
    outputs = [((), torch.int64, -1), ((), torch.uint8, 0), ((interval,), torch.float32, 0)]
    preds, correct, scores = (t.cpu() for t in _eval_pass(n, groups_of, outputs, step, device, bucket))
    q_ids = [int(q["q_id"]) for q in questions]
    acc = _dedup_accuracy(correct, q_ids, n)
    return {"preds": preds, "correct": correct, "scores": scores, "q_ids": q_ids, "acc": acc}


def train_vcr_batch(model, optimizer, scheduler, batches, opts, device, global_step=0, use_device_clip=None, trim=False):
    """One epoch of vcr_nsp_cpt.py:430-473 over ``batches`` (lists of prompts.assemble_vcr dicts with img_feats, one list per micro-step, one
    ``interval`` per pass): class 0 at each question's correct choice and 1 elsewhere (scoring.nsp_choice_labels), the NSP loss, and the
    accumulation loop of train_gqa_batch (_accumulate).  Returns (global_step, [loss tensors, as divided]).
    trim: length-aware training (the extent from the mask alone: the loss reads [CLS]), see the top of this module."""
    global_step, losses, _ = _vcr_pass(model, optimizer, scheduler, batches, opts, device, global_step, use_device_clip, trim)
    return global_step, losses


def _vcr_pass(model, optimizer, scheduler, batches, opts, device, global_step, use_device_clip, trim=False):
    model.train()
    batches = list(batches)
    interval = batches[0][0]["input_ids"].shape[0] if batches else 0

    def micro():
        for chunk in batches:
            b, iv = _vcr_block(chunk, device, trim)
            if iv != interval:
                raise ValueError("VCR Q->A: one interval per pass (got %d after %d)" % (iv, interval))
            cls_labels = scoring.nsp_choice_labels([_vcr_label(q) for q in chunk], interval, len(chunk) * interval, device)
            yield model(b["input_ids"], b["token_type_ids"], b["attention_mask"], next_sentence_label=cls_labels, img_feats=b["img_feats"])[0]
    return _accumulate(model, optimizer, scheduler, micro(), opts, global_step, use_device_clip)
