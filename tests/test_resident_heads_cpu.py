"""CPU: the head tables of the device-resident sets (cpt_amd/resident.py: from_pairs, from_vcr, from_vcr_qar, from_train_batches) -- their numpy
gather against the host path they replace (drivers._vg_cat, _vcr_block, _qar_blocks, _device_batch with _label_grid / vg_label_grid, all on the
CPU device) on every batch of every walk, the head rows, the labels and the label grid included; the extents against batching; the refusals; the
drivers with a set reading no tensor of the items; the binding of cpt_gather_batch_heads.  Everything is equality.  The item builders are shared
with tests/test_gpu_resident_heads.py."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import test_gpu_trim_drivers as T
import test_resident_cpu as RC
from cpt_amd import batching as BT
from cpt_amd import drivers
from cpt_amd import resident as R
from cpt_amd import scoring as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
LT, LI, D = RC.LT, RC.LI, RC.D
WALKS = [dict(), dict(trim=True), dict(bucket=True), dict(trim=True, bucket=True)]
BATCH_KEYS = ("input_ids", "segment_ids", "attention_mask")


# ---- item builders ----------------------------------------------------------------------------------------------------------------------------
def _block(rng, regions, Li, dim):
    f = np.zeros((Li, dim), np.float32)
    f[:regions] = rng.standard_normal((regions, dim)).astype(np.float32)
    return torch.from_numpy(f)


def vg_pairs(Lt=LT, Li=LI, dim=D, seed=0, n=7, train=False):
    """VG-layout pairs: 6 sequences (3 with train) whose sequence s holds s % 3 + 1 head rows, ragged text lengths and region counts, and two
    pairs of one image sharing ONE (Li, D) feature array."""
    rng = np.random.Generator(np.random.PCG64(seed))
    P = 3 if train else 6
    out, feats, regions = [], None, 0
    for i in range(n):
        if i % 2 == 0:
            regions = int(rng.integers(0, Li + 1))
            feats = _block(rng, regions, Li, dim)
        q = {"img_key": "%d.jpg_%d_%d" % (10 + i // 2, i % 3, (i + 1) % 3), "input_ids": torch.zeros((P, Lt), dtype=torch.int64),
             "segment_ids": torch.zeros((P, Lt), dtype=torch.int64), "attention_mask": torch.zeros((P, Lt + Li), dtype=torch.int64), "img_feats": feats}
        rows = []
        for s in range(P):
            k = s % 3 + 1
            t = int(rng.integers(k + 3, Lt + 1))
            q["input_ids"][s, :t] = torch.from_numpy(rng.integers(1, 30000, t))
            q["segment_ids"][s, t // 2:t] = 1
            q["attention_mask"][s, :t] = 1
            q["attention_mask"][s, Lt:Lt + regions] = 1
            first = int(rng.integers(1, t - k))
            rows += [[s, first + j] for j in range(k)]
        q["mask_token_pos"] = torch.tensor(rows, dtype=torch.int64)
        if train:
            q["row_labels"] = torch.from_numpy(rng.integers(5, 500, len(rows)))
        out.append(q)
    return out


def vcr_questions(n=7, seed=3):
    """The VCR Q->A questions of tests/test_gpu_trim_drivers.py::test_val_vcr_options."""
    from cpt_amd import prompts
    import test_gpu_gqa_vcr as G
    tok = G._tok()
    rng, colors, names, sent = T._vcr_parts(seed)
    qs = []
    for q in range(n):
        k = int(rng.integers(2, T.LI + 1))
        d = prompts.assemble_vcr(tok, sent(int(rng.integers(2, 6))), [sent(int(rng.integers(1, 5))) for _ in range(4)], colors, names, k,
                                 label=q % 4, q_id=100 + q, max_seq_length=T.LT, max_img_seq_length=T.LI)
        d["img_feats"] = T._feats(rng, k, G._cfg().img_feature_dim)
        qs.append(d)
    return qs


def qar_questions(n=5, seed=4):
    """The VCR Q->AR questions of tests/test_gpu_trim_drivers.py::test_val_vcr_qar_options."""
    from cpt_amd import prompts
    import test_gpu_vcr_qar as Q
    tok = Q._tok()
    rng, colors, names, sent = T._vcr_parts(seed)
    qs = []
    for q in range(n):
        k = int(rng.integers(2, T.LI + 1))
        d = prompts.assemble_vcr_qar(tok, sent(int(rng.integers(2, 5))), [sent(int(rng.integers(1, 4))) for _ in range(4)],
                                     [sent(int(rng.integers(1, 5))) for _ in range(4)], colors, names, k, label=(q % 4, (2 * q) % 4), q_id=100 + q,
                                     max_seq_length=T.LT, max_img_seq_length=T.LI)
        d["img_feats"] = T._feats(rng, k, Q._cfg().img_feature_dim)
        qs.append(d)
    return qs


def colour_batches(Lt=LT, Li=LI, dim=D, seed=6, n=3, B=4):
    """train_batch / tune_soft_template batch dicts: one [MASK] position and one colour per sequence; one position counted from the end, one label
    of -1, one position in the region part."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(n):
        qs = RC.ragged_queries(Lt=Lt, Li=Li, dim=dim, seed=seed + i, n=4)
        flat = {k: torch.cat([q[k] for q in qs], 0)[:B].clone() for k in RC.KEYS}
        flat["colors"] = torch.from_numpy(rng.integers(5, 500, B))
        if i == 0:
            flat["mask_token_pos"][1] = int(flat["mask_token_pos"][1]) - (Lt + Li)          # from the end: the same position
            flat["colors"][2] = -1
        if i == 1 and Li:
            flat["mask_token_pos"][0] = Lt + 1
        out.append(flat)
    return out


def vg_train_batches(Lt=LT, Li=LI, dim=D, seed=8, n=3):
    """train_vg_batch batch dicts: sequences of 0, 1 and 3 labelled rows in one batch, a label in the last attended text column, a label of -1, a
    labelled region column."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(n):
        qs = RC.ragged_queries(Lt=Lt, Li=Li, dim=dim, seed=seed + i, n=4)
        flat = {k: torch.cat([q[k] for q in qs], 0)[:5].clone() for k in BATCH_KEYS + ("img_feats",)}
        text = BT.extents(flat["attention_mask"], Lt)[0]
        rows = [[0, 1], [0, 2], [0, int(text[0]) - 1], [2, 1], [4, int(text[4]) - 1]]             # sequences 1 and 3 own no row
        if i == 1 and Li:
            rows.append([4, Lt + Li - 1])
        if i == 2:
            rows = rows[::-1]                                                                     # not in sequence order: the grid is the same
        flat["mask_token_pos"] = torch.tensor(rows, dtype=torch.int64)
        flat["row_labels"] = torch.from_numpy(rng.integers(5, 500, len(rows)))
        if i == 0:
            flat["row_labels"][1] = -1
        out.append(flat)
    return out


# ---- 1. gather_reference against the host path ------------------------------------------------------------------------------------------------
def _same_rows(got, want, where):
    for k in BATCH_KEYS:
        w = np.asarray(want[k if k in want else {"segment_ids": "token_type_ids"}[k]])
        assert got[k].dtype == np.int64 and np.array_equal(got[k], w), (where, k)
    if want["img_feats"] is None:                  # Li' = 0 under trim: the host step runs text-only
        assert got["img_feats"].shape[1] == 0, (where, "img_feats")
        return
    w = np.asarray(want["img_feats"], dtype=np.float32)
    assert got["img_feats"].shape == w.shape and np.array_equal(RC.bits(got["img_feats"]), RC.bits(w)), (where, "img_feats")


def _groups(t, host_keys, size, walk):
    assert R.item_keys(t) == host_keys
    groups = drivers._walk(len(host_keys), size, host_keys if walk.get("bucket") else None)
    assert sorted(i for g in groups for i in g) == list(range(len(host_keys)))
    return groups


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("train", [False, True])
def test_pairs_equal_vg_cat(walk, train):
    pairs = vg_pairs(train=train, n=7)
    P = 3 if train else 6
    t = R.tables(R.from_pairs(pairs))
    assert t["n_seq"] == P * len(pairs) and t["n_heads"] == (6 if train else 12) * len(pairs) and len(t["block_rows"]) == 4
    assert (t["head_label"] is not None) == train and t["seq_label"] is None
    sf = t["seq_first"]
    for g in _groups(t, [drivers._item_length(q["attention_mask"], LT) for q in pairs], 3, walk):
        seqs = np.concatenate([np.arange(sf[i], sf[i + 1]) for i in g])
        want = drivers._vg_cat([pairs[i] for i in g], CPU, P, bool(walk.get("trim")))
        mask = torch.cat([pairs[i]["attention_mask"] for i in g], 0)
        assert R.extent(t, seqs) == BT.batch_extent(mask, LT, want["mask_token_pos"])
        ext = R.extent(t, seqs) if walk.get("trim") else (LT, LI)
        got = R.gather_reference(t, seqs, *ext)
        _same_rows(got, want, g)
        assert got["head_rows"].dtype == np.int64 and np.array_equal(got["head_rows"], want["mask_token_pos"].numpy()), g
        first = R.row_first(t, seqs)
        assert first.dtype == np.int32 and first[-1] == len(got["head_rows"]) and np.array_equal(np.diff(first), [s % 3 + 1 for s in range(P)] * len(g))
        if train:
            assert np.array_equal(got["head_labels"], torch.cat([pairs[i]["row_labels"] for i in g]).numpy())


@pytest.mark.parametrize("walk", WALKS)
def test_vcr_questions_equal_vcr_block(walk):
    qs = vcr_questions()
    t = R.tables(R.from_vcr(qs))
    assert t["n_seq"] == 4 * len(qs) and t["n_heads"] == 0 and t["head_label"] is None and not t["head_first"].any()
    sf = t["seq_first"]
    for g in _groups(t, [drivers._item_length(q["input_mask"], T.LT) for q in qs], 2, walk):
        seqs = np.concatenate([np.arange(sf[i], sf[i + 1]) for i in g])
        want, interval = drivers._vcr_block([qs[i] for i in g], CPU, bool(walk.get("trim")))
        mask = torch.cat([torch.as_tensor(qs[i]["input_mask"]) for i in g], 0)
        assert R.extent(t, seqs) == BT.batch_extent(mask, T.LT) == BT.label_extent(mask, T.LT)
        got = R.gather_reference(t, seqs, *(R.extent(t, seqs) if walk.get("trim") else (T.LT, T.LI)))
        _same_rows(got, want, g)
        assert got["head_rows"].shape == (0, 2) and "label_grid" not in got
        assert np.array_equal(got["seq_label"], SC.nsp_choice_labels([qs[i]["label"] for i in g], interval, interval * len(g)).numpy())
    assert "seq_label" not in R.gather_reference(R.tables(R.from_vcr(qs, labels=False)), [0], 1, 0)


@pytest.mark.parametrize("walk", WALKS)
def test_qar_questions_equal_qar_blocks(walk):
    qs = qar_questions()
    t = R.tables(R.from_vcr_qar(qs))
    assert t["n_seq"] == 8 * len(qs) and t["n_heads"] == 0 and t["n_ans"] == [4] * len(qs) and len(t["block_rows"]) == len(qs)
    keys = [max(drivers._item_length(q[p]["input_mask"], T.LT) for p in ("q_a", "qa_r")) for q in qs]
    for g in _groups(t, keys, 2, walk):
        seqs = R.qar_order(t["seq_first"], 4, g)
        qa, qr = drivers._qar_blocks([qs[i] for i in g], CPU, bool(walk.get("trim")))
        want = {k: torch.cat([qa[k], qr[k]], 0) for k in qa}
        masks = [torch.cat([torch.as_tensor(qs[i][p]["input_mask"]) for i in g], 0) for p in ("q_a", "qa_r")]
        exts = [BT.batch_extent(m, T.LT) for m in masks]
        assert R.extent(t, seqs) == (max(e[0] for e in exts), max(e[1] for e in exts))
        got = R.gather_reference(t, seqs, *(R.extent(t, seqs) if walk.get("trim") else (T.LT, T.LI)))
        _same_rows(got, want, g)
        la, lr = SC.qar_choice_labels([qs[i]["label"][0] for i in g], [qs[i]["label"][1] for i in g], 4, 4)
        assert np.array_equal(got["seq_label"], torch.cat([la, lr]).numpy())


def _regroup(batches, lists, sf):
    """The host batch dicts of the index lists ``lists``: the rows of the batches the set was built from, regrouped."""
    flat = {k: torch.cat([b[k] for b in batches], 0) for k in BATCH_KEYS + ("img_feats",)}
    out = []
    for idx in lists:
        rows = torch.as_tensor(np.asarray(idx, np.int64))
        nb = {k: flat[k][rows] for k in flat}
        if "colors" in batches[0]:
            nb["mask_token_pos"] = torch.cat([b["mask_token_pos"] for b in batches])[rows]
            nb["colors"] = torch.cat([b["colors"] for b in batches])[rows]
        else:
            pos, lab = [], []
            for j, s in enumerate(np.asarray(idx).tolist()):
                i = int(np.searchsorted(sf, s, side="right")) - 1
                mine = batches[i]["mask_token_pos"][:, 0] == s - int(sf[i])
                pos.append(torch.stack([torch.full((int(mine.sum()),), j), batches[i]["mask_token_pos"][mine, 1]], 1))
                lab.append(batches[i]["row_labels"][mine])
            nb["mask_token_pos"], nb["row_labels"] = torch.cat(pos), torch.cat(lab)
        out.append(nb)
    return out


@pytest.mark.parametrize("trim", [False, True])
@pytest.mark.parametrize("kind", ["colours", "vg"])
def test_train_batches_equal_device_batch(kind, trim):
    batches, grid_fn = (colour_batches(), drivers._label_grid) if kind == "colours" else (vg_train_batches(), drivers.vg_label_grid)
    t = R.tables(R.from_train_batches(batches))
    assert t["whole"] and t["n_items"] == len(batches) and t["head_label"] is not None
    sf = t["seq_first"]
    S = int(sf[-1])
    own = [np.arange(sf[i], sf[i + 1]) for i in range(len(batches))]
    rng = np.random.Generator(np.random.PCG64(1))
    perm = rng.permutation(S)
    regrouped = [perm[:3], perm[3:4], perm[4:]]
    for lists, host in ((own, batches), (regrouped, _regroup(batches, regrouped, sf))):
        for idx, hb in zip(lists, host):
            want, grid = drivers._device_batch(hb, grid_fn, CPU, trim)
            full = grid_fn({k: torch.as_tensor(v) for k, v in hb.items()})
            assert R.extent(t, idx, labelled=True) == BT.label_extent(hb["attention_mask"], LT, full)
            ext = R.extent(t, idx, labelled=True) if trim else (LT, LI)
            got = R.gather_reference(t, idx, *ext)
            _same_rows(got, want, idx)
            assert got["label_grid"].dtype == np.int64 and np.array_equal(got["label_grid"], grid.numpy()), idx
            assert np.array_equal(got["label_grid"], BT.trim_grid(full, LT, *ext).numpy())
            assert len(got["head_rows"]) == len(got["head_labels"]) == R.row_first(t, idx)[-1]
    if kind == "vg":                        # sequences of 0, 1 and 3 rows in one batch: row_first has equal neighbours
        assert np.diff(R.row_first(t, own[0])).tolist() == [3, 0, 1, 0, 1]
        assert R.gather_reference(t, [1, 3], LT, LI)["head_rows"].shape == (0, 2) and (R.gather_reference(t, [1, 3], LT, LI)["label_grid"] == -1).all()
    assert R.store_bytes(t) == sum(t[k].nbytes for k in ("ids", "seg", "mask", "mask_pos", "feat_block", "block_rows", "block_off", "head_first",
                                                          "head_pos", "head_label")) + t["feats"].shape[0] * R.pitch_of(D, "fp32") * 4


# ---- 2. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    def vg(change):
        bs = vg_train_batches()
        change(bs)
        return R.tables(R.from_train_batches(bs))

    def put(i, key, value):
        def run(bs):
            bs[i][key] = value
        return run
    with pytest.raises(ValueError, match="same position"):
        vg(put(0, "mask_token_pos", torch.tensor([[0, 1], [0, 2], [0, 1], [2, 1], [4, 1]])))
    with pytest.raises(ValueError, match="outside the padded"):
        vg(put(0, "mask_token_pos", torch.tensor([[0, 1], [0, 2], [0, LT + LI], [2, 1], [4, 1]])))
    with pytest.raises(ValueError, match="outside the padded"):             # from the end, past the start
        vg(put(0, "mask_token_pos", torch.tensor([[0, 1], [0, 2], [0, -(LT + LI) - 1], [2, 1], [4, 1]])))
    with pytest.raises(ValueError, match="names sequence"):
        vg(put(0, "mask_token_pos", torch.tensor([[0, 1], [0, 2], [5, 3], [2, 1], [4, 1]])))
    with pytest.raises(ValueError, match="labels"):
        vg(put(0, "row_labels", torch.tensor([1, 2, 2 ** 31, 4, 5])))
    with pytest.raises(ValueError, match="labels"):
        vg(put(0, "row_labels", torch.tensor([1, 2, 3, 4])))
    for key, cut in (("input_ids", (slice(None), slice(0, LT - 1))), ("attention_mask", (slice(None), slice(0, LT + LI - 1)))):
        with pytest.raises(ValueError, match="padded"):                      # another Lt, another Li
            vg(lambda bs: bs[1].update({key: bs[1][key][cut]}))
    with pytest.raises(ValueError, match="dimension"):                       # another D
        vg(lambda bs: bs[1].update(img_feats=bs[1]["img_feats"][:, :, :-1]))
    with pytest.raises(ValueError, match="same position"):
        R.tables(R.from_train_batches([dict(colour_batches()[0], mask_token_pos=torch.tensor([[0, 1], [0, 1], [1, 1], [2, 1]]))], labels="colors"))
    pairs = vg_pairs(n=2)
    pairs[1]["mask_token_pos"] = pairs[1]["mask_token_pos"].flip(0)
    with pytest.raises(ValueError, match="sequence order"):
        R.from_pairs(pairs)
    mixed = vg_pairs(n=2, train=True)
    del mixed[1]["row_labels"]
    with pytest.raises(ValueError, match="row_labels"):
        R.from_pairs(mixed)
    t = R.tables(R.from_vcr(vcr_questions(n=2)))
    with pytest.raises(ValueError):
        R.gather_reference(t, [t["n_seq"]], 1, 0)


# ---- 3. the drivers read no tensor of the items -----------------------------------------------------------------------------------------------
class _Untouchable(object):
    def _no(self, *a, **kw):
        raise AssertionError("a driver with a resident set read a tensor of an item")
    __getattr__ = __getitem__ = __len__ = __iter__ = __array__ = _no


def _hollow(item):
    return {k: _hollow(v) if isinstance(v, dict) else (_Untouchable() if isinstance(v, (np.ndarray, torch.Tensor)) else v) for k, v in item.items()}


def fake_set(t, device=CPU):
    """A ResidentSet whose gather is resident.gather_reference on the host tables: what the launch writes, as tensors on ``device``."""
    rs = R.ResidentSet({k: v for k, v in t.items() if k != "feats"}, device, "fp32", {}, object(), object())
    rs.launches = []

    def gather(seq_idx, Lt_out, Li_out, mask_pos=True, out=None, row_first=None, R_=0, heads=None, **kw):
        R_ = kw.get("R", R_)
        ref = R.gather_reference(t, seq_idx.cpu().numpy(), Lt_out, Li_out)
        if heads is not None and ("head_rows" in heads or "head_labels" in heads):
            assert np.array_equal(row_first.cpu().numpy(), R.row_first(t, seq_idx.cpu().numpy())) and R_ == len(ref["head_rows"])
        rs.launches.append((seq_idx.numel(), Lt_out, Li_out))
        keep = RC.KEYS + tuple(heads or ())
        res = {k: torch.from_numpy(v).to(device) for k, v in ref.items() if k in keep}
        if not mask_pos:
            res["mask_token_pos"] = None
        return res
    rs.gather = gather
    return rs


class _Engine(object):
    dtype = "fp32"


def _sig(ids, mask, feats):
    """One number per sequence out of everything a batch holds."""
    return ids.double().sum(1) * 1e-3 + mask.double().sum(1) * 3 + feats.double().sum((1, 2))


@pytest.mark.parametrize("walk", WALKS)
def test_eval_drivers_with_a_set_read_no_item_tensor(walk, monkeypatch):
    model = types.SimpleNamespace(eval=lambda: None, _engine=lambda: _Engine())
    idx2pred = {1: [3], 2: [4, 5]}

    def vg_scores(m, ids, seg, mask, feats, pos, idx2pred_):
        s = _sig(ids, mask, feats).index_add(0, pos[:, 0], pos[:, 1].double() * 7)
        return (s.view(-1, 2, 3).sum(-1)[..., None] * torch.arange(1, 4, dtype=torch.float64)).float()
    monkeypatch.setattr(SC, "vg_predicate_scores", vg_scores)
    pairs = vg_pairs()
    want = drivers.val_vg(model, pairs, idx2pred, CPU, batch_pairs=3, **walk)
    rs = fake_set(R.tables(R.from_pairs(pairs)))
    got = drivers.val_vg(model, [_hollow(q) for q in pairs], idx2pred, CPU, batch_pairs=3, resident=rs, **walk)
    assert torch.equal(got[0], want[0]) and got[1] == want[1] and len(rs.launches) == 3 and bool(want[0].any())
    if walk.get("trim"):
        assert any(lt + li < LT + LI for _, lt, li in rs.launches)

    def nsp(rel, interval, labels):
        n = rel.size(0) // interval
        sc = rel[:, 0]
        p = sc.view(n, interval).argmax(1)
        return sc, p, (p == torch.tensor(labels)).to(torch.uint8)
    monkeypatch.setattr(SC, "nsp_choose_device", nsp)
    vcr_model = types.SimpleNamespace(eval=lambda: None, _engine=lambda: _Engine())
    forward = lambda ids, tt, mask, img_feats=None: (torch.stack([_sig(ids, mask, img_feats).float() + tt.sum(1), mask.sum(1).float()], 1),)
    qs = vcr_questions()
    rs = fake_set(R.tables(R.from_vcr(qs)))
    want = drivers.val_vcr(_Callable(vcr_model, forward), qs, CPU, batch_questions=2, **walk)
    got = drivers.val_vcr(_Callable(vcr_model, forward), [_hollow(q) for q in qs], CPU, batch_questions=2, resident=rs, **walk)
    _equal_results(got, want)
    assert len(rs.launches) == 4

    def qar_choose(sa, sr, la, lr, n_ans, n_rats):
        pa, pr = sa.view(-1, n_ans).argmax(1), sr.view(-1, n_rats).argmax(1)
        ok = torch.stack([pa == torch.tensor(la), pr == torch.tensor(lr)], 1)
        return torch.stack([pa, pr], 1), torch.cat([ok, ok.all(1, keepdim=True)], 1).to(torch.uint8)
    monkeypatch.setattr(SC, "vcr_qar_choose_device", qar_choose)

    def qar_forward(qa, qr, return_scores=False):
        sc = torch.cat([_sig(b["input_ids"], b["attention_mask"], b["img_feats"]).float() * (k + 1) + b["token_type_ids"].sum(1)
                        for k, b in enumerate((qa, qr))])
        return None, None, sc
    qar_model = types.SimpleNamespace(eval=lambda: None, _engine=lambda: _Engine(), qar_forward=qar_forward)
    qs = qar_questions()
    rs = fake_set(R.tables(R.from_vcr_qar(qs)))
    want = drivers.val_vcr_qar(qar_model, qs, CPU, batch_questions=2, **walk)
    got = drivers.val_vcr_qar(qar_model, [_hollow(q) for q in qs], CPU, batch_questions=2, resident=rs, **walk)
    _equal_results(got, want)
    assert len(rs.launches) == 3 and rs.launches[0][0] == 16


class _Callable(object):
    def __init__(self, base, forward):
        self.__dict__.update(vars(base))
        self._forward = forward

    def __call__(self, *a, **kw):
        return self._forward(*a, **kw)


def _equal_results(got, want):
    assert list(got) == list(want)
    for k in want:
        if isinstance(want[k], torch.Tensor):
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
        else:
            assert got[k] == want[k], k


def test_a_set_of_other_items_is_refused():
    model = types.SimpleNamespace(eval=lambda: None, _engine=lambda: _Engine())
    pairs, qs, qq = vg_pairs(), vcr_questions(), qar_questions()
    with pytest.raises(ValueError, match="other items"):
        drivers.val_vg(model, pairs, {1: [3]}, CPU, resident=fake_set(R.tables(R.from_pairs(pairs[:-1]))))
    with pytest.raises(ValueError, match="other items"):
        drivers.val_vcr(model, qs, CPU, resident=fake_set(R.tables(R.from_vcr(qs[:-1]))))
    with pytest.raises(ValueError, match="from_vcr_qar"):
        drivers.val_vcr_qar(model, qq, CPU, resident=fake_set(R.tables(R.from_vcr(qs[:5]))))
    with pytest.raises(ValueError, match="shard"):
        drivers.val_vcr(model, qs, CPU, resident=fake_set(R.tables(R.from_vcr(qs), (0, 3))))
    with pytest.raises(ValueError, match="head tables"):                     # a set without head tables has no head rows to give
        drivers.val_vg(model, pairs[:1], {1: [3]}, CPU, resident=fake_set(R.tables(R.from_queries([dict(pairs[0], mask_token_pos=torch.ones(6, dtype=torch.int64))]))))
    half = fake_set(R.tables(R.from_vcr(qs)))
    half.feature_dtype = "bf16"
    with pytest.raises(ValueError, match="bf16"):
        drivers.val_vcr(model, qs, CPU, resident=half)


class _Recorder(torch.nn.Module):
    """Stand-in for the training step: records what every forward was given."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.seen = []

    def _engine(self):
        return _Engine()

    def forward(self, input_ids, segment_ids, attention_mask, img_feats=None, masked_lm_labels=None):
        self.seen.append((input_ids, segment_ids, attention_mask, img_feats, masked_lm_labels))
        return (self.w * masked_lm_labels.double().sum() * 1e-3,)


@pytest.mark.parametrize("trim", [False, True])
@pytest.mark.parametrize("kind", ["colours", "vg", "template"])
def test_training_drivers_with_a_set_run_the_host_batches(kind, trim):
    batches = vg_train_batches() if kind == "vg" else colour_batches()
    opts = types.SimpleNamespace(learning_rate=1.0, warmup_steps=0, num_train_steps=10, lr_mul=1.0)

    def run(resident, feed):
        m = _Recorder()
        opt = torch.optim.SGD(m.parameters(), lr=0.0)
        if kind == "template":
            return m, drivers.tune_soft_template(m, opt, feed, CPU, trim=trim, resident=resident)
        fn = drivers.train_vg_batch if kind == "vg" else drivers.train_batch
        step, losses = fn(m, opt, feed, opts, CPU, global_step=2, trim=trim, resident=resident)
        assert step == 2 + len(batches)
        return m, losses
    t = R.tables(R.from_train_batches(batches))
    rs = fake_set(t)
    assert [x.tolist() for x in rs.batch_indices()] == [list(range(t["seq_first"][i], t["seq_first"][i + 1])) for i in range(len(batches))]
    for feed, host in ((rs.batch_indices(), batches), ([np.arange(t["n_seq"])[::-1][i::3].copy() for i in range(3)], None)):
        if host is None:
            host = _regroup(batches, feed, t["seq_first"])
        hm, hl = run(None, host)
        rm, rl = run(rs, iter(feed))
        assert len(hm.seen) == len(rm.seen) == 3 and [float(a) for a in hl] == [float(b) for b in rl]
        for a, b in zip(hm.seen, rm.seen):
            for x, y in zip(a, b):
                assert (x is None and y is None) or (x.dtype == y.dtype and x.shape == y.shape and x.numpy().tobytes() == y.numpy().tobytes())
    with pytest.raises(ValueError, match="indices"):
        run(rs, batches)                                     # batch dicts where index lists are taken
    with pytest.raises(ValueError, match="outside"):
        run(rs, [np.array([t["n_seq"]])])
    with pytest.raises(ValueError, match="from_train_batches"):
        run(fake_set(R.tables(R.from_vcr(vcr_questions(n=2)))), [np.array([0])])


# ---- 4. the binding ---------------------------------------------------------------------------------------------------------------------------
def test_heads_struct_and_entry_point_agree_with_the_header():
    from cpt_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "cpt_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} cpt_resident_heads;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(const int32_t\*|int32_t)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in L.ResidentHeads._fields_] == ["head_first", "head_pos", "head_label", "seq_label", "n_heads"]
    assert [c for _, c in L.ResidentHeads._fields_] == [ctypes.c_void_p] * 4 + [ctypes.c_int32]
    assert ctypes.sizeof(L.ResidentHeads) == 4 * 8 + 4 + 4 and L.ResidentHeads.n_heads.offset == 32
    decl = re.search(r"int cpt_gather_batch_heads\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", src, flags=re.S)).group(1)
    params = [p.strip() for p in decl.split(",")]
    res, args = L._SIGS["cpt_gather_batch_heads"]
    assert res is ctypes.c_int and len(args) == len(params) == 18
    for p, a in zip(params, args):
        want = ctypes.c_int if p.startswith("int ") else (ctypes.POINTER(L.ResidentStore) if "cpt_resident_store" in p else
                                                         ctypes.POINTER(L.ResidentHeads) if "cpt_resident_heads" in p else ctypes.c_void_p)
        assert a is want or a == want, (p, a)
    assert args[8:13] == L._SIGS["cpt_gather_batch"][1][5:10]                # the five outputs of cpt_gather_batch, in its order
    assert hasattr(L.lib(), "cpt_gather_batch_heads") and L.lib().cpt_version() == 8
