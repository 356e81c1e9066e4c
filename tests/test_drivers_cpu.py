"""CPU: the loop skeletons of cpt_amd/drivers.py without a device -- the sharded evaluation pass (_eval_pass: shard, walk, write-back, gather and
fill) with a pure-torch ``step`` and simulated ranks, the grouping (_walk: data set order, bucket order, max_sequences packing), the
de-duplicated accuracy against the host forms of scoring.py, the scheduled training pass and the accumulation loop with stand-in models."""
import logging
import types

import pytest
import torch

from cpt_amd import batching, drivers, scoring
from cpt_amd import dist as cdist

N, SIZE = 11, 3
KEYS = [5, 2, 9, 2, 7, 5, 1, 9, 2, 4, 7]            # a fixed non-monotone permutation with ties
COUNTS = [1, 6, 2, 2, 5, 1, 3, 4, 1, 6, 2]          # ragged sequences per item
OUTPUTS = [((), torch.int64, -1), ((3,), torch.float32, 0.5)]
CPU = torch.device("cpu")


def _closed_form(n):
    i = torch.arange(n, dtype=torch.int64)
    return i, (2 * i[:, None] + torch.arange(3)).float()


def _run_pass(n, bucket, groups=None):
    """_eval_pass over n items whose step returns (item index, 2 * item index + column); -> (results, number of step calls)."""
    calls = []

    def groups_of(lo, hi):
        if groups is not None:
            return groups(lo, hi)
        return drivers._walk(hi - lo, SIZE, KEYS[lo:hi] if bucket else None)

    def step(idx, lo):
        assert not torch.is_grad_enabled()
        calls.append(list(idx))
        g = torch.tensor([lo + i for i in idx], dtype=torch.int64)
        return g, (2 * g[:, None] + torch.arange(3)).float()

    return drivers._eval_pass(n, groups_of, OUTPUTS, step, CPU, bucket), calls


@pytest.mark.parametrize("bucket", [False, True])
def test_eval_pass_single_process_equals_the_closed_form(bucket):
    (ids, mat), calls = _run_pass(N, bucket)
    want_ids, want_mat = _closed_form(N)
    assert ids.dtype == torch.int64 and mat.dtype == torch.float32
    assert torch.equal(ids, want_ids) and torch.equal(mat, want_mat)
    assert sorted(i for c in calls for i in c) == list(range(N))          # every item in exactly one group
    assert [len(c) for c in calls] == [3, 3, 3, 2]


def test_walk_orders_a_shard():
    plain = drivers._walk(N, SIZE)
    assert plain == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10]]              # consecutive runs
    by_len = drivers._walk(N, SIZE, KEYS)
    flat = [i for g in by_len for i in g]
    assert sorted(flat) == list(range(N)) and [len(g) for g in by_len] == [3, 3, 3, 2]
    assert flat == sorted(range(N), key=lambda i: (KEYS[i], i))            # non-decreasing key, ties in data set order
    assert [KEYS[i] for i in flat] == sorted(KEYS)
    assert drivers._walk(0, SIZE) == [] and drivers._walk(0, SIZE, []) == []


@pytest.mark.parametrize("cap", [4, 7, 64])
def test_walk_packs_whole_items_under_max_sequences(cap):
    plain = drivers._walk(N, SIZE, None, COUNTS, cap)
    assert plain == batching.pack_queries(COUNTS, cap)
    order = batching.length_order(KEYS, 0)[0].tolist()
    by_len = drivers._walk(N, SIZE, KEYS, COUNTS, cap)
    assert by_len == [[order[i] for i in g] for g in batching.pack_queries([COUNTS[i] for i in order], cap)]
    assert [i for g in by_len for i in g] == order
    for groups in (plain, by_len):
        assert sorted(i for g in groups for i in g) == list(range(N))
        for g in groups:
            assert sum(COUNTS[i] for i in g) <= cap or (len(g) == 1 and COUNTS[g[0]] > cap)
    assert drivers._walk(0, SIZE, None, [], cap) == []


@pytest.mark.parametrize("cap", [7, 64])
@pytest.mark.parametrize("bucket", [False, True])
def test_eval_pass_with_packed_groups(bucket, cap):
    groups = lambda lo, hi: drivers._walk(hi - lo, SIZE, KEYS[lo:hi] if bucket else None, COUNTS[lo:hi], cap)
    (ids, mat), _ = _run_pass(N, bucket, groups)
    want_ids, want_mat = _closed_form(N)
    assert torch.equal(ids, want_ids) and torch.equal(mat, want_mat)


@pytest.mark.parametrize("bucket", [False, True])
@pytest.mark.parametrize("n", [0, 1, 5, 11])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_eval_pass_on_simulated_ranks(monkeypatch, world, n, bucket):
    """Every rank's shard-local tensors, as handed to gather_fixed, concatenated in rank order are the single-process result."""
    single, _ = _run_pass(n, bucket)
    want = _closed_form(n)
    for s, w in zip(single, want):
        assert torch.equal(s, w)
    parts = [[] for _ in OUTPUTS]
    for rank in range(world):
        seen = []

        def gather(local, n_total, fill=0):
            seen.append((local.clone(), n_total, fill))
            return local

        monkeypatch.setattr(cdist, "rank_world", lambda: (rank, world))
        monkeypatch.setattr(cdist, "gather_fixed", gather)
        _, calls = _run_pass(n, bucket)
        lo, hi = cdist.shard_range(n, rank, world)
        if hi == lo:
            assert calls == []                                               # an empty shard runs no step ...
        assert len(seen) == len(OUTPUTS)                                     # ... and still gathers, once per output, in order
        for k, ((local, n_total, fill), (shape, dtype, want_fill)) in enumerate(zip(seen, OUTPUTS)):
            assert tuple(local.shape) == (hi - lo,) + shape and local.dtype == dtype
            assert n_total == n and fill == want_fill
            parts[k].append(local)
    for k in range(len(OUTPUTS)):
        assert torch.equal(torch.cat(parts[k], 0), single[k])


def test_eval_pass_fills_what_no_step_wrote():
    """The shard-local tensors start at each output's fill: a step that returns nothing for an output leaves it there."""
    out = drivers._eval_pass(4, lambda lo, hi: [[0, 1]], OUTPUTS, lambda idx, lo: _closed_form(2), CPU, False)
    assert out[0].tolist() == [0, 1, -1, -1]
    assert torch.equal(out[1][2:], torch.full((2, 3), 0.5))


def test_dedup_accuracy_equals_the_host_forms():
    ids, flags = [7, 3, 7, 9, 3], [1, 0, 0, 1, 1]
    got = drivers._dedup_accuracy(torch.tensor(flags, dtype=torch.uint8), ids, len(ids))
    assert isinstance(got, float) and got == 2 / 5
    assert got == scoring.gqa_accuracy([{"question_id": q, "correct": f} for q, f in zip(ids, flags)], len(ids))
    by_question = [{"questionId": q, "correct": f} for q, f in zip(ids, flags)]
    assert got == scoring.nsp_accuracy(by_question, len(ids)) == scoring.vcr_qar_accuracy(by_question, len(ids))
    cols = torch.tensor([[1, 0, 0], [0, 1, 0], [0, 1, 0], [1, 1, 1], [1, 0, 0]], dtype=torch.uint8)
    got3 = drivers._dedup_accuracy(cols, ids, len(ids))
    want3 = [scoring.vcr_qar_accuracy([{"questionId": q, "correct": int(f)} for q, f in zip(ids, cols[:, j].tolist())], len(ids)) for j in range(3)]
    assert got3 == want3 == [2 / 5, 2 / 5, 1 / 5]


def test_accumulation_helper_has_two_names():
    assert drivers.qar_accumulation is drivers.gqa_accumulation
    for args, kw in (((100, 1, 8, 13), {"num_train_epochs": 2}), ((1000, 4, 8, 250), {"num_train_epochs": 5}), ((3, 4, 2, 1), {}),
                     ((1000, 4, 8, 250), {"num_train_epochs": 5, "max_steps": 17})):
        assert drivers.qar_accumulation(*args, **kw) == drivers.gqa_accumulation(*args, **kw)


# ---- the scheduled pass (train_batch, train_vg_batch) --------------------------------------------------------------------------------------
class _GridModel(torch.nn.Module):
    """Stand-in: two tiny Linear layers (four parameters -> four groups); records the label grid and the plain rate of every forward and raises
    on the calls listed in ``fail``."""

    def __init__(self, fail=()):
        super().__init__()
        self.a, self.b = torch.nn.Linear(2, 1), torch.nn.Linear(2, 1)
        self.fail, self.grids, self.rates, self.optimizer = set(fail), [], [], None

    def forward(self, input_ids, segment_ids, attention_mask, img_feats=None, masked_lm_labels=None):
        self.grids.append(masked_lm_labels)
        self.rates.append([g["lr"] for g in self.optimizer.param_groups])
        if len(self.grids) - 1 in self.fail:
            raise RuntimeError("stand-in failure")
        return ((self.a(img_feats) + self.b(img_feats)).sum(),)


def _grid_setup(fail=()):
    m = _GridModel(fail)
    m.optimizer = torch.optim.SGD([{"params": [p]} for p in m.parameters()], lr=0.0)
    opts = types.SimpleNamespace(learning_rate=1.0, warmup_steps=0, num_train_steps=10, lr_mul=10.0)     # rate of step s: (10 - s) / 10
    return m, m.optimizer, opts


def _ref_batch():
    return {"input_ids": torch.zeros(2, 3, dtype=torch.long), "segment_ids": torch.zeros(2, 3, dtype=torch.long),
            "attention_mask": torch.ones(2, 5, dtype=torch.long), "img_feats": torch.ones(2, 2, 2),
            "mask_token_pos": torch.tensor([1, 2]), "colors": torch.tensor([7, 8])}


def test_scheduled_pass_advances_once_per_completed_step(caplog):
    m, opt, opts = _grid_setup(fail=(1,))
    marks = []

    def grid_fn(batch):
        marks.append(sorted(batch))
        return torch.full((2, 5), len(marks))

    with caplog.at_level(logging.INFO, logger="cpt_amd.drivers"):
        step, losses = drivers._scheduled_pass(m, opt, [_ref_batch()] * 3, opts, CPU, 0, grid_fn)
    assert step == 2 and len(losses) == 2 and m.training
    assert [int(g[0, 0]) for g in m.grids] == [1, 2, 3] and marks[0] == sorted(_ref_batch())
    # the skipped batch 1 does not advance the schedule: batch 2 runs at the rate of step 1 (0.9), not of step 2 (0.8)
    assert [r[2] for r in m.rates] == [1.0, 0.9, 0.9]
    assert m.rates[2] == [9.0, 9.0, 0.9, 0.9]                                 # groups 0-1 take lr x lr_mul
    assert sum("step 1 of this pass skipped: stand-in failure" in r.getMessage() for r in caplog.records) == 1
    step, losses = drivers._scheduled_pass(m, opt, [_ref_batch()] * 2, opts, CPU, step, grid_fn)
    assert step == 4 and [r[2] for r in m.rates[3:]] == [0.8, 0.7]


def test_train_batch_and_train_vg_batch_pass_their_own_grid():
    m, opt, opts = _grid_setup()
    batch = _ref_batch()
    step, losses = drivers.train_batch(m, opt, [batch], opts, CPU)
    assert step == 1 and len(losses) == 1 and torch.equal(m.grids[0], drivers._label_grid(batch))
    vg = dict(_ref_batch(), mask_token_pos=torch.tensor([[0, 1], [0, 4], [1, 2]]), row_labels=torch.tensor([3, 4, 5]))
    del vg["colors"]
    step, losses = drivers.train_vg_batch(m, opt, [vg], opts, CPU, global_step=step)
    assert step == 2 and len(losses) == 1 and torch.equal(m.grids[1], drivers.vg_label_grid(vg))
    assert (m.grids[1] >= 0).sum() == 3 and (m.grids[0] >= 0).sum() == 2


# ---- the accumulation loop (train_gqa_batch, train_vcr_batch, train_vcr_qar_batch) ----------------------------------------------------------
def _accumulation_setup():
    events = []
    model = torch.nn.Linear(2, 1, bias=False)
    with torch.no_grad():
        model.weight.copy_(torch.tensor([[0.5, -0.25]]))
    zero = model.zero_grad
    model.zero_grad = lambda *a, **k: (events.append("zero"), zero(*a, **k))[1]
    scheduler = types.SimpleNamespace(step=lambda: events.append("sched"))
    optimizer = types.SimpleNamespace(step=lambda: events.append("opt"),
                                      clip_grad_norm_device=lambda max_norm: (events.append("device clip"), torch.tensor(0.0))[1])
    xs = [torch.tensor([float(i + 1), float(2 * i - 3)]) for i in range(7)]
    opts = types.SimpleNamespace(gradient_accumulation_steps=3, max_grad_norm=1e9)        # (a clip that never scales)
    return events, model, scheduler, optimizer, xs, opts


def test_accumulate_orders_a_window_and_keeps_the_unfinished_gradient():
    events, model, scheduler, optimizer, xs, opts = _accumulation_setup()
    raw = [float(model(x).sum().detach()) for x in xs]
    step, losses, norms = drivers._accumulate(model, optimizer, scheduler, (model(x).sum() for x in xs), opts, 5, use_device_clip=False)
    assert events == ["sched", "opt", "zero"] * 2 and step == 7                # 2 steps; never the optimizer's device clip
    assert len(losses) == len(norms) == 7
    for got, want in zip(losses, raw):
        assert not got.requires_grad and abs(float(got) - want / 3) < 1e-6
    torch.testing.assert_close(model.weight.grad, xs[6][None] / 3)             # the seventh micro-step's gradient is still there
    torch.testing.assert_close(norms[6], (xs[6] / 3).norm())                   # (the norm before the clip, from torch.nn.utils.clip_grad_norm_)


def test_accumulate_takes_the_device_clip_only_when_asked():
    events, model, scheduler, optimizer, xs, opts = _accumulation_setup()
    opts.gradient_accumulation_steps = 1
    step, losses, norms = drivers._accumulate(model, optimizer, scheduler, (model(x).sum() for x in xs[:2]), opts, 0)
    assert events == ["device clip", "sched", "opt", "zero"] * 2 and step == 2
    assert abs(float(losses[0]) - float(model(xs[0]).sum().detach())) < 1e-6          # gas == 1: the loss is not divided
