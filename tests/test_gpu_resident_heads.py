"""GPU: resident sets with head tables.  cpt_gather_batch_heads against its numpy restatement (resident.gather_reference) into outputs pre-filled
with sentinels; val_vg, val_vcr and val_vcr_qar with a ResidentSet against the same call on host items, every field by its bits; train_batch,
train_vg_batch and tune_soft_template with a ResidentSet against the host path on the same batches; two ranks with their shards of a VCR set.
Everything is equality -- the gather writes the host batch's bits and equal inputs on an equal shape repeat bit for bit -- except the parameters
the backward sums with atomics, which are held to the run-to-run rule of tests/test_gpu_train.py."""
import copy
import os
import tempfile
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _softcheck as S
import test_gpu_gqa_vcr as G
import test_gpu_resident as GR
import test_gpu_trim_drivers as T
import test_gpu_vcr_qar as Q
import test_gpu_vg_eval as V
import test_resident_cpu as RC
import test_resident_heads_cpu as HC
from cpt_amd import dist as cdist
from cpt_amd import drivers
from cpt_amd import resident as R
from cpt_amd import soft_prompt
from cpt_amd import synth
from cpt_amd import train as TR
from test_gpu_train_trim import B, TLI, TLT, tiny  # noqa: F401  (tiny: the module fixture of the few-shot checkpoint)

pytestmark = pytest.mark.gpu
LT = 12
SENT = GR.INT_SENTINEL
HEADS = R.HEAD_OUTPUTS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------
def _head_sentinels(B_, R_, lt, li, dev):
    return {k: torch.full(shape, SENT, dtype=torch.int64, device=dev)
            for k, shape in (("head_rows", (R_, 2)), ("head_labels", (R_,)), ("label_grid", (B_, lt + li)), ("seq_label", (B_,)))}


def _labelled_tables(dim, Li):
    """Training batches with sequences of 0, 1 and 3 head rows, a label of -1, a label in the last attended text column and a labelled region
    column, plus a label per sequence."""
    items = R.from_train_batches(HC.vg_train_batches(Lt=LT, Li=Li, dim=dim))
    items["seq_labels"] = [np.arange(5) * 3 + 100 * i for i in range(items["n_items"])]
    return R.tables(items)


def _check(rs, t, idx, lt, li, dev, feature_dtype, heads=HEADS, with_pos=True):
    B_, seq = len(idx), torch.tensor(idx, dtype=torch.int32, device=dev)
    want = R.gather_reference(t, idx, lt, li)
    if feature_dtype == "bf16":
        want["img_feats"] = GR._bf16_round(want["img_feats"], dev)
    first = R.row_first(t, idx)
    R_ = int(first[-1])
    pre = dict(GR._sentinels(B_, lt, li, t["D"], dev), **_head_sentinels(B_, R_, lt, li, dev))
    got = rs.gather(seq, lt, li, mask_pos=with_pos, out=pre, row_first=torch.from_numpy(first).to(dev), R=R_, heads=heads)
    where = (idx, lt, li, heads)
    for k in ("input_ids", "segment_ids", "attention_mask") + (("mask_token_pos",) if with_pos else ()):
        assert got[k].data_ptr() == pre[k].data_ptr() and np.array_equal(got[k].cpu().numpy(), want[k]), (k,) + where
    assert np.array_equal(pre["img_feats"].view(torch.int32).cpu().numpy(), RC.bits(want["img_feats"])), where
    for k in HEADS:
        if k in heads:                  # every element overwritten: the reference holds no sentinel
            assert got[k].data_ptr() == pre[k].data_ptr() and np.array_equal(got[k].cpu().numpy(), want[k]), (k,) + where
            assert not (want[k] == SENT).any()
        else:                           # an output that was not asked for is not touched
            assert k not in got and bool((pre[k] == SENT).all()), (k,) + where
    return want


@pytest.mark.parametrize("feature_dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("dim,Li", [(2054, 50), (38, 5), (37, 5)])
def test_gather_batch_heads_equals_reference(dev, dim, Li, feature_dtype):
    t = _labelled_tables(dim, Li)
    rs = R.upload(t, dev, feature_dtype)
    assert rs.nbytes == R.store_bytes(t, feature_dtype) and rs.n_sequences == t["n_seq"] == 15
    p_last = int(t["text_len"][0]) - 1                                  # sequence 0 is labelled in its last attended text column
    assert p_last in t["head_pos"][:3] and LT + Li - 1 in t["head_pos"] and -1 in t["head_label"]
    if dim == 2054:
        cases = [([14, 0, 9, 0, 2], (LT, Li)), ([14, 0, 9, 0, 2], (p_last + 1, 0))]                 # B = 5: about 2 MB of features
    else:
        lists = [[0], [9], [2, 0, 2, 0], [14, 3, 0, 9, 1, 4, 7]]        # B = 1, a repeated sequence, arbitrary order; 0, 1 and 3 rows in one batch
        cases = [(idx, cut) for idx in lists for cut in ((LT, Li), (LT, 0), (p_last + 1, 0), (p_last + 1, 2))]
        cases += [([1, 3, 6], (LT, Li)), ([1, 3], (1, 0))]              # R = 0
    for idx, (lt, li) in cases:
        want = _check(rs, t, idx, lt, li, dev, feature_dtype)
        if 0 in idx and lt == p_last + 1:                               # the label in the last kept text column
            assert want["label_grid"][idx.index(0), lt - 1] != -1
        if 9 in idx and li == Li:                                       # the labelled region column (Lt_out = Lt)
            assert want["label_grid"][idx.index(9), lt + li - 1] != -1
    assert np.diff(R.row_first(t, [14, 3, 0, 9, 1, 4, 7])).tolist() == [1, 0, 3, 2, 0, 1, 1]
    # each of the four outputs NULL in turn; the launch with none of them; without mask_pos
    idx = [14, 3, 0, 9, 1]
    for drop in HEADS:
        _check(rs, t, idx, LT, Li, dev, feature_dtype, heads=tuple(k for k in HEADS if k != drop))
    _check(rs, t, idx, LT, Li, dev, feature_dtype, heads=())
    _check(rs, t, idx, LT, 0, dev, feature_dtype, heads=("label_grid",), with_pos=False)
    # an index outside the store is clamped to its nearest sequence (the Python side validates; the kernel never reads outside)
    S_ = t["n_seq"]
    first = R.row_first(t, [0, S_ - 1])
    got = rs.gather(torch.tensor([-5, S_ + 3], dtype=torch.int32, device=dev), LT, Li, row_first=torch.from_numpy(first).to(dev), R=int(first[-1]),
                    heads=HEADS)
    want = R.gather_reference(t, [0, S_ - 1], LT, Li)
    for k in ("input_ids", "attention_mask") + HEADS:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k


def test_gather_batch_heads_refusals(dev):
    pairs = HC.vg_pairs(Lt=LT, dim=38)
    t = R.tables(R.from_pairs(pairs))                                   # zero-shot pairs: head rows without labels
    rs = R.upload(t, dev)
    idx = [7, 0, 13]
    seq, first = torch.tensor(idx, dtype=torch.int32, device=dev), R.row_first(t, idx)
    rf = torch.from_numpy(first).to(dev)
    got = rs.gather(seq, LT, RC.LI, row_first=rf, R=int(first[-1]), heads=("head_rows",))
    assert np.array_equal(got["head_rows"].cpu().numpy(), R.gather_reference(t, idx, LT, RC.LI)["head_rows"])
    for heads in (("label_grid",), ("head_labels",), ("seq_label",)):   # a NULL table that an output needs: the error code, not a launch
        pre = dict(GR._sentinels(3, LT, RC.LI, 38, dev), **_head_sentinels(3, int(first[-1]), LT, RC.LI, dev))
        with pytest.raises(RuntimeError, match="cpt_gather_batch_heads"):
            rs.gather(seq, LT, RC.LI, out=pre, row_first=rf, R=int(first[-1]), heads=heads)
        assert all(bool((v == SENT).all()) for k, v in pre.items() if k != "img_feats")
    with pytest.raises(ValueError, match="row_first"):
        rs.gather(seq, LT, RC.LI, heads=("head_rows",))
    with pytest.raises(ValueError, match="heads"):
        rs.gather(seq, LT, RC.LI, heads=("rows",))
    plain = R.upload(R.from_queries(RC.ragged_queries(n=2)), dev)
    with pytest.raises(ValueError, match="head tables"):
        plain.gather(seq[:1] * 0, LT, 0, heads=())


# ---- the evaluation drivers -------------------------------------------------------------------------------------------------------------------
OPTIONS = [dict(), dict(trim=True), dict(bucket=True), dict(trim=True, bucket=True)]


def _clear():
    for counter in R.H2D.values():
        counter.clear()


def _compare(run, rs, model, index_bytes):
    """run(resident=..., **opts) with the set against the host items under every option; then a second pass, which uploads its lists only."""
    shapes = T.Shapes(model)
    for opts in OPTIONS:
        want = run(None, **opts)
        ran = shapes.take()
        _clear()
        got = run(rs, **opts)
        assert shapes.take() == ran, opts                               # the same shapes ran, trimmed ones included
        GR._same(got, want, str(opts))
        assert dict(R.H2D["calls"]) == {"seq_idx": 1} and dict(R.H2D["bytes"]) == {"seq_idx": index_bytes}, (opts, R.H2D)
        if opts.get("trim"):
            assert T._rows_run(ran) < sum(s[0] * (rs.Lt + rs.Li) for s in ran)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_val_vg_resident_equals_host(dev, mode):
    pairs, idx2pred = V._rows()
    m, _ = V._model(V._cfg(), dev, mode)
    _clear()
    rs = R.upload(R.from_pairs(pairs), dev)
    assert R.H2D["calls"]["tables"] > 0 and R.H2D["bytes"]["features"] == 4 * int(rs.tables["block_rows"].sum()) * rs.D
    n_seq, n_groups = 6 * len(pairs), -(-len(pairs) // 3)

    def run(resident, **opts):
        scores, keys = drivers.val_vg(m, pairs, idx2pred, dev, batch_pairs=3, resident=resident, **opts)
        return {"scores": scores.cpu(), "keys": keys}                   # (by their bits: the -inf / NaN pattern included)
    _compare(run, rs, m, 4 * (n_seq + n_seq + n_groups))               # the index lists and row_first (B + 1 per step), one copy
    if mode == "bf16":
        half = R.upload(R.from_pairs(pairs), dev, feature_dtype="bf16")
        GR._same(run(half, trim=True), run(None, trim=True), "bf16 store")
        m.set_compute_dtype("fp32")
        with pytest.raises(ValueError, match="bf16"):
            run(half)
    with pytest.raises(ValueError, match="other items"):
        run(R.upload(R.from_pairs(pairs[:-1]), dev))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_val_vcr_resident_equals_host(dev, mode):
    m = G._vcr_model(dev).eval()
    m.set_compute_dtype(mode)
    qs = HC.vcr_questions()
    rs = R.upload(R.from_vcr(qs), dev)
    run = lambda resident, **opts: drivers.val_vcr(m, qs, dev, batch_questions=2, resident=resident, **opts)
    _compare(run, rs, m, 4 * 4 * len(qs))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_val_vcr_qar_resident_equals_host(dev, mode):
    m = Q._model(Q._cfg(), dev, mode).eval()
    qs = HC.qar_questions()
    rs = R.upload(R.from_vcr_qar(qs), dev)
    assert len(rs.tables["block_rows"]) == len(qs)                      # one block per question for its eight sequences
    run = lambda resident, **opts: drivers.val_vcr_qar(m, qs, dev, batch_questions=2, resident=resident, **opts)
    _compare(run, rs, m, 4 * 8 * len(qs))


def _vcr_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        m = G._vcr_model(dev).eval()
        qs = HC.vcr_questions()
        rs = R.upload(R.from_vcr(qs), dev)                                # (each rank: its shard_range only)
        assert (rs.item_lo, rs.item_hi) == cdist.shard_range(len(qs), rank, world) and rs.tables["n_seq"] < rs.n_sequences
        opts = dict(batch_questions=2, trim=True, bucket=True)
        res = drivers.val_vcr(m, qs, dev, resident=rs, **opts)
        GR._same(res, drivers.val_vcr(m, qs, dev, **opts), "rank %d" % rank)
        torch.save(res, os.path.join(tmp, "v%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_two_ranks_val_vcr_with_resident_shards(dev):
    """Both ranks share cuda:0 over gloo, as tests/test_gpu_resident.py runs its two ranks: every rank uploads and walks its own shard and
    compares with the host-item pass of the same two ranks; both end with the same gathered results."""
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_vcr_worker, args=(2, G._free_port(), tmp), nprocs=2, join=True)
        r = [torch.load(os.path.join(tmp, "v%d.pt" % i), weights_only=False) for i in range(2)]
    GR._same(r[0], r[1], "rank 0 against rank 1")
    assert len(r[0]["q_ids"]) == 7


# ---- the training drivers ---------------------------------------------------------------------------------------------------------------------
# A step repeats its own bits -- loss, head-row scores, the Linear weights of the encoder -- on equal inputs; what the backward sums with fp32 atomic
# adds (bias, LayerNorm and table gradients) moves in its last bits from run to run, and through the update so do the NEXT step's inputs (README
# "Reproducibility"; measured with test_a_whole_pass_uploads_one_index_list: in a free-running pass the first two steps repeat every score bit and
# in the third 1777 of 2072 score elements differ in their last bits host path against host path, 1678 resident against host).
# So the two paths run in lockstep: every step is run by both from EQUAL parameters and optimizer state, compared -- loss and scores by their bits, the parameters after the step by the rule of tests/test_gpu_train.py --
# and then the resident side takes the host side's state, so that the next step again starts from equal inputs.
STEPS, LR, SEED = 3, 1e-4, 1234


def _is_linear_weight(n):
    return "encoder.layer" in n and n.endswith(".weight") and "LayerNorm" not in n


class _Side(object):
    """The few-shot checkpoint with dropout 0.1 and a pinned dropout stream, its optimizer, and the head-row scores of every forward."""

    def __init__(self, dev, tiny, kind, freeze=False):
        from cpt_amd.modeling_rec import REC_MLM_CPT
        self.dev, self.kind = dev, kind
        m = self.m = tiny[1](REC_MLM_CPT)
        drivers.set_dropout(m, 0.1)
        if freeze:
            TR.freeze_layers(m, 1)
        self.scores = []
        m.register_forward_hook(lambda mod, args, out: self.scores.append(out[1].detach().clone()))
        self.template = None
        if kind == "template":
            self.template = soft_prompt.attach(m, n_slots=S.N_SLOTS)
            with torch.no_grad():
                self.template.copy_(S.make_template(m.state_dict()[S.WORD].double().cpu()).to(self.template))
            self.opt = torch.optim.AdamW([self.template], lr=0.02, eps=1e-8)
        else:
            self.opt = TR.FusedAdamW(m, lr=LR)
        TR.set_dropout_seed(m, SEED)
        self.opts = types.SimpleNamespace(learning_rate=LR, warmup_steps=1, num_train_steps=10, lr_mul=1.0)

    def run(self, feed, resident, trim, step=0):
        """One driver call over ``feed`` -> the loss tensors."""
        if self.kind == "template":
            return drivers.tune_soft_template(self.m, self.opt, feed, self.dev, trim=trim, resident=resident)
        fn = drivers.train_vg_batch if self.kind == "vg" else drivers.train_batch
        after, losses = fn(self.m, self.opt, feed, self.opts, self.dev, global_step=step, trim=trim, resident=resident)
        assert after == step + len(losses)
        return losses

    def params(self):
        return {n: p.detach().clone() for n, p in self.m.named_parameters()}

    def take(self, other):
        """The parameters and the optimizer state of ``other``."""
        with torch.no_grad():
            for mine, theirs in zip(self.m.parameters(), other.m.parameters()):
                mine.copy_(theirs)
        self.opt.load_state_dict(copy.deepcopy(other.opt.state_dict()))      # (a copy: load_state_dict keeps tensors that need no conversion)


def _tiny_batches(cfg, kind):
    bs = [synth.make_batch(B, cfg(), seed=900 + i, max_seq_len=TLT, img_seq_len=TLI, n_regions=6, vary_regions=True) for i in range(STEPS)]
    if kind == "template":
        return [S.plant_slots(b) for b in bs]
    if kind == "vg":                        # sequences of 2, 1, 0 and 1 labelled rows
        out = []
        for i, b in enumerate(bs):
            p = [int(x) for x in b["mask_token_pos"]]
            vg = dict(b, mask_token_pos=torch.tensor([[0, p[0]], [0, 2 if p[0] == 1 else 1], [1, p[1]], [3, p[3]]]),
                      row_labels=torch.tensor([9, 10, 11, 12]) + i)
            del vg["colors"]
            out.append(vg)
        return out
    return bs


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _lockstep(dev, tiny, kind, host_batches, feed, rs, trim, freeze=False):
    """STEPS steps, every one run by the host path and by the resident path from equal state.  Returns the resident side."""
    host, res = _Side(dev, tiny, kind, freeze), _Side(dev, tiny, kind, freeze)
    for k in range(STEPS):
        lh, = host.run([host_batches[k]], None, trim, k)
        _clear()
        lr_, = res.run([feed[k]], rs, trim, k)
        assert dict(R.H2D["calls"]) == {"seq_idx": 1} and dict(R.H2D["bytes"]) == {"seq_idx": 4 * len(feed[k])}
        shape = res.m._engine().last_train_shape
        assert shape == host.m._engine().last_train_shape and (shape[1] + shape[2] < TLT + TLI) == trim, (k, shape)
        sh, sr = host.scores[-1], res.scores[-1]
        print("%s trim=%s step %d: loss %r against %r, %d of %d score elements differ" % (kind, trim, k, float(lh), float(lr_), int((sh != sr).sum()),
                                                                                         sh.numel()))
        assert _bits(lh) == _bits(lr_), (kind, k, float(lh), float(lr_))
        assert sh.shape == sr.shape and _bits(sh) == _bits(sr), (kind, k)
        ph, pr = host.params(), res.params()
        for n in ph:                        # the rule of tests/test_gpu_train.py, its run-to-run bound where the backward adds with atomics
            if n.endswith("attention.self.key.bias"):
                continue
            if _is_linear_weight(n):
                assert torch.equal(ph[n], pr[n]), (kind, k, n)
            else:
                assert float((ph[n].double() - pr[n].double()).norm()) <= 1e-4 * float(ph[n].double().norm()) + 1e-12, (kind, k, n)
        res.take(host)
    assert len(host.scores) == len(res.scores) == STEPS and _bits(host.scores[0]) != _bits(host.scores[1])
    return res


@pytest.mark.parametrize("trim", [False, True])
@pytest.mark.parametrize("kind", ["colours", "vg", "template"])
def test_training_with_a_resident_set_equals_the_host_path(dev, tiny, kind, trim):
    batches = _tiny_batches(tiny[0], kind)
    rs = R.upload(R.from_train_batches(batches), dev)
    assert rs.n_sequences == STEPS * B and (rs.item_lo, rs.item_hi) == (0, STEPS)
    _lockstep(dev, tiny, kind, batches, rs.batch_indices(), rs, trim)


def test_training_on_a_regrouped_index_list(dev, tiny):
    batches = _tiny_batches(tiny[0], "colours")
    rs = R.upload(R.from_train_batches(batches), dev)
    perm = np.random.Generator(np.random.PCG64(5)).permutation(STEPS * B)
    feed = [perm[i * B:(i + 1) * B] for i in range(STEPS)]
    _lockstep(dev, tiny, "colours", HC._regroup(batches, feed, rs.seq_first), feed, rs, True)


def test_training_with_a_resident_set_under_layer_freezing(dev, tiny):
    from cpt_amd.modeling_rec import REC_MLM_CPT
    batches = _tiny_batches(tiny[0], "colours")
    rs = R.upload(R.from_train_batches(batches), dev)
    got = _lockstep(dev, tiny, "colours", batches, rs.batch_indices(), rs, True, freeze=True).params()
    start = tiny[1](REC_MLM_CPT).state_dict()
    name = "bert.encoder.layer.%d.attention.self.query.weight"
    assert torch.equal(got[name % 0].cpu(), start[name % 0].cpu()) and not torch.equal(got[name % 1].cpu(), start[name % 1].cpu())


def test_a_whole_pass_uploads_one_index_list(dev, tiny):
    """One driver call over the whole pass: the lists of all steps go up in one copy, the first step -- equal inputs -- repeats the host pass's
    bits, and the later steps, whose parameters carry the atomics' last bits on either side, agree within the run-to-run bound
    tests/test_gpu_train.py holds the loss to.  The host pass against itself is printed beside it."""
    batches = _tiny_batches(tiny[0], "colours")
    rs = R.upload(R.from_train_batches(batches), dev)
    sides = [_Side(dev, tiny, "colours") for _ in range(3)]
    first = sides[0].run(batches, None, True)
    again = sides[1].run(batches, None, True)
    _clear()
    got = sides[2].run(iter(rs.batch_indices()), rs, True)
    assert dict(R.H2D["calls"]) == {"seq_idx": 1} and dict(R.H2D["bytes"]) == {"seq_idx": 4 * STEPS * B}
    assert len(got) == len(first) == STEPS and _bits(got[0]) == _bits(first[0]) and _bits(sides[2].scores[0]) == _bits(sides[0].scores[0])
    for k in range(STEPS):
        print("step %d: score elements that differ, host against host %d, resident against host %d of %d"
              % (k, int((sides[0].scores[k] != sides[1].scores[k]).sum()), int((sides[0].scores[k] != sides[2].scores[k]).sum()), sides[0].scores[k].numel()))
        assert abs(float(got[k]) - float(first[k])) <= 1e-6 * abs(float(first[k])), (k, float(got[k]), float(first[k]))
