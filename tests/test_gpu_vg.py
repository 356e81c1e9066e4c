"""VG-CPT predicate scoring on the GPU: the MLM head on (sequence, position) rows with the full-vocabulary log-sum-exp
(include/cpt_hip.h cpt_model_fwd_rows), the mean log-probability scores (cpt_mean_logprob_scores) and the REC_MLM_CPT
(n, 2) / log_softmax forms, against the CPU oracle."""
import pytest
import torch

from cpt_amd import config as cfgmod
from cpt_amd import scoring as S
from cpt_amd import synth
from oracle import cpt_oracle as O

pytestmark = pytest.mark.gpu
BF16_TOL = 0.025          # the suite's bf16 band on logits (test_gpu_model.py)
MODES = (("fp32", 1e-4), ("bf16x3", 1e-4), ("bf16", BF16_TOL))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _model(cfg, seed, dev, mode):
    from cpt_amd.modeling_rec import REC_MLM_CPT
    sd = synth.init_state_dict(cfg, seed, head="cpt")
    m = REC_MLM_CPT(cfg)
    m.load_state_dict(sd)
    m.tie_weights()
    m.to(dev).eval()
    m.set_compute_dtype(mode)
    return m, sd


def _rows(B, L, per_seq, seed):
    """(row_seq, mask_pos): per_seq[b] rows for sequence b at distinct positions, ascending sequences."""
    g = torch.Generator().manual_seed(seed)
    seq, pos = [], []
    for b, k in enumerate(per_seq):
        p = torch.randperm(L, generator=g)[:k].sort().values
        seq += [b] * k
        pos += p.tolist()
    return torch.tensor(seq, dtype=torch.int64), torch.tensor(pos, dtype=torch.int64)


def _oracle_rows(sd, cfg, b, seq, pos):
    """Full-vocabulary scores of the head rows, float64 log-sum-exp."""
    with torch.no_grad():
        x, _ = O.bert_img_forward(sd, cfg.to_dict(), b["input_ids"], b["segment_ids"], b["attention_mask"], img_feats=b["img_feats"])
        logits = O.lm_head(sd, cfg.to_dict(), x[seq, pos])
    return logits, torch.logsumexp(logits.double(), -1)


def _run(m, b, seq, pos, dev, cols=None, lse=True):
    with torch.no_grad():
        return m._engine().forward_rows(b["input_ids"].to(dev), b["segment_ids"].to(dev), b["attention_mask"].to(dev), None,
                                        b["img_feats"].to(dev), row_seq=seq.to(dev), mask_pos=pos.to(dev),
                                        cols=None if cols is None else cols.to(dev), lse=lse)


@pytest.mark.parametrize("mode,tol", MODES)
def test_rows_and_lse_match_oracle_tiny(dev, mode, tol):
    """Several rows per sequence, sequences without rows, duplicate columns; V = 518 (not a multiple of the 64-column tile)."""
    cfg = cfgmod.tiny(max_position_embeddings=64)
    m, sd = _model(cfg, 11, dev, mode)
    b = synth.make_batch(6, cfg, seed=5, max_seq_len=20, img_seq_len=10)
    seq, pos = _rows(6, 30, [2, 0, 3, 1, 0, 3], 7)
    cols = torch.tensor([3, 517, 103, 3, 0, 250, 511, 512], dtype=torch.int64)
    ref, ref_lse = _oracle_rows(sd, cfg, b, seq, pos)
    out = _run(m, b, seq, pos, dev, cols)
    e_log = (out["logits"].cpu() - ref[:, cols]).abs().max().item()
    e_lse = (out["lse"].cpu().double() - ref_lse).abs().max().item()
    print("%s: max|logits - oracle| %.3e, max|lse - oracle| %.3e" % (mode, e_log, e_lse))
    assert e_log <= tol and e_lse <= tol
    assert torch.equal(out["logits"][:, 0], out["logits"][:, 3])       # duplicate column


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_full_vocab_lse_and_listed_columns(dev, mode):
    """cols = NULL: row_lse is the log-sum-exp of the same call's (n, V) scores; the listed columns equal those columns."""
    cfg = cfgmod.tiny(max_position_embeddings=64)
    m, _ = _model(cfg, 12, dev, mode)
    b = synth.make_batch(4, cfg, seed=6, max_seq_len=20, img_seq_len=10)
    seq, pos = _rows(4, 30, [3, 1, 0, 2], 8)
    full = _run(m, b, seq, pos, dev)
    assert full["logits"].shape == (seq.numel(), cfg.vocab_size)
    lse = torch.logsumexp(full["logits"].double(), -1)
    rel = ((full["lse"].double() - lse).abs() / lse.abs().clamp_min(1.0)).max().item()
    assert rel <= 1e-5, rel
    cols = torch.arange(0, cfg.vocab_size, 37, dtype=torch.int64)
    part = _run(m, b, seq, pos, dev, cols)
    tol = 1e-5 if mode == "fp32" else 1e-4
    assert (part["logits"] - full["logits"][:, cols.to(dev)]).abs().max().item() <= tol
    assert (part["lse"].double() - lse).abs().max().item() <= tol


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_lse_no_overflow_with_large_bias(dev, mode):
    cfg = cfgmod.tiny(max_position_embeddings=64)
    m, sd = _model(cfg, 13, dev, mode)
    hot = torch.tensor([5, 300, 517])
    with torch.no_grad():
        m.cls.bias[hot.to(dev)] += 80.0
    sd = {k: v.clone() for k, v in sd.items()}
    sd["cls.bias"][hot] += 80.0
    b = synth.make_batch(3, cfg, seed=9, max_seq_len=20, img_seq_len=10)
    seq, pos = _rows(3, 30, [1, 2, 1], 9)
    _, ref_lse = _oracle_rows(sd, cfg, b, seq, pos)
    out = _run(m, b, seq, pos, dev, torch.tensor([5, 6]))
    assert torch.isfinite(out["lse"]).all()
    assert (out["lse"].cpu().double() - ref_lse).abs().max().item() <= (1e-4 if mode == "fp32" else BF16_TOL)


def test_one_row_per_sequence_equals_mask_logits(dev):
    cfg = cfgmod.tiny(max_position_embeddings=64)
    m, _ = _model(cfg, 14, dev, "fp32")
    b = synth.make_batch(5, cfg, seed=10, max_seq_len=20, img_seq_len=10)
    d = {k: v.to(dev) for k, v in b.items()}
    with torch.no_grad():
        ref = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], mask_token_pos=d["mask_token_pos"])[0]
    out = _run(m, b, torch.arange(5), b["mask_token_pos"], dev)
    assert (out["logits"] - ref).abs().max().item() <= 1e-5


def test_shape_errors(dev):
    cfg = cfgmod.tiny(max_position_embeddings=64)
    m, _ = _model(cfg, 15, dev, "fp32")
    b = synth.make_batch(3, cfg, seed=11, max_seq_len=20, img_seq_len=10)
    cases = [(torch.tensor([], dtype=torch.int64), torch.tensor([], dtype=torch.int64), None),     # no rows
             (torch.tensor([1, 0]), torch.tensor([3, 4]), None),                                    # not ascending
             (torch.tensor([0, 3]), torch.tensor([3, 4]), None),                                    # sequence outside [0, B)
             (torch.tensor([0, 1]), torch.tensor([3, 30]), None),                                   # position outside [0, L)
             (torch.tensor([0, 1]), torch.tensor([3, -1]), None),
             (torch.tensor([0, 1]), torch.tensor([3, 4]), torch.zeros(cfg.vocab_size + 1, dtype=torch.int64)),   # n_cols > V
             (torch.tensor([0, 1]), torch.tensor([3, 4]), torch.tensor([3, cfg.vocab_size])),                     # column id outside [0, V)
             (torch.tensor([0, 1]), torch.tensor([3, 4]), torch.tensor([-1, 3]))]
    for seq, pos, cols in cases:
        with pytest.raises(RuntimeError, match=r"status -1\)"):
            _run(m, b, seq, pos, dev, cols)


def _vg_batch(cfg, n_pairs, seed, Lt, Li):
    """6 sequences per pair; sequence 3 d + k - 1 of a pair carries k head rows (k = 1, 2, 3), as the VG test dataset lays them out."""
    b = synth.make_batch(6 * n_pairs, cfg, seed=seed, max_seq_len=Lt, img_seq_len=Li)
    g = torch.Generator().manual_seed(seed)
    rows = []
    for s in range(6 * n_pairs):
        k = s % 3 + 1
        p0 = int(torch.randint(1, Lt - 4, (1,), generator=g))
        rows += [(s, p0 + j) for j in range(k)]
    return b, torch.tensor(rows, dtype=torch.int64)


IDX2PRED = {1: [7], 2: [20, 21], 3: [30, 31, 32], 4: [7, 40], 5: [103], 6: [5, 6, 7], 7: [450]}


@pytest.mark.parametrize("mode,tol", MODES)
def test_predicate_scores_match_val_loop(dev, mode, tol):
    """vg_predicate_scores (forward_rows on the word-piece union + cpt_mean_logprob_scores) against the torch restatement of
    val()'s loop over the oracle's full score rows."""
    cfg = cfgmod.tiny(max_position_embeddings=64)
    m, sd = _model(cfg, 16, dev, mode)
    b, mtp = _vg_batch(cfg, 3, 12, 24, 10)
    d = {k: v.to(dev) for k, v in b.items()}
    with torch.no_grad():
        got = S.vg_predicate_scores(m, d["input_ids"], d["segment_ids"], d["attention_mask"], d["img_feats"], mtp.to(dev), IDX2PRED)
        x, _ = O.bert_img_forward(sd, cfg.to_dict(), b["input_ids"], b["segment_ids"], b["attention_mask"], img_feats=b["img_feats"])
    seq_rows = [O.lm_head(sd, cfg.to_dict(), x[s, mtp[mtp[:, 0] == s, 1]]) for s in range(b["input_ids"].size(0))]
    ref = S.vg_val_scores_reference(seq_rows, IDX2PRED)
    assert got.shape == ref.shape
    assert torch.equal(got[:, :, 0].cpu(), torch.zeros_like(ref[:, :, 0]))        # background slot
    err = (got.cpu() - ref).abs().max().item()
    print("%s: max|scores - val()| %.3e" % (mode, err))
    assert err <= tol


def test_mean_logprob_missing_template_is_nan(dev):
    logits = torch.randn(6, 4, device=dev)
    lse = torch.randn(6, device=dev)
    slot = torch.tensor([[0, -1, 3]], dtype=torch.int32)
    cc = torch.tensor([[0, 0, 0], [1, 0, 0], [2, 3, 0], [1, 2, 3]], dtype=torch.int32)
    cl = torch.tensor([0, 1, 2, 3], dtype=torch.int32)
    out = S.mean_logprob_scores_device(logits, lse, slot, cc, cl).cpu()
    lc, lsc = logits.cpu(), lse.cpu()
    assert out[0, 0] == 0 and torch.isnan(out[0, 2])
    assert abs(out[0, 1] - (lc[0, 1] - lsc[0])) <= 1e-6
    want = ((lc[3, 1] - lsc[3]) + (lc[4, 2] - lsc[4]) + (lc[5, 3] - lsc[5])) / 3
    assert abs(out[0, 3] - want) <= 1e-6


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_rec_mlm_cpt_pair_rows_and_log_softmax(dev, mode):
    """REC_MLM_CPT.forward with (n, 2) mask_token_pos (any row order) and log_softmax=True, with and without vocab_columns."""
    cfg = cfgmod.tiny(max_position_embeddings=64)
    m, sd = _model(cfg, 17, dev, mode)
    b = synth.make_batch(4, cfg, seed=13, max_seq_len=20, img_seq_len=10)
    d = {k: v.to(dev) for k, v in b.items()}
    mtp = torch.tensor([[2, 5], [0, 3], [0, 4], [3, 1], [2, 6]], dtype=torch.int64)
    ref, _ = _oracle_rows(sd, cfg, b, mtp[:, 0], mtp[:, 1])
    cols = torch.tensor([103, 7, 9], dtype=torch.int64)
    tol = 1e-4 if mode == "fp32" else BF16_TOL
    with torch.no_grad():
        raw = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], mask_token_pos=mtp.to(dev))[0]
        lsm = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], mask_token_pos=mtp.to(dev),
                vocab_columns=cols.to(dev), log_softmax=True)[0]
        one = m(d["input_ids"], d["segment_ids"], d["attention_mask"], img_feats=d["img_feats"], mask_token_pos=d["mask_token_pos"],
                log_softmax=True)[0]
    assert (raw.cpu() - ref).abs().max().item() <= tol
    assert (lsm.cpu() - ref.log_softmax(-1)[:, cols]).abs().max().item() <= tol
    ref1, _ = _oracle_rows(sd, cfg, b, torch.arange(4), b["mask_token_pos"])
    assert (one.cpu() - ref1.log_softmax(-1)).abs().max().item() <= tol


@pytest.mark.parametrize("mode,tol", [("fp32", 1e-3), ("bf16x3", 1e-3), ("bf16", BF16_TOL)])
def test_oscar_base_16_pairs(dev, mode, tol):
    """Oscar-base shapes (V = 30522, H = 768), 16 pairs = 96 sequences of 70 + 60, 192 head rows (2 encoder layers to keep the CPU
    oracle short; L = 130 runs the unfused encoder path).  Listed columns and row_lse against the oracle; the predicate argmax agrees
    wherever the oracle's top two are further apart than twice the band."""
    cfg = cfgmod.oscar_base(num_hidden_layers=2)
    m, sd = _model(cfg, 21, dev, mode)
    b, mtp = _vg_batch(cfg, 16, 14, 70, 60)
    assert mtp.size(0) == 192
    idx2pred = {i + 1: [1000 + 3 * i + j for j in range(i % 3 + 1)] for i in range(50)}
    cols, cand_cols, cand_len = S.vg_candidates(idx2pred)
    ref, ref_lse = _oracle_rows(sd, cfg, b, mtp[:, 0], mtp[:, 1])
    out = _run(m, b, mtp[:, 0], mtp[:, 1], dev, cols)
    e_log = (out["logits"].cpu() - ref[:, cols]).abs().max().item()
    e_lse = (out["lse"].cpu().double() - ref_lse).abs().max().item()
    print("%s: max|logits - oracle| %.3e, max|lse - oracle| %.3e" % (mode, e_log, e_lse))
    assert e_log <= tol and e_lse <= tol
    got = S.mean_logprob_scores_device(out["logits"], out["lse"], S.vg_slot_rows(16), cand_cols, cand_len).cpu()[:, 1:]
    want = S.mean_logprob_scores_device(ref[:, cols].to(dev), ref_lse.float().to(dev), S.vg_slot_rows(16), cand_cols, cand_len).cpu()[:, 1:]
    top2 = want.topk(2, -1).values
    clear = (top2[:, 0] - top2[:, 1]) > 4 * tol
    assert torch.equal(got.argmax(-1)[clear], want.argmax(-1)[clear])


def test_mean_logprob_device_matches_reference_val_pt(dev, golden_dir):
    """cpt_mean_logprob_scores against the scores the reference's val() saved (tools/make_golden_vg.py)."""
    import os
    import numpy as np
    g = np.load(os.path.join(golden_dir, "tiny_vg_val.npz"))
    idx2pred = {i: [int(t) for t in row if t >= 0] for i, row in enumerate(g["pred_pieces"]) if (row >= 0).any()}
    cols, cc, cl = S.vg_candidates(idx2pred)
    rows = torch.from_numpy(g["row_logits"]).to(dev)
    n = rows.size(0)
    seq = torch.from_numpy(g["row_seq"])
    slot = S.vg_slot_rows_from(seq, int(seq.max()) + 1)
    lse = torch.logsumexp(rows.double(), -1).float()
    got = S.mean_logprob_scores_device(rows[:, cols.to(dev)].contiguous(), lse, slot, cc, cl).cpu()
    want = torch.from_numpy(g["val_scores"]).reshape(got.shape)
    assert n == int(slot.max()) + 3
    assert (got - want).abs().max().item() <= 1e-5
