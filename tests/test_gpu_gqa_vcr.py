"""GPU: the GQA-CPT and VCR Q->A driver loops on the HIP path -- cpt_gqa_choose and cpt_nsp_choose against the host restatements and the
reference's own evaluate() fixtures (tools/make_golden_gqa_vcr_eval.py), cpt_grad_clip against float64 and torch.nn.utils.clip_grad_norm_, and
the drivers (val_gqa / val_vcr at world 1 and 2, train_gqa_batch / train_vcr_batch against the reference's training trace)."""
import os
import socket
import tempfile
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from cpt_amd import config as cfgmod
from cpt_amd import scoring as S
from cpt_amd import synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _gold(name):
    g = np.load(os.path.join(GOLDEN, name))
    return {k: g[k] for k in g.files}


def _tok():
    from transformers import BertTokenizer
    g = np.load(os.path.join(GOLDEN, "tiny_gqa_vcr_prompts.npz"))
    d = tempfile.mkdtemp()
    vf = os.path.join(d, "vocab.txt")
    with open(vf, "w") as f:
        f.write("\n".join(str(w) for w in g["vocab"]) + "\n")
    return BertTokenizer(vf, do_lower_case=True)


# ---- cpt_gqa_choose ------------------------------------------------------------------------------------------------------------------------
def _gqa_case(R, C, G, seed):
    """Scores of three distinct values (ties inside one lane's stride of 64 columns and across lanes), with planted rows: a NaN, all -inf, a
    -0 / +0 tie; string ids with -2 entries and -1 padding."""
    g = torch.Generator().manual_seed(seed)
    sc = torch.randint(0, 3, (R, C), generator=g).float() / 2
    sc[0] = -1.0
    sc[0, C - 1] = 1.0                          # the maximum in the last column
    if C > 64:
        sc[0, C - 65] = 1.0                     # ... tied with the same lane's previous column: the lower index wins
    if R > 1:
        sc[1, torch.randint(0, C, (1,), generator=g)] = float("nan")
        sc[1, C // 2] = float("nan")            # two NaN: the first wins
    if R > 2:
        sc[2] = float("-inf")
    if R > 3:
        sc[3] = -5.0
        sc[3, C // 3] = 0.0
        sc[3, 0] = -0.0                         # -0 == +0: column 0 wins when C // 3 > 0
    if R > 4:
        sc[4] = 0.25
        sc[4, min(C - 1, 70)] = 2.0
        sc[4, min(C - 1, 7)] = 2.0              # a tie across lanes
    piece = torch.randint(0, max(2, C // 2), (C,), generator=g).int()
    piece[torch.rand(C, generator=g) < 0.2] = -2
    gt = torch.randint(0, max(2, C // 2), (R, G), generator=g).int()
    if G > 1:
        gt[torch.rand(R, G, generator=g) < 0.4] = -1
        gt[:, 0].clamp_(min=0)
    return sc, piece, gt


def _gqa_host(sc, piece, gt):
    """gqa_choose_reference on strings made from the ids: label i is the string "s<i>", its first piece "s<piece[i]>" (or a string no label
    has), the ground truths of row r the labels gt[r] >= 0."""
    C = sc.size(1)
    n_str = max(C, int(gt.max()) + 1, int(piece.max()) + 1)
    labels = ["s%d" % i for i in range(n_str)]
    answer_labels = [("s%d" % int(p)) if int(p) >= 0 else "none%d" % i for i, p in enumerate(piece)]
    igts = [[int(x) for x in row if int(x) >= 0] for row in gt]
    res = S.gqa_choose_reference(sc, labels, answer_labels, igts)
    return sc.argmax(1).tolist(), [bool(r["correct"]) for r in res]


@pytest.mark.parametrize("R", [1, 5, 257])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 1853])
def test_gqa_choose_matches_host_restatement(dev, R, C):
    for G in (1, 3):
        sc, piece, gt = _gqa_case(R, C, G, seed=1000 * R + C + G)
        want_pred, want_ok = _gqa_host(sc, piece, gt)
        counts = torch.zeros(1, dtype=torch.int32, device=dev)
        pred, ok = S.gqa_choose_device(sc.to(dev), piece, gt, counts=counts)
        assert pred.dtype == torch.int64 and ok.dtype == torch.uint8
        assert pred.cpu().tolist() == want_pred
        assert ok.cpu().bool().tolist() == want_ok
        assert int(counts.item()) == sum(want_ok)
        S.gqa_choose_device(sc.to(dev), piece, gt, counts=counts)          # accumulates
        assert int(counts.item()) == 2 * sum(want_ok)
    if R >= 5 and C > 3:
        assert want_pred[2] == 0 and want_pred[3] == 0                      # all -inf: the first column; -0 / +0: a tie


def test_gqa_choose_matches_reference_evaluate_fixture(dev):
    g = _gold("tiny_gqa_eval.npz")
    tok = _tok()
    labels = [str(x) for x in g["labels"]]
    token_ids, label_sid, piece_sid = S.gqa_string_ids(labels, tok)
    _, answer_labels = S.gqa_first_pieces(labels, tok)
    igts = [[int(x) for x in row if x >= 0] for row in g["igt"]]
    logits = torch.from_numpy(g["rows"])[:, token_ids]
    counts = torch.zeros(1, dtype=torch.int32, device=dev)
    pred, ok = S.gqa_choose_device(logits.to(dev), piece_sid, S.gqa_gt_table(igts, label_sid), counts=counts)
    assert [answer_labels[p] for p in pred.cpu().tolist()] == [str(a) for a in g["answer"]]
    assert ok.cpu().bool().tolist() == g["correct"].tolist()
    assert int(counts.item()) == int(g["correct"].sum())
    res = [{"question_id": int(q), "correct": bool(c)} for q, c in zip(g["q_ids"], ok.cpu().tolist())]
    assert S.gqa_accuracy(res, len(res)) == float(g["acc"])
    ref = S.gqa_choose_reference(logits, labels, answer_labels, igts)
    assert [r["correct"] for r in ref] == ok.cpu().bool().tolist()


# ---- cpt_nsp_choose ------------------------------------------------------------------------------------------------------------------------
def _nsp_case(n_q, interval, n_rel, seed):
    """Relation rows from a pool whose choice scores are >= 1e-3 apart (float64): inside a question two scores are exactly tied (the same
    row) or cannot be flipped by an fp32 softmax difference -- the fixture's rule."""
    g = torch.Generator().manual_seed(seed)
    while True:
        pool = torch.randn(6, n_rel, generator=g)
        s = 1 - pool.double().softmax(-1)[:, 1]
        if float(((s[:, None] - s[None, :]).abs() + torch.eye(6)).min()) >= 1e-3:
            break
    rel = pool[torch.randint(0, 6, (n_q * interval,), generator=g)]
    labels = torch.randint(0, interval, (n_q,), generator=g)
    return rel, labels


@pytest.mark.parametrize("n_rel", [2, 3])
@pytest.mark.parametrize("interval", [1, 4, 5])
def test_nsp_choose_matches_host(dev, interval, n_rel):
    n_q = 131
    rel, labels = _nsp_case(n_q, interval, n_rel, seed=10 * interval + n_rel)
    want_sc, want_pred = S.nsp_choose(rel, interval)
    counts = torch.zeros(1, dtype=torch.int32, device=dev)
    sc, pred, ok = S.nsp_choose_device(rel.to(dev), interval, labels, counts=counts)
    assert (sc.cpu() - want_sc).abs().max().item() <= 1e-6
    assert pred.cpu().tolist() == want_pred
    want_ok = [p == int(lb) for p, lb in zip(want_pred, labels)]
    assert ok.cpu().bool().tolist() == want_ok
    assert int(counts.item()) == sum(want_ok)
    S.nsp_choose_device(rel.to(dev), interval, labels, counts=counts)
    assert int(counts.item()) == 2 * sum(want_ok)


def test_nsp_choose_fixture_nan_and_remainder(dev):
    g = _gold("tiny_vcr_nsp_eval.npz")
    interval = int(g["interval"])
    rel = torch.from_numpy(g["rel"])
    sc, pred, ok = S.nsp_choose_device(rel.to(dev), interval, g["labels"].tolist())
    assert pred.cpu().tolist() == g["answer"].tolist()
    assert ok.cpu().bool().tolist() == g["correct"].tolist()
    assert np.abs(sc.cpu().view(-1, interval).numpy() - g["choice_logits"]).max() <= 1e-6
    res = [{"questionId": int(q), "correct": bool(c)} for q, c in zip(g["q_ids"], ok.cpu().tolist())]
    assert S.nsp_accuracy(res, len(res)) == float(g["acc"])
    # a NaN score counts as the maximum, the first one wins (torch.argmax)
    bad = rel.clone()
    bad[2, 0] = float("nan")
    bad[3, 1] = float("nan")
    want_sc, want_pred = S.nsp_choose(bad, interval)
    sc, pred, _ = S.nsp_choose_device(bad.to(dev), interval, g["labels"].tolist())
    assert pred.cpu().tolist() == want_pred and want_pred[0] == 2
    assert torch.isnan(sc.cpu()).tolist() == torch.isnan(want_sc).tolist()
    with pytest.raises(RuntimeError, match="whole number"):
        S.nsp_choose_device(rel[:-1].to(dev), interval, g["labels"].tolist())


# ---- cpt_grad_clip -------------------------------------------------------------------------------------------------------------------------
def _clip(g, max_norm, ws, sq_in=None):
    from cpt_amd import _lib as L
    out = torch.empty(2, dtype=torch.float32, device=g.device)
    L.check(L.lib().cpt_grad_clip(g.data_ptr(), g.numel(), float(max_norm), L.ptr(sq_in), out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr()),
            "cpt_grad_clip")
    return out


def _clip_ws(dev):
    from cpt_amd import _lib as L
    return torch.zeros(int(L.lib().cpt_grad_clip_workspace_bytes()), dtype=torch.uint8, device=dev)


def _tiny_flat_size():
    cfg = cfgmod.tiny()
    return sum(int(np.prod(v.shape)) for k, v in synth.init_state_dict(cfg, 1, head="cpt").items() if "decoder.weight" not in k)


# 16384 elements per workgroup before the grid is capped: 300 workgroups are more than the 256 lanes of the final stage
@pytest.mark.parametrize("n", [1, 63, 1025, 300 * 16384 + 7, _tiny_flat_size()])
@pytest.mark.parametrize("offset", [0, 1])
def test_grad_clip_norm_scaling_and_determinism(dev, n, offset):
    gen = torch.Generator().manual_seed(n)
    base = (torch.randn(n + offset, generator=gen) * 0.01).to(dev)
    g0 = base[offset:]                            # offset 1: a buffer that does not start on a 16-byte boundary
    ws = _clip_ws(dev)
    true = float(g0.double().norm())
    g = g0.clone() if offset == 0 else base.clone()[offset:]
    out = _clip(g, 0.5 * true, ws)
    norm, coef = float(out[0]), float(out[1])
    assert abs(norm - true) <= 1e-5 * true
    assert coef < 1.0 and abs(coef - 0.5 * true / (norm + 1e-6)) <= 1e-6
    assert torch.equal(g, g0 * out[1])
    g2 = g0.clone() if offset == 0 else base.clone()[offset:]
    out2 = _clip(g2, 0.5 * true, ws)
    assert torch.equal(out2, out) and torch.equal(g2, g)          # the same buffer: the same norm bit for bit
    g3 = g0.clone() if offset == 0 else base.clone()[offset:]
    out3 = _clip(g3, 2.0 * true + 1.0, ws)
    assert float(out3[1]) == 1.0 and torch.equal(g3, g0) and torch.equal(out3[0], out[0])
    assert int(ws[:4].view(torch.int32).item()) == 0               # the ticket is left 0


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_grad_clip_nonfinite_as_torch(dev, bad):
    gen = torch.Generator().manual_seed(3)
    g0 = torch.randn(5000, generator=gen).to(dev)
    g0[1234] = bad
    p = torch.nn.Parameter(torch.zeros_like(g0))
    p.grad = g0.clone()
    tnorm = torch.nn.utils.clip_grad_norm_([p], 1.0)
    g = g0.clone()
    out = _clip(g, 1.0, _clip_ws(dev))
    assert torch.isnan(out[0]).item() == torch.isnan(tnorm).item() and torch.isinf(out[0]).item() == torch.isinf(tnorm).item()
    assert torch.equal(torch.isnan(g), torch.isnan(p.grad))
    fin = ~torch.isnan(p.grad)
    assert torch.equal(g[fin], p.grad[fin])
    if bad != bad:
        assert torch.isnan(out[1]).item() and bool(torch.isnan(g).all())
    else:
        assert float(out[1]) == 0.0 and int(torch.isnan(g).sum()) == 1 and float(g[fin].abs().max()) == 0.0      # inf * 0 = NaN, as torch


def test_grad_clip_sum_of_squares_from_elsewhere(dev):
    g0 = torch.randn(4099, generator=torch.Generator().manual_seed(5)).to(dev)
    sq = torch.tensor([16.0], dtype=torch.float64, device=dev)
    g = g0.clone()
    out = _clip(g, 1.0, _clip_ws(dev), sq_in=sq)
    assert float(out[0]) == 4.0 and torch.equal(g, g0 * out[1]) and abs(float(out[1]) - 1.0 / (4.0 + 1e-6)) < 1e-7


# ---- models and data of the driver tests -----------------------------------------------------------------------------------------------------
def _cfg():
    cfg = cfgmod.tiny()
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
    return cfg


def _gqa_model(dev, seed=4321):
    from cpt_amd.modeling_bert import BertImgForPreTraining
    from cpt_amd.modeling_rec import REC_MLM_CPT
    cfg = _cfg()
    pre = BertImgForPreTraining(cfg)
    pre.load_state_dict(synth.init_state_dict(cfg, seed, head="pretrain"))
    pre.tie_weights()
    m = REC_MLM_CPT(cfg)
    m.copy_from_pretraining_model(pre)
    m.to(dev).set_compute_dtype("fp32")
    return m


def _vcr_model(dev, seed=4321):
    from cpt_amd.modeling_bert import BertImgForPreTraining
    from cpt_amd.modeling_vcr import NSPCPT
    cfg = _cfg()
    pre = BertImgForPreTraining(cfg)
    pre.load_state_dict(synth.init_state_dict(cfg, seed, head="pretrain"))
    pre.tie_weights()
    m = NSPCPT(cfg)
    m.copy_from_pretraining_model(pre)
    m.to(dev).set_compute_dtype("fp32")
    return m


def _oracle_sd(seed=4321):
    return synth.init_state_dict(_cfg(), seed, head="pretrain")


GQA_LABELS = [str(x) for x in np.load(os.path.join(GOLDEN, "tiny_gqa_eval.npz"))["labels"]]


def _gqa_questions(n_q=7, Li=5, seed=3):
    from cpt_amd import prompts
    tok = _tok()
    rng = np.random.Generator(np.random.PCG64(seed))
    texts = ["what is the man holding?", "is the dog on the left of the cat?", "what color is the cup on the table?", "is the woman sitting?",
             "what is next to the chair?"]
    out = []
    for q in range(n_q):
        igt = [int(x) for x in rng.integers(0, len(GQA_LABELS), 1 + 2 * (q % 2))]
        d = prompts.assemble_gqa(tok, texts[q % len(texts)], igt, len(GQA_LABELS), Li, q_id=300 + (q if q != 5 else 1), max_seq_length=24,
                                 max_img_seq_length=Li)
        d["img_feats"] = torch.from_numpy(rng.standard_normal((Li, _cfg().img_feature_dim)).astype(np.float32))
        d["igt"] = igt
        out.append(d)
    return tok, out


def _vcr_questions(n_q=5, Li=5, seed=3):
    from cpt_amd import prompts
    tok = _tok()
    rng = np.random.Generator(np.random.PCG64(seed))
    colors, names = {"0": "red", "1_2": "blue"}, {"0": "person", "1_2": "dog and cat", "3": "table", "1": "dog", "2": "cat"}
    words = ["the", "dog", "cat", "is", "on", "table", "holding", "cup", "because", "she", "wants", "it", "sitting", "next", "to"]
    out = []
    for q in range(n_q):
        sent = lambda n: [words[i] if i < len(words) else [int(i - len(words))] for i in rng.integers(0, len(words) + 3, n)]
        d = prompts.assemble_vcr(tok, sent(5), [sent(4) for _ in range(4)], colors, names, Li, label=q % 4, q_id=100 + (q if q != 4 else 2),
                                 max_seq_length=24, max_img_seq_length=Li)
        d["img_feats"] = torch.from_numpy(rng.standard_normal((Li, _cfg().img_feature_dim)).astype(np.float32))
        out.append(d)
    return out


def _check_val_gqa(res, tok, qs):
    """Predictions, flags and accuracy equal the host restatement of evaluate() fed the same device logits; the repeated question_id counts once."""
    _, answer_labels = S.gqa_first_pieces(GQA_LABELS, tok)
    ref = S.gqa_choose_reference(res["logits"], GQA_LABELS, answer_labels, [q["igt"] for q in qs], q_ids=res["q_ids"])
    assert res["answers"] == [r["answer"] for r in ref]
    assert res["preds"].tolist() == res["logits"].argmax(1).tolist()
    assert res["correct"].bool().tolist() == [bool(r["correct"]) for r in ref]
    assert res["acc"] == S.gqa_accuracy(ref, len(qs))
    assert len(set(res["q_ids"])) == len(qs) - 1


def test_val_gqa_world1(dev):
    from cpt_amd import drivers
    from oracle import cpt_oracle as O
    m = _gqa_model(dev).eval()
    tok, qs = _gqa_questions()
    res = drivers.val_gqa(m, qs, GQA_LABELS, tok, dev, batch_questions=3)
    _check_val_gqa(res, tok, qs)
    # the gathered label-column logits against the oracle's REC_MLM_CPT (fp32 bound of test_scores_and_loss_match_oracle)
    osd = {k.replace("cls.predictions.", "cls."): v for k, v in _oracle_sd().items()}
    ids = torch.stack([torch.as_tensor(q["input_ids"]) for q in qs])
    seg = torch.stack([torch.as_tensor(q["segment_ids"]) for q in qs])
    msk = torch.stack([torch.as_tensor(q["input_mask"]) for q in qs])
    feats = torch.stack([q["img_feats"] for q in qs])
    mpos = torch.tensor([q["mask_token_pos"][0] for q in qs])
    with torch.no_grad():
        full = O.rec_mlm_cpt_forward(osd, _cfg().to_dict(), ids, seg, msk, img_feats=feats, mask_rows_only=mpos)[0]
    token_ids, _, _ = S.gqa_string_ids(GQA_LABELS, tok)
    assert (res["logits"] - full[:, token_ids]).abs().max().item() < 2e-5


def _check_val_vcr(res, qs):
    labels = [int(q["label"]) for q in qs]
    sc = res["scores"]
    want_pred = [int(sc[i].argmax()) for i in range(len(qs))]
    assert res["preds"].tolist() == want_pred
    flags = [p == lb for p, lb in zip(want_pred, labels)]
    assert res["correct"].bool().tolist() == flags
    ref = [{"questionId": q, "correct": c} for q, c in zip(res["q_ids"], flags)]
    assert res["acc"] == S.nsp_accuracy(ref, len(qs))
    assert len(set(res["q_ids"])) == len(qs) - 1


def test_val_vcr_world1(dev):
    from cpt_amd import drivers
    from oracle import cpt_oracle as O
    m = _vcr_model(dev).eval()
    qs = _vcr_questions()
    res = drivers.val_vcr(m, qs, dev, batch_questions=2)
    _check_val_vcr(res, qs)
    blk, interval = drivers._vcr_block(qs, torch.device("cpu"))
    with torch.no_grad():
        rel = O.nsp_cpt_forward(_oracle_sd(), _cfg().to_dict(), blk["input_ids"], blk["token_type_ids"], blk["attention_mask"], blk["img_feats"])[0]
    assert (res["scores"].view(-1) - S.choice_scores(rel)).abs().max().item() < 2e-5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _val_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cpt_amd import drivers
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        tok, qs = _gqa_questions()
        res = {"gqa": drivers.val_gqa(_gqa_model(dev).eval(), qs, GQA_LABELS, tok, dev, batch_questions=3),
               "vcr": drivers.val_vcr(_vcr_model(dev).eval(), _vcr_questions(), dev, batch_questions=2)}
        torch.save(res, os.path.join(tmp, "v%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_val_gqa_and_val_vcr_two_ranks_equal_single_process(dev):
    from cpt_amd import drivers
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_val_worker, args=(2, _free_port(), tmp), nprocs=2, join=True)
        r = [torch.load(os.path.join(tmp, "v%d.pt" % i)) for i in range(2)]
    tok, qs = _gqa_questions()
    want = {"gqa": drivers.val_gqa(_gqa_model(dev).eval(), qs, GQA_LABELS, tok, dev, batch_questions=3),
            "vcr": drivers.val_vcr(_vcr_model(dev).eval(), _vcr_questions(), dev, batch_questions=2)}
    for x in r:
        for task, score_key in (("gqa", "logits"), ("vcr", "scores")):
            a, b = x[task], want[task]
            assert torch.equal(a["preds"], b["preds"]) and torch.equal(a["correct"], b["correct"])
            assert torch.equal(a[score_key], b[score_key]) and a["acc"] == b["acc"] and a["q_ids"] == b["q_ids"]
        assert x["gqa"]["answers"] == want["gqa"]["answers"]


# ---- the training loops against the reference's trace --------------------------------------------------------------------------------------
def _trace_run(dev, task, device_clip):
    """The fixture's 3 optimizer steps x 2 micro-steps through the driver's pass, one optimizer step per call so that the parameters can be
    sampled after each.  Returns (losses, norms, coefficients or None, [parameter samples])."""
    from cpt_amd import drivers
    from cpt_amd.train import AdamW, WarmupLinearSchedule
    g = _gold("tiny_gqa_vcr_train.npz")
    cfg = _cfg()
    lr, eps, wd, max_norm = [float(x) for x in g[task + "_hyper"]]
    gas, micro, B = int(g["gas"]), int(g["micro"]), int(g["B"])
    m = _gqa_model(dev) if task == "gqa" else _vcr_model(dev)
    opt = AdamW(m, lr=lr, eps=eps, weight_decay=wd)
    sch = WarmupLinearSchedule(opt, warmup_steps=int(g["warmup_steps"]), t_total=int(g["t_total"]))
    opts = types.SimpleNamespace(gradient_accumulation_steps=gas, max_grad_norm=max_norm)
    bs = [synth.make_batch(B, cfg, seed=int(g[task + "_seed0"]) + i, max_seq_len=int(g["max_seq_len"]), img_seq_len=int(g["img_seq_len"]),
                           vary_regions=True) for i in range(micro)]
    named = dict(m.named_parameters())
    losses, norms, coefs, params = [], [], [], []
    step = 0
    for w in range(micro // gas):
        window = bs[w * gas:(w + 1) * gas]
        if task == "gqa":
            batches = [{"input_ids": b["input_ids"], "attention_mask": b["attention_mask"], "segment_ids": b["segment_ids"],
                        "img_feats": b["img_feats"], "label_id": torch.from_numpy(g["gqa_label_ids"][w * gas + i])} for i, b in enumerate(window)]
            args = (m, opt, sch, batches, opts, dev, torch.from_numpy(g["gqa_label_tokens"]), step, device_clip)
            run = drivers._gqa_pass
        else:
            # one question of 4 choices per micro-step, in prompts.assemble_vcr's layout
            batches = [[{"input_ids": b["input_ids"].numpy(), "input_mask": b["attention_mask"].numpy(), "segment_ids": b["segment_ids"].numpy(),
                         "img_feats": b["img_feats"], "label": int(g["vcr_labels"][w * gas + i]), "q_id": i}] for i, b in enumerate(window)]
            args = (m, opt, sch, batches, opts, dev, step, device_clip)
            run = drivers._vcr_pass
        if device_clip:
            # the coefficient of every micro-step: read from the optimizer behind each clip
            seen = []
            orig = opt.clip_grad_norm_device
            opt.clip_grad_norm_device = lambda mn: (orig(mn), seen.append(opt.last_clip))[0]
            step, ls, ns = run(*args)
            opt.clip_grad_norm_device = orig
            coefs += [float(c[1]) for c in seen]
        else:
            step, ls, ns = run(*args)
        losses += [float(x) for x in ls]
        norms += [float(x) for x in ns]
        params.append(np.stack([named[str(n)].detach().reshape(-1)[:int(g["n_sample"])].cpu().numpy() for n in g["sample_names"]]))
    assert step == micro // gas
    return g, losses, norms, coefs, np.stack(params)


@pytest.mark.parametrize("task", ["gqa", "vcr"])
def test_train_batch_matches_reference_trace(dev, task):
    """train_gqa_batch / train_vcr_batch (their shared pass) in fp32 against tiny_gqa_vcr_train.npz, the trace of the reference's own model under
    its loop.  Bounds: the fp32 bounds of tests/test_gpu_vcr_qar.py on the same tiny configuration -- loss 1e-5 absolute and gradients 2e-4
    relative (here: the gradient norm before each clip), updated parameters 1e-6 absolute (test_train_vcr_qar_batch).  The clip must act:
    the device coefficient is below 1 on every micro-step.  The same loop with torch.nn.utils.clip_grad_norm_ gives the same parameters."""
    g, losses, norms, coefs, params = _trace_run(dev, task, device_clip=True)
    print(task, "loss diff", np.abs(np.array(losses) - g[task + "_loss"]).max(), "norm rel", (np.abs(np.array(norms) - g[task + "_norm"]) / g[task + "_norm"]).max(),
          "param diff", np.abs(params - g[task + "_params"]).max(), "coefs", coefs)
    assert len(coefs) == int(g["micro"]) and all(c < 1.0 for c in coefs)
    assert np.abs(np.array(losses) - g[task + "_loss"]).max() < 1e-5
    assert (np.abs(np.array(norms) - g[task + "_norm"]) / g[task + "_norm"]).max() < 2e-4
    assert np.abs(params - g[task + "_params"]).max() <= 1e-6
    assert np.abs(g[task + "_params"][-1] - g[task + "_params"][0]).max() > 1e-5          # (the parameters did move)
    _, losses_t, norms_t, _, params_t = _trace_run(dev, task, device_clip=False)
    print(task, "torch clip: param diff", np.abs(params_t - params).max())
    assert np.abs(params_t - params).max() <= 1e-6
    assert np.abs(np.array(losses_t) - np.array(losses)).max() < 1e-5
    assert (np.abs(np.array(norms_t) - np.array(norms)) / np.array(norms)).max() < 1e-5


def test_device_clip_norm_ignores_ranges_without_gradient(dev):
    """Tiny REC_MLM_CPT after one backward: the pooler receives no gradient (p.grad is None) and its range of the flat buffer adds nothing --
    the device norm over the whole buffer equals torch's norm over model.parameters()."""
    from cpt_amd.train import AdamW
    m = _gqa_model(dev).train()
    opt = AdamW(m, lr=1e-4)
    b = {k: v.to(dev) for k, v in synth.make_batch(4, _cfg(), seed=7, max_seq_len=20, img_seq_len=6, vary_regions=True).items()}
    grid = torch.full(b["attention_mask"].shape, -1, dtype=torch.long, device=dev)
    grid[torch.arange(4, device=dev), b["mask_token_pos"]] = b["colors"]
    loss = m(b["input_ids"], b["segment_ids"], b["attention_mask"], img_feats=b["img_feats"], masked_lm_labels=grid)[0]
    loss.backward()
    assert m.bert.pooler.dense.weight.grad is None
    before = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    norm = opt.clip_grad_norm_device(1e9)                       # coef == 1: the gradient is left bit for bit
    assert float(opt.last_clip[1]) == 1.0
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, before[n]), n
    tnorm = torch.nn.utils.clip_grad_norm_(m.parameters(), 1e9)
    assert abs(float(norm) - float(tnorm)) <= 1e-5 * float(tnorm)
    # and clipping through the optimizer scales what the p.grad views alias
    norm2 = opt.clip_grad_norm_device(0.5 * float(tnorm))
    assert torch.equal(norm2, norm)
    n0 = "bert.encoder.layer.0.attention.self.query.weight"
    assert torch.equal(dict(m.named_parameters())[n0].grad, before[n0] * opt.last_clip[1])
