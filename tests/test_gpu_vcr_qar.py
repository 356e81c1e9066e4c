"""GPU: VCR Q->AR (VCRQAR_NSPCPT, modeling_vcr.py:194-251; fewshot/vcr_qar_nsp_cpt.py) on the HIP path -- the two-head kernel against the oracle's
autograd (one nsp_cpt_forward per head, losses summed), the one-pass route against two forward(head=...) calls, the device Q->AR choice
against the host restatement of evaluate(), the ABI's error codes, and the drivers (val_vcr_qar at world 1 and 2, train_vcr_qar_batch)."""
import ctypes as C
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


def _cfg(dropout=False):
    cfg = cfgmod.tiny()
    if not dropout:
        cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
    return cfg


def _model(cfg, dev, mode, seed=4321):
    """VCRQAR_NSPCPT as the driver builds it (vcr_qar_nsp_cpt.py:1003-1006), cls_rat moved off cls_ans by a seeded offset (equal heads would
    hide a swapped head)."""
    from cpt_amd.modeling_bert import BertImgForPreTraining
    from cpt_amd.modeling_vcr import VCRQAR_NSPCPT
    pre = BertImgForPreTraining(cfg)
    pre.load_state_dict(synth.init_state_dict(cfg, seed, head="pretrain"))
    pre.tie_weights()
    m = VCRQAR_NSPCPT(cfg)
    m.copy_from_pretraining_model(pre)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        m.cls_rat.weight.add_(torch.randn(m.cls_rat.weight.shape, generator=g) * 0.05)
        m.cls_rat.bias.add_(torch.randn(m.cls_rat.bias.shape, generator=g) * 0.05)
    m.to(dev).set_compute_dtype(mode)
    return m


def _batch(n_q=2, n_ans=4, n_rats=4, seed=11):
    cfg = _cfg()
    b = synth.make_batch(n_q * (n_ans + n_rats), cfg, seed=seed, max_seq_len=20, img_seq_len=6, vary_regions=True)
    B0 = n_q * n_ans
    part = lambda lo, hi: {"input_ids": b["input_ids"][lo:hi], "token_type_ids": b["segment_ids"][lo:hi],
                           "attention_mask": b["attention_mask"][lo:hi], "img_feats": b["img_feats"][lo:hi]}
    return part(0, B0), part(B0, b["input_ids"].size(0))


def _to(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def _labels(n_q=2, n_ans=4, n_rats=4):
    return S.qar_choice_labels([2, 0][:n_q] if n_q <= 2 else [i % n_ans for i in range(n_q)],
                               [1, 3][:n_q] if n_q <= 2 else [(3 * i) % n_rats for i in range(n_q)], n_ans, n_rats)


def _oracle(m, qa, qr, la=None, lr=None, grad=False):
    from oracle import cpt_oracle as O
    cfg = m.config
    osd = {k: v.detach().cpu().clone().requires_grad_(grad) for k, v in m.state_dict().items()}
    outs = []
    for blk, key, lab in ((qa, "cls_ans", la), (qr, "cls_rat", lr)):
        outs.append(O.nsp_cpt_forward(osd, cfg.to_dict(), blk["input_ids"], blk["token_type_ids"], blk["attention_mask"], blk["img_feats"],
                                      next_sentence_label=lab, w_key=key + ".weight", b_key=key + ".bias"))
    return osd, outs


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
def test_scores_and_loss_match_oracle(dev, mode):
    m = _model(_cfg(), dev, mode).eval()
    qa, qr = _batch()
    la, lr = _labels()
    _, ((lo_a, rel_a), (lo_r, rel_r)) = _oracle(m, qa, qr, la, lr)
    with torch.no_grad():
        loss, ga, gr = m.qar_forward(_to(qa, dev), _to(qr, dev), la, lr)
    tol = 2e-5 if mode == "fp32" else 5e-3
    assert (ga.cpu() - rel_a).abs().max().item() < tol
    assert (gr.cpu() - rel_r).abs().max().item() < tol
    assert abs(loss.item() - (lo_a + lo_r).item()) < (1e-5 if mode == "fp32" else 5e-3)
    if mode == "fp32":        # the choice of evaluate() on our scores equals the one on the oracle's
        ref = S.vcr_qar_choose_reference(S.choice_scores(rel_a), S.choice_scores(rel_r), [2, 0], [1, 3], 4, 4)
        got = S.vcr_qar_choose_reference(S.choice_scores(ga.cpu()), S.choice_scores(gr.cpu()), [2, 0], [1, 3], 4, 4)
        assert [r["answer"] for r in got] == [r["answer"] for r in ref]


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("n_rats", [4, 16])
def test_one_pass_bit_identical_to_two_forwards(dev, mode, n_rats):
    """The encoder is batch-invariant (as test_gpu_dp.py asserts) and both routes run the same head kernel: the same bits per sequence."""
    m = _model(_cfg(), dev, mode).eval()
    qa, qr = _batch(n_q=4, n_rats=n_rats, seed=5)
    qa, qr = _to(qa, dev), _to(qr, dev)
    with torch.no_grad():
        a, r, sc = m.qar_forward(qa, qr, return_scores=True)
        a2 = m(qa["input_ids"], qa["token_type_ids"], qa["attention_mask"], img_feats=qa["img_feats"], head="ans")[0]
        r2 = m(qr["input_ids"], qr["token_type_ids"], qr["attention_mask"], img_feats=qr["img_feats"], head="rat")[0]
        none = m(qa["input_ids"], qa["token_type_ids"], qa["attention_mask"], img_feats=qa["img_feats"], head="")
    assert torch.equal(a, a2) and torch.equal(r, r2)
    assert none == (None,)
    assert torch.equal(sc, S.choice_scores(torch.cat([a, r], 0))) or (sc - S.choice_scores(torch.cat([a, r], 0))).abs().max().item() < 1e-6


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_training_gradients_match_oracle(dev, mode):
    cfg = _cfg()
    m = _model(cfg, dev, mode).train()
    qa, qr = _batch()
    la, lr = _labels()
    loss, ga, gr = m.qar_forward(_to(qa, dev), _to(qr, dev), la, lr)
    loss.backward()
    osd, ((lo_a, _), (lo_r, _)) = _oracle(m, qa, qr, la, lr, grad=True)
    (lo_a + lo_r).backward()
    ltol, gtol = {"fp32": (1e-5, 2e-4), "bf16": (5e-3, 8e-2)}[mode]
    assert abs(loss.item() - (lo_a + lo_r).item()) < ltol
    named = dict(m.named_parameters())
    worst = 0.0
    for name, prm in named.items():
        ref = osd[name].grad
        if ref is None or prm.grad is None:
            assert ref is None or float(ref.abs().max()) == 0.0, name
            continue
        if float(ref.abs().max()) < 1e-6 and float(prm.grad.abs().max()) < (1e-3 if mode == "bf16" else 1e-5):
            continue                     # key bias: true gradient 0 (softmax is shift-invariant), rounding noise on both sides
        got = prm.grad.double().cpu().flatten()
        r = ref.double().flatten()
        e = float((got - r).norm() / (r.norm() + 1e-30))
        worst = max(worst, e)
        assert e < gtol, (name, e)
    assert named["cls_rat.weight"].grad.abs().max() > 0 and named["cls_ans.weight"].grad.abs().max() > 0
    print("VCR Q->AR %s: loss %.6f, worst relative gradient error %.2e" % (mode, loss.item(), worst))
    # the same backward twice: bit-identical head gradients (fixed-order sums, no float atomics)
    first = {n: named[n].grad.clone() for n in ("cls_ans.weight", "cls_ans.bias", "cls_rat.weight", "cls_rat.bias", "bert.pooler.dense.weight")}
    m.zero_grad()
    loss2 = m.qar_forward(_to(qa, dev), _to(qr, dev), la, lr)[0]
    loss2.backward()
    assert torch.equal(loss2.detach(), loss.detach())
    for n, v in first.items():
        assert torch.equal(named[n].grad, v), n


def test_single_head_training_and_stale_backward(dev):
    """forward(head=..., next_sentence_label) trains through the same kernel (B0 = B / 0); the reference's two training forwards before one
    backward raise the engine's clear error instead of giving a wrong gradient."""
    m = _model(_cfg(), dev, "fp32").train()
    qa, qr = _batch()
    qa, qr = _to(qa, dev), _to(qr, dev)
    la, lr = _labels()
    la, lr = la.to(dev), lr.to(dev)
    l1, _ = m(qa["input_ids"], qa["token_type_ids"], qa["attention_mask"], next_sentence_label=la, img_feats=qa["img_feats"], head="ans")
    l2, _ = m(qr["input_ids"], qr["token_type_ids"], qr["attention_mask"], next_sentence_label=lr, img_feats=qr["img_feats"], head="rat")
    with pytest.raises(RuntimeError, match="stale|backward called twice"):      # (autograd runs the later forward's backward first)
        (l1 + l2).backward()
    m.zero_grad()
    l1, _ = m(qa["input_ids"], qa["token_type_ids"], qa["attention_mask"], next_sentence_label=la, img_feats=qa["img_feats"], head="ans")
    l1.backward()
    with torch.no_grad():
        lq = m.qar_forward(qa, qr, la, lr)[0]
    _, ((lo_a, _), (lo_r, _)) = _oracle(m, {k: v.cpu() for k, v in qa.items()}, {k: v.cpu() for k, v in qr.items()}, la.cpu(), lr.cpu())
    assert abs(l1.item() - lo_a.item()) < 1e-5 and abs(lq.item() - (lo_a + lo_r).item()) < 1e-5
    assert float(m.cls_rat.weight.grad.abs().max()) == 0.0 and float(m.cls_ans.weight.grad.abs().max()) > 0


def _random_scores(seed, n_q, n_ans, n_rats):
    g = torch.Generator().manual_seed(seed)
    qa = torch.randint(0, 3, (n_q * n_ans,), generator=g).float() / 2      # few distinct values: ties everywhere
    qr = torch.randint(0, 3, (n_q * n_rats,), generator=g).float() / 2
    qa[torch.randperm(qa.numel(), generator=g)[: qa.numel() // 9]] = float("nan")
    qr[torch.randperm(qr.numel(), generator=g)[: qr.numel() // 9]] = float("nan")
    al = torch.randint(0, n_ans, (n_q,), generator=g)
    rl = torch.randint(0, n_rats if n_rats <= n_ans else n_ans, (n_q,), generator=g)
    return qa, qr, al, rl


@pytest.mark.parametrize("n_rats", [4, 16])
def test_device_choose_matches_reference(dev, n_rats):
    n_q, n_ans = 300, 4
    qa, qr, al, rl = _random_scores(7 + n_rats, n_q, n_ans, n_rats)
    ref = S.vcr_qar_choose_reference(qa, qr, al.tolist(), rl.tolist(), n_ans, n_rats)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    preds, flags = S.vcr_qar_choose_device(qa.to(dev), qr.to(dev), al, rl, n_ans, n_rats, counts=counts)
    preds, flags = preds.cpu(), flags.cpu()
    assert preds.tolist() == [r["answer"] for r in ref]
    assert flags[:, 2].bool().tolist() == [r["correct"] for r in ref]
    assert flags[:, 0].tolist() == [int(r["gt"][0] == r["answer"][0]) for r in ref]
    assert flags[:, 1].tolist() == [int(r["gt"][1] == r["answer"][1]) for r in ref]
    assert counts.cpu().tolist() == flags.long().sum(0).tolist()
    S.vcr_qar_choose_device(qa.to(dev), qr.to(dev), al, rl, n_ans, n_rats, counts=counts)       # accumulates
    assert counts.cpu().tolist() == (2 * flags.long().sum(0)).tolist()


def test_abi_error_codes(dev):
    from cpt_amd import _lib as L
    lib = L.lib()
    B, H, n_rel = 8, 64, 2
    pooled = torch.randn(B, H, device=dev)
    w = torch.randn(n_rel, H, device=dev)
    b = torch.randn(n_rel, device=dev)
    rel = torch.empty(B, n_rel, device=dev)
    dl = torch.empty(B, n_rel, device=dev)
    loss = torch.empty(3, device=dev)
    ws = torch.zeros(lib.cpt_rel2_workspace_bytes(B), dtype=torch.uint8, device=dev)
    st = L.stream_ptr()

    def call(B0=4, lab=None, labh=None, w1=w, nrel=n_rel):
        return lib.cpt_rel2_scores(L.CPT_F32, pooled.data_ptr(), B, H, nrel, B0, w.data_ptr(), b.data_ptr(), L.ptr(w1), b.data_ptr(),
                                   L.ptr(lab), labh.ctypes.data if labh is not None else None, rel.data_ptr(), None, loss.data_ptr(),
                                   loss.data_ptr() + 8, dl.data_ptr(), ws.data_ptr(), ws.numel(), st)
    good = torch.tensor([0, 1, -1, 1, 0, 0, 1, 1], device=dev)
    assert call(lab=good) == 0
    assert call(B0=-1) == -1
    assert call(B0=B + 1) == -1
    assert call(nrel=65) == -1
    assert call(w1=None) == -6
    assert call(lab=torch.tensor([0, 1, 2, 0, 0, 0, 0, 0], device=dev)) == -1                 # device labels, read back
    assert call(lab=good, labh=np.array([0, 1, -2, 0, 0, 0, 0, 0], dtype=np.int64)) == -1     # host copy checked
    # the training entry: bad B0 and a missing second head
    m = _model(_cfg(), dev, "fp32").train()
    eng = m._engine()
    eng.ensure_packed()
    eng.refresh_shadow(train=True)
    from cpt_amd import train as T
    st_ = T._state(eng)
    st_.ensure()
    qa, qr = _batch()
    ids = torch.cat([qa["input_ids"], qr["input_ids"]]).to(dev)
    msk = torch.cat([qa["attention_mask"], qr["attention_mask"]]).to(dev)
    feats = torch.cat([qa["img_feats"], qr["img_feats"]]).to(dev)
    labels = torch.zeros(ids.size(0), dtype=torch.int64, device=dev)
    md, _ = eng.descriptor(train=True)
    bt = L.Batch(B=ids.size(0), Lt=ids.size(1), Li=feats.size(1), input_ids=ids.data_ptr(), attn_mask=msk.data_ptr(), img_feats=feats.data_ptr(),
                 labels=labels.data_ptr())
    relo = torch.empty(ids.size(0), 2, device=dev)
    lo = torch.empty(3, device=dev)
    o = L.Outputs(rel=relo.data_ptr(), loss=lo.data_ptr())
    wsp = st_.workspace(ids.size(0), ids.size(1), feats.size(1))
    for B0, w1, rc in ((ids.size(0) + 1, True, -1), (-3, True, -1), (8, False, -6)):
        x = T.rel2_desc(eng, st_, B0)
        if not w1:
            x.w_rel1 = None
        got = lib.cpt_train_fwd_rel2(C.byref(md), C.byref(x), C.byref(bt), C.byref(o), wsp.data_ptr(), wsp.numel(), L.stream_ptr(), L.NULL_CB, None, None)
        assert got == rc, (B0, w1, got)
    torch.cuda.synchronize()


def _tok():
    from transformers import BertTokenizer
    g = np.load(os.path.join(GOLDEN, "tiny_gqa_vcr_prompts.npz"))
    d = tempfile.mkdtemp()
    vf = os.path.join(d, "vocab.txt")
    with open(vf, "w") as f:
        f.write("\n".join(str(w) for w in g["vocab"]) + "\n")
    return BertTokenizer(vf, do_lower_case=True)


def _questions(n_q=5, n_rats=4, Li=5, dim=None, seed=3):
    from cpt_amd import prompts
    tok = _tok()
    rng = np.random.Generator(np.random.PCG64(seed))
    colors, names = {"0": "red", "1_2": "blue"}, {"0": "person", "1_2": "dog and cat", "3": "table", "1": "dog", "2": "cat"}
    words = ["the", "dog", "cat", "is", "on", "table", "holding", "cup", "because", "she", "wants", "it", "sitting", "next", "to"]
    dim = dim or _cfg().img_feature_dim
    out = []
    for q in range(n_q):
        sent = lambda n: [words[i] if i < len(words) else [int(i - len(words))] for i in rng.integers(0, len(words) + 3, n)]
        qd = prompts.assemble_vcr_qar(tok, sent(5), [sent(4) for _ in range(4)], [sent(5) for _ in range(n_rats)], colors, names, Li,
                                      label=(q % 4, (2 * q) % 4), q_id=100 + q, max_seq_length=24, max_img_seq_length=Li)
        qd["img_feats"] = torch.from_numpy(rng.standard_normal((Li, dim)).astype(np.float32))
        out.append(qd)
    return out


def test_val_vcr_qar_world1(dev):
    from cpt_amd import drivers
    m = _model(_cfg(), dev, "fp32").eval()
    qs = _questions()
    res = drivers.val_vcr_qar(m, qs, dev, batch_questions=2)
    # yardstick: per question two forward(head=...) calls and the host restatement of evaluate()
    results = []
    for q in qs:
        blk = drivers._qar_blocks([q], dev)
        with torch.no_grad():
            a = m(blk[0]["input_ids"], blk[0]["token_type_ids"], blk[0]["attention_mask"], img_feats=blk[0]["img_feats"], head="ans")[0]
            r = m(blk[1]["input_ids"], blk[1]["token_type_ids"], blk[1]["attention_mask"], img_feats=blk[1]["img_feats"], head="rat")[0]
        results += S.vcr_qar_choose_reference(S.choice_scores(a.cpu()), S.choice_scores(r.cpu()), [q["label"][0]], [q["label"][1]], 4, 4,
                                              q_ids=[q["q_id"]])
    assert res["preds"].tolist() == [x["answer"] for x in results]
    assert res["flags"][:, 2].bool().tolist() == [x["correct"] for x in results]
    assert res["acc"]["q_ar"] == S.vcr_qar_accuracy(results, len(qs))


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
        m = _model(_cfg(), dev, "fp32").eval()
        res = drivers.val_vcr_qar(m, _questions(), dev, batch_questions=2)
        torch.save(res, os.path.join(tmp, "v%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_val_vcr_qar_two_ranks_equal_single_process(dev):
    from cpt_amd import drivers
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_val_worker, args=(2, _free_port(), tmp), nprocs=2, join=True)
        r = [torch.load(os.path.join(tmp, "v%d.pt" % i)) for i in range(2)]
    m = _model(_cfg(), dev, "fp32").eval()
    want = drivers.val_vcr_qar(m, _questions(), dev, batch_questions=2)
    for x in r:
        assert torch.equal(x["preds"], want["preds"]) and torch.equal(x["flags"], want["flags"])
        assert torch.equal(x["scores"], want["scores"]) and x["acc"] == want["acc"]


def test_train_vcr_qar_batch(dev, tmp_path):
    """The driver's order -- per-micro-step clipping, scheduler before optimizer, one step per accumulation window -- equals a loop written
    out in the reference's order on an identical model; a few windows lower the loss; a checkpoint round trip reproduces the scores."""
    from cpt_amd import drivers
    from cpt_amd.train import AdamW, WarmupLinearSchedule, save_checkpoint, load_checkpoint
    cfg = _cfg()
    qs = _questions(n_q=4, seed=9)
    batches = [[q] for q in qs]
    gas, t_total = drivers.qar_accumulation(len(qs), 1, 1, len(batches), num_train_epochs=3)
    assert (gas, t_total) == (4, 3)
    opts = types.SimpleNamespace(gradient_accumulation_steps=gas, max_grad_norm=1.0)
    m = _model(cfg, dev, "fp32")
    opt = AdamW(m, lr=1e-3, eps=1e-6, weight_decay=0.01)
    sch = WarmupLinearSchedule(opt, warmup_steps=1, t_total=t_total)
    step, losses = drivers.train_vcr_qar_batch(m, opt, sch, batches, opts, dev)
    assert step == 1
    # the same window, by hand, in the reference's order
    m2 = _model(cfg, dev, "fp32").train()
    opt2 = AdamW(m2, lr=1e-3, eps=1e-6, weight_decay=0.01)
    sch2 = WarmupLinearSchedule(opt2, warmup_steps=1, t_total=t_total)
    for i, chunk in enumerate(batches):
        qa, qr = drivers._qar_blocks(chunk, dev)
        la, lr = S.qar_choice_labels([chunk[0]["label"][0]], [chunk[0]["label"][1]], 4, 4)
        loss = m2.qar_forward(qa, qr, la, lr)[0] / gas
        assert torch.equal(loss.detach(), losses[i])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m2.parameters(), 1.0)
    sch2.step()
    opt2.step()
    m2.zero_grad()
    # (the bias / LayerNorm gradients of the encoder's backward are summed with float atomics: a last-bit difference there moves an updated
    # parameter by an ulp, never by a step)
    for (n, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert (p.detach() - p2.detach()).abs().max().item() <= 1e-6, n
    # more windows lower the loss
    first = sum(l.item() for l in losses)
    for _ in range(2):
        step, losses = drivers.train_vcr_qar_batch(m, opt, sch, batches, opts, dev, global_step=step)
    assert step == 3 and sum(l.item() for l in losses) < first
    # checkpoint round trip
    m.eval()
    want = drivers.val_vcr_qar(m, qs, dev)["scores"]
    save_checkpoint(str(tmp_path), m, opt, global_step=step)
    m3 = _model(cfg, dev, "fp32", seed=99).eval()
    load_checkpoint(str(tmp_path), m3)
    assert torch.equal(drivers.val_vcr_qar(m3, qs, dev)["scores"], want)


# ---- against the reference's own VCRQAR_NSPCPT and evaluate() (tools/make_golden_vcr_qar.py) ----------------------------------------------
def _gold_model(dev, mode, train=False):
    """The fixture's model: synth pretrain weights through copy_from_pretraining_model, cls_rat as the fixture moved it."""
    from cpt_amd.modeling_bert import BertImgForPreTraining
    from cpt_amd.modeling_vcr import VCRQAR_NSPCPT
    g = np.load(os.path.join(GOLDEN, "tiny_vcr_qar_model.npz"))
    cfg = _cfg()
    pre = BertImgForPreTraining(cfg)
    pre.load_state_dict(synth.init_state_dict(cfg, 4321, head="pretrain"))
    pre.tie_weights()
    m = VCRQAR_NSPCPT(cfg)
    m.copy_from_pretraining_model(pre)
    with torch.no_grad():
        m.cls_rat.weight.copy_(torch.from_numpy(g["cls_rat_weight"]))
        m.cls_rat.bias.copy_(torch.from_numpy(g["cls_rat_bias"]))
    assert list(m.state_dict().keys()) == [str(k) for k in g["keys"]]
    m.to(dev).set_compute_dtype(mode)
    m.train() if train else m.eval()
    b = {k[3:]: torch.from_numpy(g[k]).to(dev) for k in g.files if k.startswith("in_")}
    blk = lambda lo, hi: {"input_ids": b["input_ids"][lo:hi], "token_type_ids": b["segment_ids"][lo:hi],
                          "attention_mask": b["attention_mask"][lo:hi], "img_feats": b["img_feats"][lo:hi]}
    return m, g, blk(0, 8), blk(8, 16)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
def test_scores_loss_and_choice_match_reference_fixture(dev, mode):
    m, g, qa, qr = _gold_model(dev, mode)
    la, lr = S.qar_choice_labels(g["ans"].tolist(), g["rat"].tolist(), 4, 4)
    with torch.no_grad():
        loss, a, r, sc = m.qar_forward(qa, qr, la, lr, return_scores=True)
        a2 = m(qa["input_ids"], qa["token_type_ids"], qa["attention_mask"], img_feats=qa["img_feats"], head="ans")[0]
    tol = 2e-5 if mode == "fp32" else 5e-3
    assert (a.cpu() - torch.from_numpy(g["q_a_rel"])).abs().max().item() < tol
    assert (r.cpu() - torch.from_numpy(g["qa_r_rel"])).abs().max().item() < tol
    assert torch.equal(a, a2)
    assert abs(loss.item() - float(g["loss"])) < (1e-5 if mode == "fp32" else 5e-3)
    ref = S.vcr_qar_choose_reference(S.choice_scores(torch.from_numpy(g["q_a_rel"])), S.choice_scores(torch.from_numpy(g["qa_r_rel"])),
                                     g["ans"].tolist(), g["rat"].tolist(), 4, 4)
    preds, _ = S.vcr_qar_choose_device(sc[:8], sc[8:], g["ans"].tolist(), g["rat"].tolist(), 4, 4)
    if mode == "fp32":
        assert preds.cpu().tolist() == [x["answer"] for x in ref]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_training_gradients_match_reference_fixture(dev, mode):
    """loss.backward() of qar_forward against the autograd gradients of the reference's own q_a_loss + qa_r_loss (bounds of
    test_vcr_nspcpt_finetune_gradients)."""
    m, g, qa, qr = _gold_model(dev, mode, train=True)
    la, lr = S.qar_choice_labels(g["ans"].tolist(), g["rat"].tolist(), 4, 4)
    loss, _, _ = m.qar_forward(qa, qr, la, lr)
    loss.backward()
    ltol, gtol = {"fp32": (1e-5, 2e-4), "bf16": (5e-3, 8e-2)}[mode]
    assert abs(loss.item() - float(g["loss"])) < ltol
    named = dict(m.named_parameters())
    for name, key in (("cls_ans.weight", "grad_cls_ans_weight"), ("cls_ans.bias", "grad_cls_ans_bias"), ("cls_rat.weight", "grad_cls_rat_weight"),
                      ("cls_rat.bias", "grad_cls_rat_bias"), ("bert.pooler.dense.weight", "grad_pooler_weight"),
                      ("bert.encoder.layer.0.attention.self.query.weight", "grad_q0_weight")):
        got = named[name].grad.double().cpu().flatten()
        ref = torch.from_numpy(g[key]).double().flatten()
        assert float((got - ref).norm() / (ref.norm() + 1e-30)) < gtol, name


@pytest.mark.parametrize("layout", ["r4", "r16"])
def test_device_choose_matches_reference_evaluate(dev, layout):
    """cpt_vcr_qar_choose on the fixture's relation scores gives what the reference evaluate() pickled, and its counts give its acc (no repeated
    questionId has a different outcome here: the counts are over all rows)."""
    g = np.load(os.path.join(GOLDEN, "tiny_vcr_qar_eval.npz"))
    k = layout + "_"
    n_rats = int(g[k + "n_rats"])
    qa = S.choice_scores(torch.from_numpy(g[k + "q_a_rel"])).to(dev)
    qr = S.choice_scores(torch.from_numpy(g[k + "qa_r_rel"])).to(dev)
    preds, flags = S.vcr_qar_choose_device(qa, qr, g[k + "ans"].tolist(), g[k + "rat"].tolist(), 4, n_rats)
    assert preds.cpu().tolist() == g[k + "answer"].tolist()
    assert flags[:, 2].bool().cpu().tolist() == g[k + "correct"].tolist()
    res = [{"questionId": int(q), "correct": bool(c)} for q, c in zip(g[k + "q_ids"], flags[:, 2].cpu().tolist())]
    assert S.vcr_qar_accuracy(res, len(res)) == float(g[k + "acc"])


def test_device_choose_negative_answer_labels_follow_python_slices(dev):
    """16-rationale layout with answer labels the data never holds (-4 .. -2): the slice x[al * n_ans : (al + 1) * n_ans] by Python's rules, as
    the host restatement takes it (-1 is left out: its slice is empty and the reference's argmax raises)."""
    n_q, n_ans, n_rats = 60, 4, 16
    qa, qr, _, rl = _random_scores(31, n_q, n_ans, n_rats)
    al = torch.tensor([-4, -3, -2] * (n_q // 3))
    ref = S.vcr_qar_choose_reference(qa, qr, al.tolist(), rl.tolist(), n_ans, n_rats)
    preds, _ = S.vcr_qar_choose_device(qa.to(dev), qr.to(dev), al, rl, n_ans, n_rats)
    assert preds.cpu().tolist() == [x["answer"] for x in ref]
    preds, _ = S.vcr_qar_choose_device(qa.to(dev), qr.to(dev), [-1] * n_q, rl, n_ans, n_rats)
    assert (preds[:, 1] == -1).all()
