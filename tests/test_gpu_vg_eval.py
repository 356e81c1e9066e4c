"""GPU: VG-CPT Recall@K on the device (include/cpt_hip.h cpt_vg_recall_ranks; scoring.vg_recall_device) against the host restatement
of eval_vg and the reference's own string (tests/golden/tiny_vg_eval.npz), and the VG drivers (drivers.val_vg, train_vg_batch) on the
tiny model and the committed VG rows."""
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
PREDICATES = {"1": "on", "2": "has", "3": "next to", "4": "in front of", "5": "wears", "6": "near", "7": "with"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _gts(gold):
    gts, off = [], 0
    for img, n in zip(gold["gt_imgs"], gold["gt_counts"]):
        gts.append({"img_path": str(img), "relations": gold["gt_rels"][off:off + int(n)]})
        off += int(n)
    return gts


def _close(a, b, tol=1e-12):
    for part in ("recall", "mrecall"):
        for K in a[part]:
            assert abs(a[part][K] - b[part][K]) <= tol, (part, K, a[part][K], b[part][K])


def test_fixture_ranks_and_reference_string(dev):
    gold = np.load(os.path.join(GOLDEN, "tiny_vg_eval.npz"))
    keys = [str(k) for k in gold["pred_keys"]]
    preds = {k: torch.from_numpy(v.copy()) for k, v in zip(keys, gold["pred_scores"])}
    ref = S.eval_vg_reference(preds, _gts(gold))
    table = S.vg_eval_table(keys, _gts(gold))
    got = S.vg_recall_device(torch.from_numpy(gold["pred_scores"]).to(dev), table)
    assert torch.equal(got["ranks"].cpu().long(), ref["ranks"])
    assert S.format_vg_recall(got) == str(gold["eval_string"]) == ref["string"]
    _close(got, ref)


def _random_split(seed, n_img=2000, C=51):
    """Ragged candidate counts 1 .. past the LDS tile (4096), integer-valued scores (ties inside rows and across candidates, also at
    the K boundaries), -inf and NaN scores, images without prediction, ground truth on predicted and unpredicted pairs."""
    rng = np.random.Generator(np.random.PCG64(seed))
    counts = rng.integers(1, 160, size=n_img)
    counts[rng.choice(n_img, 6, replace=False)] = [4096, 4097, 4200, 4700, 5000, 4095]
    keys, rows, gts = [], [], []
    for i, n in enumerate(counts):
        img = "%d.jpg" % i
        if i % 97 == 5:                       # no prediction: the dummy candidate
            gts.append({"img_path": img, "relations": np.array([[0, 0, 1], [0, 1, 2]])})
            continue
        boxes = int(np.ceil((1 + np.sqrt(1 + 4 * n)) / 2)) + 1
        allp = [(s, o) for s in range(boxes) for o in range(boxes) if s != o]
        pick = rng.permutation(len(allp))[:n]
        pairs = [allp[j] for j in pick]
        sc = rng.integers(-4, 5, size=(n, C)).astype(np.float32)
        if i % 3 == 0:
            sc[rng.random((n, C)) < 0.05] = -np.inf
        if i % 5 == 0:
            sc[rng.random((n, C)) < 0.02] = np.nan
        if i % 7 == 0:
            sc[rng.random(n) < 0.3] = -np.inf         # whole rows of -inf
        for (s, o), r in zip(pairs, sc):
            keys.append("%s_%d_%d" % (img, s, o))
            rows.append(r)
        ng = int(rng.integers(1, 12))
        rel = []
        for _ in range(ng):
            j = int(rng.integers(0, n))
            s, o = pairs[j]
            r = sc[j, 1:]
            if rng.random() < 0.6 and not np.isnan(r).any():
                pr = int(np.argmax(r)) + 1
            else:
                pr = int(rng.integers(0, C))
            if rng.random() < 0.1:
                s, o = boxes + 1, 0                     # a pair never predicted
            rel.append([s, o, pr])
        gts.append({"img_path": img, "relations": np.array(rel)})
    return keys, np.stack(rows), gts


def test_random_split_matches_restatement(dev):
    keys, rows, gts = _random_split(7)
    preds = {k: torch.from_numpy(r) for k, r in zip(keys, rows)}
    ref = S.eval_vg_reference(preds, gts)
    table = S.vg_eval_table(keys, gts)
    got = S.vg_recall_device(torch.from_numpy(rows).to(dev), table)
    ranks = got["ranks"].cpu().long()
    assert int((ranks < 0).sum()) == 0
    bad = (ranks != ref["ranks"]).nonzero().view(-1)
    assert bad.numel() == 0, (bad[:10].tolist(), ranks[bad[:10]].tolist(), ref["ranks"][bad[:10]].tolist())
    _close(got, ref)
    # other K: hit@K = rank < K straight from the same ranks
    _close(S.vg_recall_from_ranks(got["ranks"], table, modes=(1, 5, 4096, 4097)), S.eval_vg_reference(preds, gts, modes=(1, 5, 4096, 4097)))


# ---- drivers on the tiny model and the committed VG rows -----------------------------------------------------------------------------
def _tok():
    transformers = pytest.importorskip("transformers")
    gold = np.load(os.path.join(GOLDEN, "tiny_vg_eval.npz"))
    d = tempfile.mkdtemp()
    vf = os.path.join(d, "vocab.txt")
    with open(vf, "w") as f:
        f.write("\n".join(str(w) for w in gold["vocab"]) + "\n")
    return transformers.BertTokenizer(vf, do_lower_case=True)


def _rows(train=False):
    from cpt_amd import io, prompts
    tok = _tok()
    tsv = io.TSVFile(os.path.join(GOLDEN, "tiny_vg_rows.tsv"))
    out = []
    for i in range(tsv.num_rows()):
        name, payload = tsv.seek_raw(i)
        name = name.decode() if isinstance(name, bytes) else name
        info, feats, fmask, counts = io.decode_row(payload, img_seq_len=60)
        q = (prompts.assemble_vg_train if train else prompts.assemble_vg_zsl)(tok, name, info)
        q = {"img_key": name, "input_ids": torch.from_numpy(q["input_ids"]), "segment_ids": torch.from_numpy(q["segment_ids"]),
             "attention_mask": torch.from_numpy(q["input_mask"]), "mask_token_pos": torch.from_numpy(q["mask_token_pos"]),
             "img_feats": feats[0], **({"row_labels": torch.from_numpy(q["row_labels"])} if train else {})}
        out.append(q)
    return out, prompts.vg_predicates(PREDICATES, tok)


def _cfg():
    return cfgmod.tiny(max_position_embeddings=80, img_feature_dim=2054, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def _model(cfg, dev, mode, train=False):
    from cpt_amd.modeling_rec import REC_MLM_CPT
    m = REC_MLM_CPT(cfg)
    sd = synth.init_state_dict(cfg, 31, head="cpt")
    m.load_state_dict(sd)
    m.tie_weights()
    m.to(dev)
    m.train() if train else m.eval()
    m.set_compute_dtype(mode)
    return m, sd


VG_GTS = [{"img_path": "10.jpg", "relations": np.array([[0, 1, 1], [2, 0, 3], [1, 2, 5], [1, 0, 2]])},
          {"img_path": "20.jpg", "relations": np.array([[1, 0, 4], [0, 1, 6]])},
          {"img_path": "30.jpg", "relations": np.array([[0, 1, 1]])}]


def _dict(keys, scores):
    preds = {}
    for k, v in zip(keys, scores.reshape(-1, scores.shape[-1])):
        preds[k] = v                                   # val()'s predictions[k] = v: first position, last value
    return preds


def test_val_vg_end_to_end_fp32(dev):
    from cpt_amd import drivers
    pairs, idx2pred = _rows()
    cfg = _cfg()
    m, _ = _model(cfg, dev, "fp32")
    scores, keys = drivers.val_vg(m, pairs, idx2pred, dev, batch_pairs=3)
    assert scores.shape == (4, 2, 8) and len(keys) == 8 and keys[1] == "10.jpg_1_0" and keys[2] == "10.jpg_1_0"
    b = drivers._vg_cat(pairs, dev, 6)
    with torch.no_grad():
        direct = S.vg_predicate_scores(m, b["input_ids"], b["segment_ids"], b["attention_mask"], b["img_feats"], b["mask_token_pos"], idx2pred)
        full = m(b["input_ids"], b["segment_ids"], b["attention_mask"], img_feats=b["img_feats"], mask_token_pos=b["mask_token_pos"])[0]
    assert torch.equal(scores, direct)
    seq = b["mask_token_pos"][:, 0].cpu()
    per_seq = [full[seq == s].cpu() for s in range(24)]
    ref_scores = S.vg_val_scores_reference(per_seq, idx2pred)
    assert (ref_scores - scores.cpu()).abs().max().item() < 1e-4
    got = S.vg_recall_device(scores, S.vg_eval_table(keys, VG_GTS))
    ref = S.eval_vg_reference(_dict(keys, ref_scores), VG_GTS)
    assert torch.equal(got["ranks"].cpu().long(), ref["ranks"])
    assert S.format_vg_recall(got) == ref["string"]
    _close(got, ref)


def test_val_vg_bf16_own_scores(dev):
    from cpt_amd import drivers
    pairs, idx2pred = _rows()
    m, _ = _model(_cfg(), dev, "bf16")
    scores, keys = drivers.val_vg(m, pairs, idx2pred, dev)
    assert bool(torch.isfinite(scores[:, :, 1:]).all())
    got = S.vg_recall_device(scores, S.vg_eval_table(keys, VG_GTS))
    ref = S.eval_vg_reference(_dict(keys, scores.cpu()), VG_GTS)
    assert torch.equal(got["ranks"].cpu().long(), ref["ranks"])
    _close(got, ref)


def test_vg_few_shot_step_fp32(dev):
    from cpt_amd import drivers
    from cpt_amd.train import build_optimizer, get_lr_sched
    from oracle import cpt_oracle as O
    pairs, _ = _rows(train=True)
    cfg = _cfg()
    m, sd = _model(cfg, dev, "fp32", train=True)
    batch = {k: torch.cat([q[k] for q in pairs], 0) for k in ("input_ids", "segment_ids", "attention_mask", "row_labels")}
    batch["img_feats"] = torch.cat([q["img_feats"][None].expand(3, -1, -1) for q in pairs], 0).contiguous()
    batch["mask_token_pos"] = torch.cat([q["mask_token_pos"] + torch.tensor([3 * i, 0]) for i, q in enumerate(pairs)], 0)
    assert batch["mask_token_pos"].shape == (24, 2)
    grid = drivers.vg_label_grid(batch)
    assert int((grid != -1).sum()) == 24
    with torch.no_grad():
        x, _ = O.bert_img_forward(sd, cfg.to_dict(), batch["input_ids"], batch["segment_ids"], batch["attention_mask"], img_feats=batch["img_feats"])
        pos = batch["mask_token_pos"]
        want = torch.nn.functional.cross_entropy(O.lm_head(sd, cfg.to_dict(), x[pos[:, 0], pos[:, 1]]).double(), batch["row_labels"])
    opts = drivers.vg_schedule(types.SimpleNamespace(learning_rate=3e-5, weight_decay=0.01, betas=(0.9, 0.98), lr_mul=1.0), 3)
    opt = build_optimizer(m, opts)
    lrs, losses, step = [], [], 0
    for _ in range(4):
        step, ls = drivers.train_vg_batch(m, opt, [batch], opts, dev, global_step=step)
        lrs.append(opt.param_groups[0]["lr"])
        losses += ls
    print("VG few-shot loss %.8f oracle %.8f" % (losses[0].item(), want.item()))
    assert abs(losses[0].item() - want.item()) <= 1e-5
    assert step == 4 and all(torch.isfinite(l).all() for l in losses)
    assert lrs == [get_lr_sched(s, types.SimpleNamespace(learning_rate=3e-5, warmup_steps=0, num_train_steps=3)) for s in range(4)]
    assert lrs[3] == 1e-8 and lrs[0] == 3e-5


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
        pairs, idx2pred = _rows()
        m, _ = _model(_cfg(), dev, "fp32")
        scores, keys = drivers.val_vg(m, pairs, idx2pred, dev, batch_pairs=1)
        got = S.vg_recall_device(scores, S.vg_eval_table(keys, VG_GTS))
        torch.save({"scores": scores.cpu(), "keys": keys, "recall": got["recall"], "mrecall": got["mrecall"]}, os.path.join(tmp, "v%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_val_vg_two_ranks_equal_single_process(dev):
    from cpt_amd import drivers
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_val_worker, args=(2, _free_port(), tmp), nprocs=2, join=True)
        r = [torch.load(os.path.join(tmp, "v%d.pt" % i)) for i in range(2)]
    pairs, idx2pred = _rows()
    m, _ = _model(_cfg(), dev, "fp32")
    scores, keys = drivers.val_vg(m, pairs, idx2pred, dev, batch_pairs=1)
    got = S.vg_recall_device(scores, S.vg_eval_table(keys, VG_GTS))
    for x in r:
        assert x["keys"] == keys and torch.equal(x["scores"], scores.cpu())
        assert x["recall"] == got["recall"] and x["mrecall"] == got["mrecall"]
