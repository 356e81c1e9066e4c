"""CPU: soft-template prompt tuning -- the oracle construction the GPU tests compare against is pinned to the reference's own
TemplateEmbedding (tests/golden/soft_template_tiny.npz, tools/make_golden_soft_template.py), the Python surface (attach, checkpoints,
refusals, nearest_tokens) without a GPU."""
import os

import numpy as np
import pytest
import torch

import _softcheck as S
from cpt_amd import config as cfgmod
from cpt_amd import soft_prompt, synth
from oracle import cpt_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _tiny_model():
    from cpt_amd.modeling_bert import BertImgForPreTraining
    from cpt_amd.modeling_rec import REC_MLM_CPT
    ck = os.path.join(GOLDEN, "tiny_ckpt")
    cfg = cfgmod.BertConfig.from_pretrained(ck)
    pre = BertImgForPreTraining.from_pretrained(ck, config=cfg)
    m = REC_MLM_CPT(cfg)
    m.copy_from_pretraining_model(pre)
    return m.eval(), cfg


def _fixture():
    g = np.load(os.path.join(GOLDEN, "soft_template_tiny.npz"))
    b = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("in_")}
    return g, b


def test_fixture_holds_every_case():
    g, b = _fixture()
    ids = b["input_ids"]
    T = g["template"].shape[0]
    assert T == S.N_SLOTS
    slot = (ids > 0) & (ids < T)
    assert int((ids[0] == 3).sum()) == 2                                  # a slot used twice in one sequence
    assert int(((ids == 3).sum(1) > 0).sum()) >= 2                        # a slot used in several sequences
    assert bool((slot.sum(1) == 0).any())                                 # a sequence with no slot at all
    att = b["attention_mask"][:, :ids.size(1)] == 1
    assert bool(((ids == 0) & att).any())                                 # id 0 at an attended position
    used = sorted(int(i) for i in torch.unique(ids[slot]))
    assert used == sorted(S.USED)
    gt = g["grad_template"]
    for s in range(T):
        if s in used:
            assert np.abs(gt[s]).max() > 0
        else:
            assert not gt[s].any()                                        # slots never used: exactly zero


def test_oracle_construction_matches_reference_template_embedding():
    """word_embeddings rows 1:T replaced by the template, decoder a separate tensor: the oracle's scores, loss and the gradient of those
    rows agree with the reference's TemplateEmbedding within 1e-5 (the agreement the repository records between oracle and reference)."""
    g, b = _fixture()
    m, cfg = _tiny_model()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    tmpl = torch.from_numpy(g["template"])
    loss, grad, scores = S.oracle_step(sd, cfg.to_dict(), b, tmpl)
    assert abs(float(loss) - float(g["loss"])) < 1e-5
    assert float((scores - torch.from_numpy(g["scores"])).abs().max()) < 1e-5
    ref = torch.from_numpy(g["grad_template"])
    assert float((grad - ref).abs().max()) < 1e-5 * max(1.0, float(ref.abs().max()))
    assert float((grad - ref).norm() / ref.norm()) < 1e-5
    # ... and the construction is not the plain model: without the template the scores differ
    plain = O.rec_mlm_cpt_forward(sd, cfg.to_dict(), b["input_ids"], b["segment_ids"], b["attention_mask"], img_feats=b["img_feats"],
                                  mask_rows_only=b["mask_token_pos"])[0]
    assert float((plain - torch.from_numpy(g["scores"])).abs().max()) > 1e-3


def test_attach_copies_word_rows_and_freezes():
    m, cfg = _tiny_model()
    w = soft_prompt.attach(m)
    assert tuple(w.shape) == (21, cfg.hidden_size) and w.dtype == torch.float32
    assert torch.equal(w[1:], m.bert.embeddings.word_embeddings.weight[1:21])
    assert soft_prompt.KEY in m.state_dict()
    assert [n for n, p in m.named_parameters() if p.requires_grad] == [soft_prompt.KEY]
    assert soft_prompt.frozen_step(m)
    assert soft_prompt.attach(m) is w                                     # a second attach keeps the template
    soft_prompt.detach(m)
    assert soft_prompt.template_of(m) is None and soft_prompt.KEY not in m.state_dict()


def test_checkpoint_round_trip(tmp_path):
    from cpt_amd.modeling_rec import REC_MLM_CPT
    m, cfg = _tiny_model()
    w = soft_prompt.attach(m, n_slots=9)
    with torch.no_grad():
        w.add_(torch.randn(w.shape, generator=torch.Generator().manual_seed(5)) * 0.1)
    d = str(tmp_path)
    m.save_pretrained(d)
    assert soft_prompt.KEY in torch.load(os.path.join(d, "pytorch_model.bin"), map_location="cpu")
    m2, info = REC_MLM_CPT.from_pretrained(d, output_loading_info=True)
    w2 = soft_prompt.template_of(m2)
    assert w2 is not None and torch.equal(w2, w.detach())
    assert not info["unexpected_keys"] and not [k for k in info["missing_keys"]]
    for (n, p), (n2, p2) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert n == n2 and torch.equal(p, p2)


def test_checkpoint_without_template_loads_as_before(tmp_path):
    from cpt_amd.modeling_rec import REC_MLM_CPT
    m, cfg = _tiny_model()
    d = str(tmp_path)
    m.save_pretrained(d)
    m2 = REC_MLM_CPT.from_pretrained(d)
    assert soft_prompt.template_of(m2) is None
    assert list(m2.state_dict()) == list(m.state_dict())


def test_trainable_backbone_beside_template_raises():
    m, cfg = _tiny_model()
    soft_prompt.attach(m, freeze_backbone=False)
    b = synth.make_batch(2, cfg, seed=3, max_seq_len=20, img_seq_len=6)
    m.train()
    with pytest.raises(NotImplementedError, match="trainable backbone"):
        m(b["input_ids"], b["segment_ids"], b["attention_mask"], img_feats=b["img_feats"], masked_lm_labels=b["colors"],
          mask_token_pos=b["mask_token_pos"])


def test_nsp_and_qar_heads_refuse_template_training():
    from cpt_amd.modeling_bert import BertImgForPreTraining
    from cpt_amd.modeling_vcr import NSPCPT, VCRQAR_NSPCPT
    cfg = cfgmod.tiny()
    b = synth.make_batch(2, cfg, seed=3, max_seq_len=20, img_seq_len=6)
    lab = torch.tensor([0, 1])
    for cls, kw in ((NSPCPT, {}), (VCRQAR_NSPCPT, {"head": "ans"})):
        pre = BertImgForPreTraining(cfg)
        m = cls(cfg)
        m.copy_from_pretraining_model(pre)
        soft_prompt.attach(m)
        m.train()
        with pytest.raises(NotImplementedError, match="MLM head"):
            m(b["input_ids"], b["segment_ids"], b["attention_mask"], next_sentence_label=lab, img_feats=b["img_feats"], **kw)


def test_nearest_tokens_is_the_mlm_head_on_the_template_rows():
    m, cfg = _tiny_model()
    w = soft_prompt.attach(m)
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    want = O.lm_head(sd, cfg.to_dict(), w.detach()[None])[0]
    vals, ids = soft_prompt.nearest_tokens(m, k=5)
    wv, wi = want.topk(5, dim=-1)
    assert tuple(vals.shape) == (21, 5)
    assert torch.equal(ids, wi) and float((vals - wv).abs().max()) < 1e-5
