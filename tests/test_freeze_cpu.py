"""CPU: layer freezing (cpt_amd/train.py freeze_layers / freeze_embeddings / train_head_only / unfreeze) without a GPU -- the stage <->
``requires_grad`` mapping of the three model classes, the refusal of a flag pattern that is not a frozen prefix, the AdamW element range
and the data-parallel bucket subset as they follow from engine.bucket_table, and the optimizer's refusal of a stage change behind it."""
import os

import pytest
import torch

from cpt_amd import config as cfgmod
from cpt_amd import dist as cdist
from cpt_amd import engine, soft_prompt, train

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADS = ("cpt", "nsp", "qar")


def _model(head):
    from cpt_amd.modeling_bert import BertImgForPreTraining
    from cpt_amd.modeling_rec import REC_MLM_CPT
    from cpt_amd.modeling_vcr import NSPCPT, VCRQAR_NSPCPT
    ck = os.path.join(GOLDEN, "tiny_ckpt")
    cfg = cfgmod.BertConfig.from_pretrained(ck)
    pre = BertImgForPreTraining.from_pretrained(ck, config=cfg)
    m = {"cpt": REC_MLM_CPT, "nsp": NSPCPT, "qar": VCRQAR_NSPCPT}[head](cfg)
    m.copy_from_pretraining_model(pre)
    assert m._engine().head == head
    return m, cfg


def _flags(m):
    return {n: p.requires_grad for n, p in m._engine()._named().items()}


def _expected(m, s):
    nl = m.config.num_hidden_layers
    return {n: engine.bucket_of(n, nl) >= s for n in m._engine()._named()}


@pytest.mark.parametrize("head", HEADS)
def test_stage_sets_the_prefix_pattern(head):
    m, cfg = _model(head)
    N = cfg.num_hidden_layers
    assert N >= 2
    assert train.trainable_stage(m) == 0 and all(_flags(m).values())
    for s, call in [(1, lambda: train.freeze_embeddings(m)), (2, lambda: train.freeze_layers(m, 1)), (N, lambda: train.freeze_layers(m, N - 1)),
                    (N + 1, lambda: train.train_head_only(m)), (N + 1, lambda: train.freeze_layers(m, N)), (1, lambda: train.freeze_layers(m, 0))]:
        assert call() == s and train.trainable_stage(m) == s
        assert _flags(m) == _expected(m, s), s
        train.check_stage_flags(m)
        # every parameter of the module is an engine parameter: nothing is left with a stale flag
        by_id = {id(p) for p in m._engine()._named().values()}
        assert all(id(p) in by_id for p in m.parameters())
        f = _flags(m)
        assert not f["bert.embeddings.word_embeddings.weight"] and not f["bert.img_embedding.weight"] and not f["bert.embeddings.LayerNorm.weight"]
        assert f["bert.encoder.layer.%d.output.dense.weight" % (N - 1)] == (s <= N)
        assert f["bert.encoder.layer.0.attention.self.query.weight"] == (s <= 1)
        assert f["bert.pooler.dense.weight"]
        head_names = {"cpt": ["cls.bias", "cls.transform.dense.weight", "cls.transform.LayerNorm.weight"], "nsp": ["cls.weight", "cls.bias"],
                      "qar": ["cls_ans.weight", "cls_rat.weight", "cls_rat.bias"]}[head]
        assert all(f[n] for n in head_names)
    with pytest.raises(ValueError):
        train.freeze_layers(m, N + 1)
    with pytest.raises(ValueError):
        train.freeze_layers(m, -1)


def test_tied_decoder_is_frozen_with_the_word_table():
    """The decoder weight IS the word table (stage 0): one Parameter, so it cannot train above a frozen embedding side; cls.bias does."""
    m, cfg = _model("cpt")
    assert m.cls.decoder.weight is m.bert.embeddings.word_embeddings.weight
    for s in range(1, cfg.num_hidden_layers + 2):
        train._set_stage(m, s)
        assert not m.cls.decoder.weight.requires_grad and m.cls.bias.requires_grad and m.cls.transform.dense.weight.requires_grad
    # ... and switching the table back on by hand is refused, named
    m.bert.embeddings.word_embeddings.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r"bert\.embeddings\.word_embeddings\.weight"):
        train.check_stage_flags(m)


def test_pooler_under_the_mlm_head_is_outside_the_check():
    """REC_MLM_CPT: the pooler belongs to stage N + 1 and is set with it, but takes no part in the loss (train.NO_GRAD_PREFIXES): its flag is
    not part of the pattern that a training forward checks."""
    m, cfg = _model("cpt")
    train.train_head_only(m)
    assert m.bert.pooler.dense.weight.requires_grad and m.bert.pooler.dense.bias.requires_grad
    m.bert.pooler.dense.weight.requires_grad_(False)
    train.check_stage_flags(m)
    m2, _ = _model("nsp")                 # the NSP head trains its pooler: there the flag counts
    train.train_head_only(m2)
    m2.bert.pooler.dense.weight.requires_grad_(False)
    with pytest.raises(NotImplementedError, match=r"bert\.pooler\.dense\.weight"):
        train.check_stage_flags(m2)


@pytest.mark.parametrize("head", HEADS)
def test_non_prefix_pattern_is_refused_with_the_parameter_named(head):
    m, cfg = _model(head)
    N = cfg.num_hidden_layers
    # no stage set: flags are ignored, as before
    m.bert.encoder.layer[0].output.dense.weight.requires_grad_(False)
    train.check_stage_flags(m)
    m.bert.encoder.layer[0].output.dense.weight.requires_grad_(True)
    train.freeze_layers(m, 1)
    name = "bert.encoder.layer.%d.intermediate.dense.bias" % (N - 1)
    m.bert.encoder.layer[N - 1].intermediate.dense.bias.requires_grad_(False)          # a hole above the boundary
    with pytest.raises(NotImplementedError, match=name.replace(".", r"\.")):
        train.check_stage_flags(m)
    m.bert.encoder.layer[N - 1].intermediate.dense.bias.requires_grad_(True)
    m.bert.encoder.layer[0].attention.output.LayerNorm.weight.requires_grad_(True)      # a trainable tensor below it
    with pytest.raises(NotImplementedError, match=r"bert\.encoder\.layer\.0\.attention\.output\.LayerNorm\.weight"):
        train.check_stage_flags(m)
    # the training forward itself refuses, before anything touches the device
    ids = torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match=r"layer\.0\.attention\.output\.LayerNorm\.weight"):
        if head == "cpt":
            m(ids, masked_lm_labels=torch.tensor([5, 6]), mask_token_pos=torch.tensor([1, 2]))
        elif head == "nsp":
            m(ids, next_sentence_label=torch.tensor([0, 1]))
        else:
            m(ids, next_sentence_label=torch.tensor([0, 1]), head="ans")


@pytest.mark.parametrize("head", HEADS)
def test_adamw_range_and_bucket_subset_follow_the_bucket_table(head):
    cfg = cfgmod.tiny()
    N = cfg.num_hidden_layers
    offsets, buckets, total = engine.bucket_table(cfg, head)
    assert sorted(buckets) == list(range(N + 2))
    sizes = {k: hi - lo for k, (lo, hi) in buckets.items()}
    for s in (0, 1, 1 + (N - 1), N + 1):
        lo, hi = train.trainable_range(buckets, s)
        assert hi == total and lo == (buckets[s][0] if s else 0)
        assert hi - lo == sum(sizes[k] for k in buckets if k >= s)            # buckets are contiguous: ONE AdamW launch covers them
        assert lo % engine.BUCKET_ALIGN == 0
        # every parameter lies wholly inside or wholly outside the range, by its stage
        for n, (off, num) in offsets.items():
            assert (off >= lo) == (engine.bucket_of(n, N) >= s), (n, s)
            assert off + num <= lo or off >= lo
        sub = train.trainable_buckets(buckets, s)
        assert sorted(sub) == [k for k in sorted(buckets) if k >= s]
        sync = cdist.ShardedGradSync(sub, "cpu")
        assert sync.order == sorted(sub) and sync.shard_elems == hi - lo
        assert sum(b - a for a, b in sync.buckets.values()) * 4 == (hi - lo) * 4       # bytes on the wire per step (fp32)
    assert train.trainable_range(buckets, N + 1)[0] == buckets[N + 1][0] > buckets[N][0]


def test_optimizer_refuses_a_stage_change_after_a_step():
    m, cfg = _model("cpt")
    opt = train.FusedAdamW(m, lr=1e-3)
    train.freeze_layers(m, 1)
    assert opt._check_stage() == 2                 # not stepped yet: the optimizer follows
    train.freeze_embeddings(m)
    assert opt._check_stage() == 1
    opt.step_count = 1                             # (as after the first step(): the moments now belong to stage 1)
    opt._check_stage()
    train.freeze_layers(m, 1)
    with pytest.raises(RuntimeError, match="build a new optimizer"):
        opt.step()
    with pytest.raises(RuntimeError, match="build a new optimizer"):
        opt._check_stage()
    train.unfreeze(m)
    with pytest.raises(RuntimeError, match="build a new optimizer"):
        opt.step()
    train.freeze_embeddings(m)
    opt._check_stage()                             # back at the optimizer's stage: fine
    assert train.FusedAdamW(m, lr=1e-3)._check_stage() == 1


@pytest.mark.parametrize("head", HEADS)
def test_unfreeze_restores_everything(head):
    m, cfg = _model(head)
    train.train_head_only(m)
    assert not all(_flags(m).values())
    assert train.unfreeze(m) == 0
    assert train.trainable_stage(m) == 0 and m._engine().first_stage is None
    assert all(p.requires_grad for p in m.parameters())
    train.check_stage_flags(m)


def test_template_is_left_alone_and_joins_the_trainable_top():
    """A soft template lives outside the engine's parameters: setting a stage does not touch its flag, and with a stage >= 1 it is no
    longer 'a trainable template beside a trainable backbone'; with no stage set that still raises."""
    m, cfg = _model("cpt")
    w = soft_prompt.attach(m, n_slots=5, freeze_backbone=False)
    assert w.requires_grad
    with pytest.raises(NotImplementedError, match="trainable soft template"):
        soft_prompt.frozen_step(m)
    train.freeze_layers(m, 1)
    assert w.requires_grad
    train.check_stage_flags(m)
    train.unfreeze(m)
    assert w.requires_grad
    with pytest.raises(NotImplementedError, match="trainable soft template"):
        m(torch.zeros(2, 4, dtype=torch.long), masked_lm_labels=torch.tensor([5, 6]), mask_token_pos=torch.tensor([1, 2]))
