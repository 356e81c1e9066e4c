"""Soft-template prompt tuning: a trainable prompt in front of a frozen model.

Counterpart of the reference's template exploration, /root/reference/Oscar/oscar/explore/sgd_to_explore_template.py:
``TemplateEmbedding`` (:26-66) keeps an ``nn.Embedding(21, H)`` whose rows replace the word-embedding rows of the ids 1..20
(``[unused0]`` .. ``[unused19]``) wherever a sequence uses them, and its loop (:389-426) hands only that table to the optimizer.

Here the table is ``model.bert.embeddings.template_embeddings`` -- the state-dict key ``bert.embeddings.template_embeddings.weight``
the reference's module produces -- and it lives OUTSIDE the engine's flat parameter buffer and bucket table, which do not change.
With a template attached every forward of the model passes it to the library (include/cpt_hip.h cpt_soft_template: the embedding
launch reads ``tmpl[id]`` for 0 < id < n_slots), and a training forward of ``REC_MLM_CPT`` whose only parameter that requires grad is
the template takes the frozen step: cpt_train_fwd_soft / cpt_train_bwd_soft, the data-gradient chain alone, no weight gradient,
no 447 MB gradient buffer, no optimizer state for the model.  ``loss.backward()`` leaves ``template_embeddings.weight.grad`` as a
(n_slots, H) fp32 tensor (added to an existing one, as autograd accumulates); any torch optimizer over that one tensor works.

With a trainable stage set (``train.freeze_layers`` ..: the embedding side and the lower layers frozen, the top layers and the head
trainable) a trainable template is accepted as well: attach it with ``freeze_backbone=False``, set the stage; the backward trains the top
stages and goes on below the boundary as the frozen step, ending in the template's gradient (include/cpt_hip.h cpt_train_bwd_from).

Limits: the MLM head only (``REC_MLM_CPT``; one [MASK] row per sequence or a label grid); a trainable template beside a backbone that
trains from the embeddings up (no stage set), and the NSP-CPT heads in training, raise NotImplementedError.
"""
import torch
from torch import nn

KEY = "bert.embeddings.template_embeddings.weight"


def _embeddings(model):
    bert = getattr(model, "bert", model)
    emb = getattr(bert, "embeddings", None)
    if emb is None or not hasattr(emb, "word_embeddings"):
        raise TypeError("cpt_amd: %s holds no BertEmbeddings to attach a template to" % type(model).__name__)
    return emb


def template_of(model):
    """The attached template's weight (n_slots, H), or None."""
    bert = getattr(model, "bert", model)
    emb = getattr(bert, "embeddings", None)
    t = getattr(emb, "template_embeddings", None) if emb is not None else None
    return t.weight if t is not None else None


def attach(model, n_slots=21, freeze_backbone=True):
    """Adds ``model.bert.embeddings.template_embeddings = nn.Embedding(n_slots, H)`` with rows 1: copied from
    ``word_embeddings.weight[1:n_slots]`` (sgd_to_explore_template.py:32); row 0 belongs to the padding id and is never read.
    A model that already carries a template of this size keeps it (a loaded checkpoint).  ``freeze_backbone``: every other
    parameter gets ``requires_grad_(False)``.  Returns the template's weight."""
    emb = _embeddings(model)
    word = emb.word_embeddings.weight
    n_slots = int(n_slots)
    if n_slots < 2 or n_slots > word.size(0):
        raise ValueError("cpt_amd: n_slots must lie in [2, vocabulary size]")
    cur = getattr(emb, "template_embeddings", None)
    if cur is None or tuple(cur.weight.shape) != (n_slots, word.size(1)):
        t = nn.Embedding(n_slots, word.size(1))
        t.to(device=word.device, dtype=torch.float32)
        with torch.no_grad():
            t.weight[1:].copy_(word[1:n_slots])
        emb.template_embeddings = t
        cur = t
    if freeze_backbone:
        for p in model.parameters():
            if p is not cur.weight:
                p.requires_grad_(False)
        cur.weight.requires_grad_(True)
    return cur.weight


def detach(model):
    """Removes the template (the model takes the plain code paths again).  Does not unfreeze anything."""
    emb = _embeddings(model)
    if hasattr(emb, "template_embeddings"):
        del emb.template_embeddings


def attach_from_state_dict(model, state_dict):
    """from_pretrained: a checkpoint that carries the template key gets a template of that shape (filled by the loader); others load as before."""
    for k, v in state_dict.items():
        if k.endswith("embeddings.template_embeddings.weight"):
            attach(model, n_slots=v.shape[0], freeze_backbone=False)
            return True
    return False


def frozen_step(model):
    """True when a training forward of ``model`` takes the frozen step: a template is attached and it is the only parameter that
    requires grad.  A trainable template beside a trainable backbone raises NotImplementedError (train.mlm_loss_with_grad does not ask
    when a stage >= 1 is set: the template then trains under the trainable top stages); a template that does not require grad leaves
    training as it is without one (the forward still substitutes its rows)."""
    t = template_of(model)
    if t is None or not t.requires_grad:
        return False
    others = [n for n, p in model.named_parameters() if p.requires_grad and p is not t]
    if others:
        raise NotImplementedError("cpt_amd: a trainable soft template together with a trainable backbone (%d parameters, e.g. %s) is not "
                                  "implemented: freeze the model (soft_prompt.attach(model, freeze_backbone=True)) or freeze the template"
                                  % (len(others), others[0]))
    return True


def refuse_soft_training(model, who):
    """The NSP-CPT heads do not train a soft template (include/cpt_hip.h: the frozen step runs on the MLM head)."""
    t = template_of(model)
    if t is not None and t.requires_grad:
        raise NotImplementedError("cpt_amd: training a soft template through %s is not implemented: the frozen step runs on the MLM head "
                                  "(REC_MLM_CPT) only" % who)


def nearest_tokens(model, k=20):
    """Which real tokens the prompt rows have drifted towards (sgd_to_explore_template.py:419-425): the MLM head on the n_slots
    template rows, top-k per slot.  Returns (scores, ids), both (n_slots, k).  Plain torch: 21 rows, not a hot path."""
    t = template_of(model)
    if t is None:
        raise RuntimeError("cpt_amd: no soft template attached")
    cls = model.cls.predictions if hasattr(model.cls, "predictions") else model.cls
    with torch.no_grad():
        h = torch.nn.functional.linear(t.detach().float(), cls.transform.dense.weight, cls.transform.dense.bias)
        h = h * 0.5 * (1.0 + torch.erf(h / 2.0 ** 0.5))
        h = cls.transform.LayerNorm(h)
        scores = torch.nn.functional.linear(h, cls.decoder.weight) + cls.bias
        return scores.topk(int(k), dim=-1)
