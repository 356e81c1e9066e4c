"""NSPCPT: the VCR colour-prompt scoring wrapper (pooled [CLS] -> pre-trained seq_relationship head), on the
HIP library.

Drop-in for /root/reference/Oscar/oscar/modeling/modeling_vcr.py:79-129: same
constructor, ``copy_from_pretraining_model`` (``self.cls`` BECOMES the pre-training model's
``cls.seq_relationship`` Linear, so the saved state dict is ``bert.*`` + ``cls.{weight,bias}``), forward argument
order and outputs ``(loss?, seq_relationship_score)``.  The encoder is the same HIP path as REC_MLM_CPT; the head
is the C ABI's CPT_OUT_REL output (pooler GEMM + tanh, then Linear(H, num_contrast_classes)).

Fine-tuning (fewshot/vcr_nsp_cpt.py:425-470) runs through the same HIP training step as REC_MLM_CPT with the NSP head
(pooler + tanh + Linear(H, 3) + cross entropy) in place of the MLM head: cpt_train_fwd / cpt_train_bwd select it when the
model carries w_pool / w_rel and no MLM head.
"""
import copy

import torch
from torch import nn

from . import _lib as L
from . import ops
from .modeling_bert import BertImgModel, BertLMPredictionHead, _EngineMixin, _check_unsupported
from .modeling_utils import BertPreTrainedModel


from .soft_prompt import refuse_soft_training

class NSPCPT(_EngineMixin, BertPreTrainedModel):
    _head = "nsp"

    def __init__(self, config):
        super().__init__(config)
        self.bert = BertImgModel(config)
        self.cls = BertLMPredictionHead(config)          # as the reference: replaced by copy_from_pretraining_model
        self.num_seq_relations = config.num_contrast_classes if hasattr(config, "num_contrast_classes") else 2
        self.apply(self.init_weights)
        self.tie_weights()

    def copy_from_pretraining_model(self, model, possible_colors=[]):
        """modeling_vcr.py:90-92."""
        self.bert = model.bert
        self.cls = model.cls.seq_relationship
        self.__dict__.pop("_cpt_engine", None)
        if "_cpt_engine" in model.__dict__:
            self._engine().dtype = model.__dict__["_cpt_engine"].dtype

    def tie_weights(self):
        """modeling_vcr.py:108-113 (a no-op once ``cls`` is the relation head)."""
        if hasattr(self.cls, "decoder"):
            self._tie_or_clone_weights(self.cls.decoder, self.bert.embeddings.word_embeddings)

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, next_sentence_label=None,
                position_ids=None, head_mask=None, img_feats=None):
        _check_unsupported(self.config, head_mask, None)
        if not isinstance(self.cls, nn.Linear):
            raise RuntimeError("cpt_amd: NSPCPT needs copy_from_pretraining_model() first (cls must be the "
                               "seq_relationship Linear, modeling_vcr.py:90-92)")
        if torch.is_grad_enabled() and next_sentence_label is not None:
            refuse_soft_training(self, "NSPCPT")
        if torch.is_grad_enabled() and next_sentence_label is not None and self.cls.weight.requires_grad:
            # few-shot fine-tuning (fewshot/vcr_nsp_cpt.py:425-470): loss with gradients through the HIP backward
            from .train import mlm_loss_with_grad
            return mlm_loss_with_grad(self, input_ids, token_type_ids, attention_mask, next_sentence_label.view(-1),
                                      position_ids, img_feats, None)
        out = self._engine().forward(input_ids, token_type_ids, attention_mask, position_ids, img_feats, flags=L.OUT_REL, trim=self.trim_padding)
        rel = out["rel"]
        outputs = (rel,)
        if next_sentence_label is not None:
            # CrossEntropyLoss(ignore_index=-1) over (B, num_seq_relations), modeling_vcr.py:124-127
            acc = ops.ce_rows(rel.view(-1, self.num_seq_relations).contiguous(),
                              next_sentence_label.view(-1).to(torch.int64).contiguous())
            outputs = (acc[0] / acc[1],) + outputs
        return outputs


class VCRQAR_NSPCPT(_EngineMixin, BertPreTrainedModel):
    """VCR Q->AR (Oscar/oscar/modeling/modeling_vcr.py:194-251; driver fewshot/vcr_qar_nsp_cpt.py): two relation heads on the pooled [CLS],
    ``cls_ans`` for the Q->A sequences and ``cls_rat`` for the QA->R sequences.

    Drop-in surface, as the reference: same constructor; ``copy_from_pretraining_model`` makes ``cls_ans`` the pre-training model's
    ``cls.seq_relationship`` and ``cls_rat`` an independent copy of it (copy.deepcopy, :206-209); the state dict is ``bert.*``,
    ``cls_ans.{weight,bias}``, ``cls_rat.{weight,bias}``; ``forward(..., head="ans" | "rat")`` returns ``(loss?, seq_relationship_score)`` with
    ``CrossEntropyLoss(ignore_index=-1)`` over (B, num_seq_relations); any other ``head`` gives the scores ``None`` (as the reference; a label then
    raises, where the reference's loss fails on ``None.view``).  The reference's ``tie_weights`` names a ``self.cls`` the model does not have
    and is never called; here it is a no-op.

    One-pass route: ``qar_forward`` runs the Q->A and the QA->R block through ONE encoder pass (rows [0, B0) -> cls_ans, [B0, B) -> cls_rat, the
    HIP head kernel cpt_rel2_scores / cpt_train_fwd_rel2).  ``forward(head=...)`` runs the same kernel with B0 = B or B0 = 0, so the two routes give
    the same per-sequence scores (the encoder is batch-invariant).  Training: the reference's ``loss = q_a_loss + qa_r_loss`` after two forwards
    cannot work on this engine -- a backward consumes only its own forward's activations, and the second training forward before a backward makes
    the first one's backward raise -- so the step is ``loss = qar_forward(..., q_a_labels, qa_r_labels)[0]; loss.backward()``."""
    _head = "qar"

    def __init__(self, config):
        super().__init__(config)
        self.bert = BertImgModel(config)
        self.cls_ans = None
        self.cls_rat = None
        self.num_seq_relations = config.num_contrast_classes if hasattr(config, "num_contrast_classes") else 2
        self.apply(self.init_weights)

    def copy_from_pretraining_model(self, model, possible_colors=[]):
        """modeling_vcr.py:206-209: cls_ans IS the pre-training model's seq_relationship Linear, cls_rat a deep copy."""
        self.bert = model.bert
        self.cls_ans = model.cls.seq_relationship
        self.cls_rat = copy.deepcopy(model.cls.seq_relationship)
        self.__dict__.pop("_cpt_engine", None)
        if "_cpt_engine" in model.__dict__:
            self._engine().dtype = model.__dict__["_cpt_engine"].dtype

    def tie_weights(self):
        """The reference's refers to a missing ``self.cls`` and is never called (modeling_vcr.py:226-231): nothing to tie."""

    def _heads_ready(self):
        if not (isinstance(self.cls_ans, nn.Linear) and isinstance(self.cls_rat, nn.Linear)):
            raise RuntimeError("cpt_amd: VCRQAR_NSPCPT needs copy_from_pretraining_model() first (cls_ans / cls_rat are the "
                               "seq_relationship Linears, modeling_vcr.py:206-209)")

    def _training(self, labels):
        if torch.is_grad_enabled() and labels is not None:
            refuse_soft_training(self, "VCRQAR_NSPCPT")
        return torch.is_grad_enabled() and labels is not None and (self.cls_ans.weight.requires_grad or self.cls_rat.weight.requires_grad)

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, next_sentence_label=None,
                position_ids=None, head_mask=None, img_feats=None, head=""):
        _check_unsupported(self.config, head_mask, None)
        self._heads_ready()
        if head not in ("ans", "rat"):
            # modeling_vcr.py:240-245: neither head runs; the reference still runs the encoder, whose result it drops
            if next_sentence_label is not None:
                raise RuntimeError("cpt_amd: VCRQAR_NSPCPT.forward with a label needs head='ans' or 'rat' (the reference fails on None.view)")
            return (None,)
        B = input_ids.size(0)
        B0 = B if head == "ans" else 0
        if self._training(next_sentence_label):
            from .train import mlm_loss_with_grad
            lab = next_sentence_label.view(-1)
            return mlm_loss_with_grad(self, input_ids, token_type_ids, attention_mask, lab.to(input_ids.device), position_ids, img_feats, None,
                                      rel2=(B0, _host_labels(lab)))
        out = self._engine().forward_rel2(input_ids, token_type_ids, attention_mask, position_ids, img_feats, B0=B0,
                                          labels=None if next_sentence_label is None else next_sentence_label.view(-1),
                                          labels_host=None if next_sentence_label is None else _host_labels(next_sentence_label.view(-1)),
                                          trim=self.trim_padding)
        outputs = (out["rel"],)
        if next_sentence_label is not None:
            outputs = (out["loss"],) + outputs
        return outputs

    def qar_forward(self, q_a_batch, qa_r_batch, q_a_labels=None, qa_r_labels=None, return_scores=False):
        """One encoder pass over the Q->A block and the QA->R block.  Each batch is a dict with ``input_ids``, ``attention_mask``,
        ``token_type_ids`` (or ``segment_ids``) and ``img_feats`` (optional), the layout of the reference's inputs dicts (vcr_qar_nsp_cpt.py:475-494).
        Returns (loss?, q_a_rel, qa_r_rel): loss = mean CE over the Q->A rows + mean CE over the QA->R rows (the driver's q_a_loss + qa_r_loss,
        :496) when both label vectors are given; under autograd it backpropagates through the HIP training step.  return_scores=True (inference
        only) appends the (B,) choice scores 1 - softmax(rel)[:, 1] of all rows (evaluate(), :641,650)."""
        self._heads_ready()
        if (q_a_labels is None) != (qa_r_labels is None):
            raise ValueError("qar_forward: give both label vectors or neither")

        def seg(b):
            return b.get("token_type_ids", b.get("segment_ids"))

        def cat(k, getter=None):
            a = getter(q_a_batch) if getter else q_a_batch.get(k)
            r = getter(qa_r_batch) if getter else qa_r_batch.get(k)
            if (a is None) != (r is None):
                raise ValueError("qar_forward: %s is given for one block only" % k)
            return None if a is None else torch.cat([a, r], 0)
        ids = cat("input_ids")
        B0 = q_a_batch["input_ids"].size(0)
        tt, mask, feats = cat("token_type_ids", seg), cat("attention_mask"), cat("img_feats")
        labels = None
        if q_a_labels is not None:
            labels = torch.cat([q_a_labels.view(-1).to(torch.int64), qa_r_labels.view(-1).to(torch.int64).to(q_a_labels.device)], 0)
        labels_host = None if labels is None else _host_labels(labels)
        if labels is not None:
            labels = labels.to(ids.device)
        if self._training(labels):
            if return_scores:
                raise ValueError("qar_forward: return_scores is for inference")
            from .train import mlm_loss_with_grad
            loss, rel = mlm_loss_with_grad(self, ids, tt, mask, labels, None, feats, None, rel2=(B0, labels_host))
            return loss, rel[:B0], rel[B0:]
        out = self._engine().forward_rel2(ids, tt, mask, None, feats, B0=B0, labels=labels, labels_host=labels_host, trim=self.trim_padding)
        rel = out["rel"]
        res = (rel[:B0], rel[B0:])
        if labels is not None:
            res = (out["loss"],) + res
        if return_scores:
            res = res + (out["score"],)
        return res


def _host_labels(labels):
    """Host int64 copy of a label vector for the library's range check: free for CPU tensors (the drivers build labels on the host); a
    device tensor is left to the library, which reads it back once."""
    if labels.device.type == "cpu":
        return labels.to(torch.int64).contiguous().numpy()
    return None
