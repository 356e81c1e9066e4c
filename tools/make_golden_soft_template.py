"""Golden vector of soft-template prompt tuning from the reference's own code (Oscar/oscar/explore/sgd_to_explore_template.py:26-66
TemplateEmbedding on Oscar/oscar/modeling/modeling_rec.py REC_MLM_CPT).

Runs on a CPU box with the reference checked out (default /root/reference, or $CPT_REFERENCE), importing its modules through
oracle/ref_stub.py.  The explore script itself cannot be imported (it imports a dataset module the reference does not ship, and
IPython), so ONLY the ``TemplateEmbedding`` class definition is taken out of that file AT RUN TIME (ast) and executed; nothing of the
reference is copied into this repository.  The class is installed on the reference's REC_MLM_CPT built from the tiny checkpoint
tests/golden/tiny_ckpt, its template moved off the word rows by a seeded offset (stored), and one eval-mode step is recorded:

    tests/golden/soft_template_tiny.npz: in_* (the batch, slot ids planted: tests/_softcheck.py plant_slots), template, labels,
    scores ([MASK]-row prediction scores), loss, grad_template (autograd through torch.where)

    python tools/make_golden_soft_template.py     # rewrites the file identically
"""
import ast
import logging
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("CPT_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")

import ref_stub  # noqa: E402

ref_stub.install()
sys.path.insert(0, os.path.join(REF, "Oscar"))
from oscar.modeling.modeling_bert import BertImgForPreTraining  # noqa: E402
from oscar.modeling.modeling_rec import REC_MLM_CPT  # noqa: E402

from cpt_amd import synth  # noqa: E402
import _softcheck as S  # noqa: E402


def template_embedding_class():
    """The reference's TemplateEmbedding, compiled from its class definition alone."""
    path = os.path.join(REF, "Oscar", "oscar", "explore", "sgd_to_explore_template.py")
    tree = ast.parse(open(path).read(), path)
    node = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "TemplateEmbedding"]
    assert len(node) == 1, "TemplateEmbedding not found in %s" % path
    ns = {"torch": torch, "nn": torch.nn}
    exec(compile(ast.Module(body=node, type_ignores=[]), path, "exec"), ns)
    return ns["TemplateEmbedding"]


def main():
    logging.disable(logging.INFO)
    torch.manual_seed(0)
    ck = os.path.join(OUT, "tiny_ckpt")
    rc = ref_stub.BertConfig.from_pretrained(ck)
    pre = BertImgForPreTraining.from_pretrained(ck, config=rc)
    m = REC_MLM_CPT(rc)
    m.copy_from_pretraining_model(pre)
    m.eval()
    m.bert.embeddings = template_embedding_class()(m.bert.embeddings)
    tmpl = m.bert.embeddings.template_embeddings.weight
    assert tuple(tmpl.shape) == (S.N_SLOTS, rc.hidden_size)
    gen = torch.Generator().manual_seed(S.TEMPLATE_SEED)
    with torch.no_grad():       # off the word rows: an implementation that ignores the template must not pass
        tmpl.copy_(m.bert.embeddings.word_embeddings.weight[:S.N_SLOTS] + torch.randn(tmpl.shape, generator=gen) * 0.05)
    for p in m.parameters():
        p.requires_grad_(False)
    tmpl.requires_grad_(True)
    b = S.plant_slots(synth.make_batch(4, rc, seed=S.TINY_BATCH_SEED, max_seq_len=20, img_seq_len=6))
    B = b["input_ids"].size(0)
    lab = torch.full(b["attention_mask"].shape, -1, dtype=torch.long)
    lab[torch.arange(B), b["mask_token_pos"]] = b["colors"]
    loss, scores = m(b["input_ids"], b["segment_ids"], b["attention_mask"], masked_lm_labels=lab, img_feats=b["img_feats"])[:2]
    loss.backward()
    g = {"in_" + k: v.numpy() for k, v in b.items()}
    g.update(template=tmpl.detach().numpy(), labels=lab.numpy(), loss=loss.detach().numpy(),
             scores=scores.detach()[torch.arange(B), b["mask_token_pos"]].numpy(), grad_template=tmpl.grad.numpy(),
             keys=np.array(sorted(m.state_dict().keys())))
    path = os.path.join(OUT, "soft_template_tiny.npz")
    np.savez_compressed(path, **g)
    print("wrote", path, os.path.getsize(path), "bytes; |grad| max %.3e, used slots %s"
          % (float(tmpl.grad.abs().max()), sorted(int(i) for i in (tmpl.grad.abs().sum(1) > 0).nonzero().flatten())))


if __name__ == "__main__":
    main()
