"""Shared pieces of the soft-template tests (a plain module, imported by test files and tools/make_golden_soft_template.py; not a conftest).

* ``plant_slots``: puts slot ids (1 .. n_slots - 1) into a synthetic batch so that every case the gradient sum has to get right is
  there: a slot used twice in one sequence, a slot used in several sequences, a sequence with no slot at all, slots never used (their
  gradient rows must be exactly zero) and id 0 at an attended position.
* ``oracle_state`` / ``oracle_step``: the float64 oracle computes the same function when ``word_embeddings.weight`` has its rows
  1:n_slots replaced by the template and ``cls.decoder.weight`` is a separate tensor (the untouched table); the gradient of rows
  1:n_slots of that table is the template's gradient.  oracle/ is not edited.
"""
import torch

from oracle import cpt_oracle as O

N_SLOTS = 21
TEMPLATE_SEED = 9090
TINY_BATCH_SEED = 31
WORD = "bert.embeddings.word_embeddings.weight"
# per sequence (index % 4): (position, id) pairs
PATTERN = {0: ((1, 3), (2, 5), (3, 3)),                 # slot 3 twice in one sequence
           1: ((1, 3), (2, 7)),                         # slot 3 again: used in several sequences
           2: (),                                       # no slot at all
           3: ((1, 5), (2, N_SLOTS - 1), (3, 0))}       # the last slot; id 0 at an attended position
USED = (3, 5, 7, N_SLOTS - 1)


def plant_slots(batch, n_slots=N_SLOTS):
    """A copy of ``batch`` (synth.make_batch) with PATTERN written into input_ids; ids that fell into the slot range by chance are moved out."""
    ids = batch["input_ids"].clone()
    assert int(batch["mask_token_pos"].min()) > 3, "the planted positions 1..3 must lie in front of every [MASK]"
    stray = (ids > 0) & (ids < n_slots)
    ids[stray] += 200
    for i in range(ids.size(0)):
        for pos, tok in PATTERN[i % 4]:
            ids[i, pos] = tok
    return dict(batch, input_ids=ids)


def make_template(word, n_slots=N_SLOTS, seed=TEMPLATE_SEED, scale=0.05):
    """word rows + a seeded offset (CPU fp32): a template that an implementation ignoring it cannot match."""
    gen = torch.Generator().manual_seed(seed)
    w = word[:n_slots].detach().float().cpu()
    return w + torch.randn(w.shape, generator=gen) * scale


def oracle_state(sd, template):
    """sd: REC_MLM_CPT state dict (any device / dtype) -> the oracle's view of the model with the template attached."""
    T = template.size(0)
    word = sd[WORD]
    out = dict(sd)
    out["cls.decoder.weight"] = word.detach().clone()          # the decoder keeps the untouched table, as a tensor of its own
    w2 = word.detach().clone()
    w2[1:T] = template[1:T].to(device=word.device, dtype=word.dtype)
    out[WORD] = w2
    return out


def oracle_step(sd, cfg_dict, batch, template, drop=None, labels=None, bf16=False):
    """(loss, template gradient (n_slots, H) with row 0 zero, head-row scores) of the oracle construction."""
    T = template.size(0)
    loss, grads, scores = O.train_step_grads(oracle_state(sd, template), cfg_dict, batch, drop=drop, labels=labels, bf16=bf16, with_scores=True)
    g = grads[WORD][:T].detach().clone()
    g[0] = 0
    return loss, g, scores
