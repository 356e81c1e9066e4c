"""Shared comparator of the training-step gradient tests (a plain module, imported by test files; not a conftest).

Every parameter gradient of a step is compared with the float64 oracle (oracle.cpt_oracle.train_step_grads) as
rel = ||got - ref|| / ||ref||, the whole tensor at once.

* fp32 / bf16x3: a fixed bound per mode, the tiny-config tests' 2e-4 / 5e-4 (two layers there, twelve layers, up to 6.4 k rows and
  dropout 0.1 here: the bounds are not raised).
* bf16: the yardstick is the bf16 design emulation of the oracle (``train_step_grads(..., bf16=True)``: bf16 operands and incoming
  gradients of every product, everything else wide).  Per parameter ``rel_kernel <= C * rel_emulation + FLOOR``, and never above the
  8e-2 band the norm-only test allowed (OLD_BAND).  C is one constant for every parameter, shape and layer: a launch that drops,
  repeats or misplaces part of a sum leaves the emulation's rounding error behind by far more than C.  C = 2.5: over the Oscar-base sweep
  (1..53 sequences, 12 layers) the worst gradient ratio is 2.0 (a LayerNorm gain at 6240 rows), most tensors sit at 1.0..1.3; the loss,
  whose emulation error is sometimes tiny by chance, is held by the floor.  Over the Oscar-large NSP-CPT / Q->AR sweep
  (tests/test_gpu_train_large.py: hidden 1024, 2 layers, 265..4240 rows) the worst gradient ratio is 1.5 (layer 1's query bias at 2120 rows).
* attention.self.key.bias: zero in exact arithmetic (softmax is shift-invariant), both sides hold rounding noise -> an absolute bound.

``check`` raises with a per-layer table (the worst parameter of layers 11 -> 0, then the embeddings and the head), so that error growth
with depth is visible at a glance.
"""
import re

FIXED = {"fp32": 2e-4, "bf16x3": 5e-4}
C = 2.5
FLOOR = 2e-3
OLD_BAND = 8e-2
KEY_BIAS_ABS = {"fp32": 1e-5, "bf16x3": 1e-5, "bf16": 1e-3}      # max |grad| of attention.self.key.bias (as tests/test_gpu_dropout.py)

_LAYER = re.compile(r"^bert\.encoder\.layer\.(\d+)\.")


def rel(got, ref):
    got = got.detach().double().flatten()
    ref = ref.detach().double().flatten().to(got.device)
    return float((got - ref).norm() / (ref.norm() + 1e-300))


def group(name):
    """'layer N', 'embeddings' (text and region embeddings, their LayerNorms) or 'head' (transform, decoder bias, the pooler and the
    relation heads, loss, scores)."""
    m = _LAYER.match(name)
    if m:
        return "layer %d" % int(m.group(1))
    if name.startswith("bert.") and not name.startswith("bert.pooler."):
        return "embeddings"
    return "head"


def param_class(name):
    if name in ("loss", "scores"):
        return name
    if "LayerNorm" in name:
        return "layernorm"
    if name.endswith("bias"):
        return "bias"
    if "embeddings." in name:
        return "table"
    return "matrix"


def is_key_bias(name):
    return name.endswith("attention.self.key.bias")


def bound(mode, rel_emu):
    if mode in FIXED:
        return FIXED[mode]
    return min(C * rel_emu + FLOOR, OLD_BAND)


def compare(mode, got, ref, emu=None):
    """got / ref / emu: {name: tensor}; ref is the float64 oracle, emu its bf16 emulation (bf16 mode only).  Names whose reference is
    None (outside the loss's graph) are skipped.  -> one dict per tensor: name, group, cls, rel, emu, bound, ok."""
    if mode not in FIXED and emu is None:
        raise ValueError("bf16 needs the emulation's gradients")
    rows = []
    for name, r in ref.items():
        if r is None:
            continue
        g = got.get(name)
        row = dict(name=name, group=group(name), cls=param_class(name), emu=float("nan"))
        if g is None:
            row.update(rel=float("inf"), bound=0.0, ok=False)
        elif is_key_bias(name):
            mx = float(g.detach().abs().max())
            row.update(cls="key bias", rel=mx, bound=KEY_BIAS_ABS[mode], ok=mx < KEY_BIAS_ABS[mode] and float(r.abs().max()) < 1e-6)
        else:
            rk = rel(g, r)
            if emu is not None:
                row["emu"] = rel(emu[name], r)
            b = bound(mode, row["emu"])
            row.update(rel=rk, bound=b, ok=rk <= b)
        rows.append(row)
    return rows


def ratio(r):
    """Kernel error over emulation error (nan without an emulation)."""
    return r["rel"] / r["emu"] if r["emu"] == r["emu"] and r["emu"] > 0 else float("nan")


def _groups_in_order(rows):
    layers = sorted({int(r["group"].split()[1]) for r in rows if r["group"].startswith("layer ")}, reverse=True)
    return ["layer %d" % i for i in layers] + ["embeddings", "head"]


def table(rows):
    """Worst tensor (by rel / bound) of each layer from the last to the first, then the embeddings and the head."""
    out = ["%-11s %-52s %10s %10s %7s %10s" % ("group", "worst tensor", "rel", "rel(emu)", "ratio", "bound")]
    for gname in _groups_in_order(rows):
        mine = [r for r in rows if r["group"] == gname and r["cls"] != "key bias"]
        if not mine:
            continue
        w = max(mine, key=lambda r: r["rel"] / r["bound"] if r["bound"] > 0 else float("inf"))
        out.append("%-11s %-52s %10.3e %10.3e %7.2f %10.3e%s" % (gname, w["name"][-52:], w["rel"], w["emu"], ratio(w), w["bound"],
                                                              "" if w["ok"] else "  FAIL"))
    return "\n".join(out)


def summary(rows):
    """Worst kernel-to-emulation ratio (bf16; rel where there is no emulation) by group and by tensor class."""
    s = {}
    for r in rows:
        if r["cls"] == "key bias":
            continue
        v = ratio(r)
        v = r["rel"] if v != v else v
        for k in (r["group"], r["cls"]):
            s[k] = max(s.get(k, 0.0), v)
    return s


def check(mode, got, ref, emu=None, what=""):
    """compare(), raising with the per-layer table and the failing tensors if any tensor is outside its bound."""
    rows = compare(mode, got, ref, emu)
    bad = [r for r in rows if not r["ok"]]
    if bad:
        lines = ["%s: %d of %d tensors outside their bound (mode %s, C = %g, floor = %g)" % (what, len(bad), len(rows), mode, C, FLOOR),
                 table(rows), "failing:"]
        lines += ["  %-60s rel %.3e  rel(emu) %.3e  bound %.3e" % (r["name"], r["rel"], r["emu"], r["bound"]) for r in bad[:40]]
        raise AssertionError("\n".join(lines))
    return rows
