"""Shared comparator of the inference-forward tests (a plain module, imported by test files; not a conftest).

Every output of a forward ([MASK]-row logits, all-row logits, sequence output, pooled output, relation scores) is compared with the
float64 oracle (oracle.cpt_oracle) in two ways:

* whole tensor: rel = ||got - ref|| / ||ref||;
* row-wise: the same figure for every row of the output (the last dimension is a row: one per sequence for [B, ...] outputs, one per
  token for [B, L, H] and [B, L, V]); the WORST row is reported and bounded.  One wrong row among 8000 moves the whole-tensor figure by
  1 / sqrt(8000) of its own error and disappears in it; it cannot disappear in its own row.

Bounds
* fp32 / bf16x3: a fixed bound per mode, for the whole tensor and for the worst row (FIXED, FIXED_ROW).
* bf16: the yardstick is the oracle's bf16 design emulation (the same call under ``O.emulate_bf16()`` in float64):
  ``rel_kernel <= C_FWD * rel_emulation + FLOOR_FWD`` for the whole tensor, and the kernel's worst row against the emulation's worst row
  in the same form.  (Worst against worst, not row r against row r: the two rounding errors of one row are independent, so the
  emulation's error of a single row is small by chance somewhere among thousands of rows and a row-by-row ratio measures that chance.  A
  row that is wrong -- not rounded differently -- leaves the emulation's worst row behind by far more than C_FWD.)
* logits and relation scores also keep the absolute band the suite held them to before (ABS_BAND).
* A NaN or Inf anywhere in an output fails it, whatever the norms say.

No output and no row is ever left out: every name of the reference must be present in ``got`` (a missing one fails), a name the
reference does not have is an error, and the row-wise figure runs over all rows.

``check`` raises with a table: case, output, worst row index, rel, rel(emu), ratio and bound, for the whole tensor and the worst row.

How the constants were set: see MEASURED below.
"""
import math

import torch

# ---- measured constants (MEASURED below) ----------------------------------------------------------------------------------------------------------------
FIXED = {"fp32": 2.4e-6, "bf16x3": 2.0e-5}         # whole tensor: 2 x the worst measured (1.17e-6, 9.60e-6)
FIXED_ROW = {"fp32": 4.7e-6, "bf16x3": 2.7e-5}     # worst row: 2 x the worst measured (2.34e-6, 1.33e-5)
C_FWD = 2.25                                       # worst measured ratio 1.80 plus 25 %
FLOOR_FWD = 1e-3
MEASURED = """
Measured 2026-10-17 on one MI355X, product build, on top of commit ce4509e, over every (case, output) of tests/test_gpu_fwd_regimes.py
(135 outputs of 45 cases; Oscar-base width with 3 layers, Oscar-large width with 2).

fp32 / bf16x3, rel against the float64 oracle (worst over the sweep; the bounds are twice these):
  mode     whole tensor                 worst row                  max |d logit|
  fp32     1.17e-6 (fp32_b1 all_logits) 2.34e-6 (fp32_b64 rel)     4.5e-6
  bf16x3   9.60e-6 (x3_b4 rel)          1.33e-5 (x3_b4 rel)        2.7e-5
  Far inside what the suite allows these modes elsewhere (2e-4 / 5e-4 relative in tests/_gradcheck.py, 1e-3 absolute on Oscar-base logits).

bf16, ratio rel_kernel / rel_emulation, worst per regime (whole tensor | worst row, with the case and output that gave it):
  L = 70 + 50, 1..160 sequences (row-major, padded, rpanel, refused, multi-round)   1.33 b1 rel         | 1.33 b1 rel
  L = 128 at 65 sequences                                                           1.01 seq            | 1.02 pooled
  L = 129 (two-kernel form, ctx panel)                                              1.01 L129_b128 seq  | 1.05 L129_b128 seq
  L = 210 (QKV / FFN-up kernel walk, ctx panel at 64)                               1.01 L210_b64 mask  | 1.11 L210_b63 rel
  L = 288 | 289                                                                     1.13 L289_b3 rel    | 1.16 L289_b3 rel
  Li > Lt, text only                                                                1.04 text_b4 rel    | 1.01 Li_gt_Lt_b5 seq
  3-D mask                                                                          1.65 mask3_b4 rel   | 1.80 mask3_b4 rel
  Oscar-large width                                                                 1.03 large_b52 rel  | 1.02 large_b52 mask
  fold off                                                                          1.31 nofold_b4 rel  | 1.13 nofold_b4 rel
  By output: [MASK]-row logits <= 1.08, all-row logits <= 1.00, sequence output <= 1.05, pooled <= 1.05 in every regime: the folded
  LayerNorm, the 3-byte residual stream, the panel layouts, the padded rows and the tail leave the error where the emulation puts it.
  Every ratio above 1.1 belongs to the relation scores of a batch of 1 to 4 sequences: 3 to 12 numbers, whose two independent rounding
  errors have a noisy quotient (the same output at 33..68 sequences: 0.9..1.1).  No regime stands above the others; the worst figure,
  1.80, sets C_FWD = 2.25.
  rel(emu) itself: 2.2e-3 (sequence output) .. 4.5e-3 (logits) for the whole tensor, never small by chance in this sweep, so no case
  needs the floor.  FLOOR_FWD = 1e-3 is kept for the outputs of a few numbers (relation scores of one sequence), whose emulation error CAN
  come out several times below its usual 3e-3: it is the size of one bf16 rounding (2^-9 / sqrt 3 = 1.1e-3) that one side may have
  and the other not, and a quarter of the smallest bound it is added to.
  max |d logit| in bf16: 1.42e-2 (band 0.04).  Wall time per case: forward <= 0.03 s, float64 oracle and emulation <= 0.52 s.

The emulation models the pooler and the relation head as GEMMs on bf16 operands (oracle.cpt_oracle: _linear / relation_head), which is
what the bf16 kernels run.  Before this sweep the oracle left those two wide under emulate_bf16(); the first measurement showed it as a
pooled ratio of 1.4..1.5 and a relation-score ratio of 1.4..3.5 in EVERY regime, the unfolded encoder included, and nowhere else.
"""
ABS_BAND = {"bf16": 0.04, "fp32": 1e-3, "bf16x3": 1e-3}      # max |difference| of logits and relation scores (tests/test_gpu_fullsize.py, tests/test_gpu_vg.py)
ABS_OUTPUTS = ("mask_logits", "all_logits", "rel")


def rel(got, ref):
    got = got.detach().double().flatten()
    ref = ref.detach().double().flatten().to(got.device)
    return float((got - ref).norm() / (ref.norm() + 1e-300))


def row_rels(got, ref):
    """rel of every row (last dimension) -> 1-D float64 tensor, one entry per row, none left out."""
    got = got.detach().double()
    ref = ref.detach().double().to(got.device)
    if got.shape != ref.shape:
        raise ValueError("shape %s against the reference's %s" % (tuple(got.shape), tuple(ref.shape)))
    g = got.reshape(-1, got.shape[-1])
    r = ref.reshape(-1, ref.shape[-1])
    return (g - r).norm(dim=1) / (r.norm(dim=1) + 1e-300)


def worst_row(got, ref):
    """(index, rel) of the worst row; a row that holds a NaN or an Inf is the worst there is."""
    rr = row_rels(got, ref)
    bad = ~torch.isfinite(rr)
    if bool(bad.any()):
        return int(bad.nonzero()[0]), float("inf")
    i = int(rr.argmax())
    return i, float(rr[i])


def bound(mode, rel_emu, row=False):
    if mode in FIXED:
        return (FIXED_ROW if row else FIXED)[mode]
    return C_FWD * rel_emu + FLOOR_FWD


def compare(mode, got, ref, emu=None):
    """got / ref / emu: {output name: tensor}; ref is the float64 oracle, emu its bf16 emulation (bf16 mode only).
    -> one dict per output of the reference: name, n_rows, rel, emu, bound, row (index of the worst row), row_rel, row_emu, row_bound,
    absmax, abs_band, ok."""
    if mode not in FIXED and emu is None:
        raise ValueError("bf16 needs the emulation's outputs")
    extra = sorted(set(got) - set(ref))
    if extra:
        raise ValueError("outputs without a reference: %s" % extra)
    rows = []
    for name, r in ref.items():
        g = got.get(name)
        row = dict(name=name, n_rows=int(r.numel() // r.shape[-1]), emu=float("nan"), row_emu=float("nan"), row=-1, absmax=float("nan"),
                   abs_band=ABS_BAND[mode] if name in ABS_OUTPUTS else float("inf"))
        if g is None or tuple(g.shape) != tuple(r.shape):
            row.update(rel=float("inf"), row_rel=float("inf"), bound=0.0, row_bound=0.0, ok=False)
            rows.append(row)
            continue
        if emu is not None:
            row["emu"] = rel(emu[name], r)
            row["row_emu"] = worst_row(emu[name], r)[1]
        rk = rel(g, r)
        if not math.isfinite(rk):
            rk = float("inf")
        i, rw = worst_row(g, r)
        am = float((g.detach().double() - r.detach().double().to(g.device)).abs().max())
        b, bw = bound(mode, row["emu"]), bound(mode, row["row_emu"], row=True)
        row.update(rel=rk, row=i, row_rel=rw, bound=b, row_bound=bw, absmax=am,
                   ok=bool(rk <= b and rw <= bw and am <= row["abs_band"]))
        rows.append(row)
    return rows


def ratio(r, row=False):
    """Kernel error over emulation error (nan without an emulation)."""
    k, e = (r["row_rel"], r["row_emu"]) if row else (r["rel"], r["emu"])
    return k / e if e == e and e > 0 else float("nan")


def table(rows, what=""):
    out = ["%-34s %-12s %8s %10s %10s %7s %10s %10s" % ("case", "output", "row", "rel", "rel(emu)", "ratio", "bound", "max|diff|")]
    for r in rows:
        ok_w = r["rel"] <= r["bound"]
        ok_r = r["row_rel"] <= r["row_bound"]
        ok_a = r["absmax"] <= r["abs_band"]
        out.append("%-34s %-12s %8s %10.3e %10.3e %7.2f %10.3e %10.3e%s" % (what[-34:], r["name"], "whole", r["rel"], r["emu"], ratio(r), r["bound"],
                                                                             r["absmax"], "" if ok_w and ok_a else "  FAIL"))
        out.append("%-34s %-12s %8d %10.3e %10.3e %7.2f %10.3e %10s%s" % (what[-34:], r["name"], r["row"], r["row_rel"], r["row_emu"], ratio(r, True),
                                                                           r["row_bound"], "of %d" % r["n_rows"], "" if ok_r else "  FAIL"))
    return "\n".join(out)


def check(mode, got, ref, emu=None, what=""):
    """compare(), raising with the table if any output is outside a bound (whole tensor, worst row or absolute band)."""
    rows = compare(mode, got, ref, emu)
    bad = [r for r in rows if not r["ok"]]
    if bad:
        raise AssertionError("%s: %d of %d outputs outside their bounds (mode %s, C_FWD = %g, FLOOR_FWD = %g)\n%s"
                             % (what, len(bad), len(rows), mode, C_FWD, FLOOR_FWD, table(rows, what)))
    return rows
