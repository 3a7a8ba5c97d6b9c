"""The checker of the binary cross-entropy entry points (calm_bce_fwd / _bwd): a float64 reference written from the formulas
of include/calm_vit.h with torch.logaddexp in double, the inputs of every case, and the bounds.  Shared by
tests/test_bce_cpu.py (on the torch emulation of the entry points and on its planted faults) and tests/test_bce_gpu.py (on
the kernels).

Bounds:
  dlogits               helpers.rel_err <= 1e-4 — the project's fp32 kernel tolerance (TOL of tests/test_loss_gpu.py);
  loss, metrics[0]      |got - ref| <= 1e-4 * ref: for targets in [0, 1] the loss is a sum of non-negative terms, so a
                        relative bound is meaningful (metrics[0] = B * loss);
  metrics[1..3]         exact: the agreement count, B and 1."""
import math

import torch

from helpers import rel_err

TOL = 1e-4
SUM_CLASSES, THRESHOLD = 1, 2                  # CALM_BCE_SUM_CLASSES, CALM_BCE_THRESHOLD
# (B, C): one class; below a vector; vector plus tail; the vector path; every second row misaligned (the scalar path); more
# partials than threads in the final workgroup; a long row
CASES = [(1, 1), (3, 3), (3, 10), (4, 1000), (5, 1001), (257, 1000), (2, 21843)]
_SUBSET = [(3, 10), (4, 1000), (5, 1001)]
# seeds of the (3, 3) threshold variants at which the agreement count against the original targets differs from the count
# against the thresholded ones (found with reference() alone; tests/test_bce_cpu.py asserts it)
SEED_CUTMIX_02, SEED_SMOOTHED_00 = 0, 0
# (B, C, logit scale, kind, flags, threshold, dloss, seed) — every case at the defaults, then the variations on a subset
VARIANTS = ([(B, C, 1.0, "cutmix", 0, 0.0, 1.0, 0) for B, C in CASES] +
            [(B, C, 1.0, "cutmix", SUM_CLASSES, 0.0, 1.0, 0) for B, C in CASES] +
            # at 100 a naive log(1 + exp(z)) overflows in fp32
            [(B, C, s, "cutmix", 0, 0.0, 1.0, 0) for B, C in _SUBSET + [(2, 21843)] for s in (8.0, 30.0, 100.0)] +
            [(B, C, 1.0, kind, f, 0.0, 1.0, 0) for B, C in _SUBSET for kind in ("smoothed", "unnormalised")
             for f in (0, SUM_CLASSES)] +
            [(B, C, 1.0, "cutmix", THRESHOLD | f, 0.2, 1.0, 0) for B, C in _SUBSET + [(257, 1000)] for f in (0, SUM_CLASSES)] +
            [(B, C, 1.0, "smoothed", THRESHOLD, 0.0, 1.0, 0) for B, C in _SUBSET] +
            # the zeros of the CutMix targets EQUAL a threshold of 0: strict > leaves them 0
            [(B, C, 1.0, "cutmix", THRESHOLD, 0.0, 1.0, 0) for B, C in _SUBSET] +
            [(3, 3, 1.0, "cutmix", THRESHOLD, 0.2, 1.0, SEED_CUTMIX_02), (3, 3, 1.0, "smoothed", THRESHOLD, 0.0, 1.0, SEED_SMOOTHED_00)] +
            [(B, C, 1.0, "cutmix", f, 0.0, 3.0, 0) for B, C in _SUBSET + [(257, 1000), (2, 21843)] for f in (0, SUM_CLASSES)] +
            [(5, 1001, 8.0, "unnormalised", SUM_CLASSES | THRESHOLD, 0.5, 3.0, 0)])


def inputs(B, C, scale=1.0, kind="cutmix", seed=0):
    """Logits scale * randn and targets: 'cutmix' = two classes per row with weights lam, 1 - lam (the CutMix / MixUp
    labels, as ce_inputs of tests/test_loss_cpu.py), 'smoothed' = those mapped by y * 0.9 + 0.1 / C (label_smoothing=0.1),
    'unnormalised' = uniform(0, 1) in every class."""
    g = torch.Generator().manual_seed(seed + 7919 * B + C)
    z = torch.randn(B, C, generator=g) * scale
    if kind == "unnormalised":
        return z, torch.rand(B, C, generator=g)
    y = torch.zeros(B, C)
    lam = torch.rand(B, generator=g) * 0.8 + 0.1
    rows = torch.arange(B)
    y[rows, torch.randint(0, C, (B,), generator=g)] += lam
    y[rows, torch.randint(0, C, (B,), generator=g)] += 1.0 - lam
    if kind == "smoothed":
        return z, y * 0.9 + 0.1 / C
    if kind != "cutmix":
        raise ValueError(kind)
    return z, y


def _argmax_lowest(v):
    w = torch.where(torch.isnan(v), torch.full_like(v, -math.inf), v)
    return (w == w.max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)


def effective_targets(y, flags, threshold):
    """t of the header, in float64.  The ABI's threshold is a float: the comparison is made against its fp32 value."""
    if not flags & THRESHOLD:
        return y.double()
    return (y.double() > float(torch.tensor(threshold, dtype=torch.float32))).double()


def agreement(z, y):
    """#{b : argmax z == argmax y}, ties to the lowest index, a row holding a NaN in z or y counts as no agreement."""
    z, y = z.double(), y.double()
    bad = torch.isnan(z).any(dim=1) | torch.isnan(y).any(dim=1)
    return int(((_argmax_lowest(z) == _argmax_lowest(y)) & ~bad).sum())


def reference(z, y, flags=0, threshold=0.0, dloss=1.0):
    """Everything the entry points produce, in float64, from the formulas of include/calm_vit.h."""
    B, C = z.shape
    t = effective_targets(y, flags, threshold)
    z = z.double()
    terms = z.clamp_min(0.0) - z * t + torch.logaddexp(torch.zeros_like(z), -z.abs())
    denom = B if flags & SUM_CLASSES else B * C
    loss = terms.sum() / denom
    return {"loss": loss, "dlogits": dloss * (torch.sigmoid(z) - t) / denom, "agree": agreement(z, y),
            "metrics0": B * loss, "B": B}


def check(got, ref):
    """got: {"loss", "dlogits", "metrics"} — the loss, the gradient and the float[4] after ONE forward on a zeroed buffer.
    Returns the list of complaints (empty: everything is within its bound); figures(got, ref) has the numbers."""
    f = figures(got, ref)
    want = float(ref["loss"])
    out = []
    if not f["loss"] <= TOL * want:                                # (a NaN fails)
        out.append(f"loss {float(got['loss'])!r} against {want!r}: off by {f['loss']:.3e} > {TOL * want:.3e}")
    if not f["dlogits"] <= TOL:
        out.append(f"dlogits: rel_err {f['dlogits']:.3e} > {TOL:.0e}")
    if not f["metrics0"] <= TOL * float(ref["metrics0"]):
        out.append(f"metrics[0] {f['metrics'][0]!r} against B * loss = {float(ref['metrics0'])!r}")
    if f["metrics"][1:] != [float(ref["agree"]), float(ref["B"]), 1.0]:
        out.append(f"metrics[1:] {f['metrics'][1:]} against agreement {ref['agree']}, rows {ref['B']}, steps 1")
    return out


def figures(got, ref):
    m = [float(v) for v in torch.as_tensor(got["metrics"]).detach().double().cpu().reshape(-1)]
    return {"loss": abs(float(got["loss"]) - float(ref["loss"])), "dlogits": rel_err(got["dlogits"].detach(), ref["dlogits"]),
            "metrics0": abs(m[0] - float(ref["metrics0"])), "metrics": m}
