"""TEST INFRASTRUCTURE: the float64 reference and the bounds of calm_grad_stats (csrc/grad_stats.hip), built on tail_f64:
the table, the state and the gradients are tail_f64's, the corrected gradient is optim_reference(...)["gcorr"], and its
element-wise error is the expression optim_reference charges for it (e_gcorr is local there, so it is formed again here,
term for term).  The module knows nothing about who produced the records it checks.

No measured tolerance.  From the arithmetic the header states (U = 2^-24, d = tail_f64.optim_sum_depth(numel)):

    g' = gcorr * inv        e = e_gc inv + |gcorr| e_inv + U |g'|        (e_inv = U inv with a scale: the reciprocal)
    grad_sq                 sum (2 |g'| e + e^2)  +  (d + 1) U sum g'^2   the elements' own errors; one rounding per square
                                                                         and the sum's depth
    grad_absmax             max e                                        |max a - max b| <= max |a - b|
    param_sq                (d + 1) U sum p^2                            the inputs are exact
    param_absmax            0
    dir_sq                  sum (2 |d| e_d + e_d^2) + (d + 1) U sum d^2   e_d: the chain optim_reference charges for `upd`
                                                                         with 1 / bc1 in place of lr / bc1 and m, v exact
    nonfinite, bad_calls, first_bad_call, the summary: exact

A tensor whose RAW gradient holds an inf / NaN: a plain one sums its finite elements (the bound over those), a
spectral-norm one has a non-finite c and therefore grad_sq = grad_absmax = 0 exactly.
"""
import math

import numpy as np
import torch

import tail_f64 as tf
from tail_f64 import U, _Report

FLOAT_FIELDS = ("grad_sq", "grad_absmax", "param_sq", "param_absmax", "dir_sq")
INT_FIELDS = ("nonfinite", "bad_calls", "first_bad_call")


def _e_gcorr(r, G):
    """The error optim_reference charges for the corrected gradient of one tensor (its e_gcorr entry)."""
    if r["sn"] is None:
        return torch.zeros_like(G)
    d = tf.optim_sum_depth(G.numel())
    u, v, sigma, rows, cols = r["sn"]
    u, v, sg = u.double(), v.double(), float(sigma.double())
    G2, W = G.view(rows, cols), r["param"].double().view(rows, cols)
    uv = torch.outer(u, v)
    c = float((G2 * W).sum()) / sg
    e_c = (d + 3) * U * float((G2 * W).abs().sum()) / sg
    gc = ((G2 - c * uv) / sg).reshape(-1)
    return ((e_c * uv.abs() + 4 * U * (G2.abs() + abs(c) * uv.abs())) / sg).reshape(-1) + 2 * U * gc.abs()


def _sq_bound(x, e, d):
    return float((2 * x.abs() * e + e * e).sum() + (d + 1) * U * (x * x).sum())


def reference(recs, grads, hp, grad_scale, step):
    """calm_grad_stats in float64 from the fp32 values the ABI receives.  recs / grads / hp as for
    tail_f64.optim_reference (hp[1:4] = beta1, beta2, eps are read); step: plan.step_dev when the call runs.
    -> (ref, bound): float64 tensors [n_tensors] per float field, ref["nonfinite"] int64."""
    b1, b2, eps = (tf.f32(v) for v in hp[1:4])
    inv = 1.0 / tf.f32(grad_scale) if grad_scale is not None else 1.0
    e_inv = U * inv if grad_scale is not None else 0.0
    gcorr = tf.optim_reference(recs, grads, hp, grad_scale, step)[0]["gcorr"]
    t = int(step)
    if t >= 1:
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        r_bc1, r_bc2 = tf._pow_err(b1, t) / bc1, tf._pow_err(b2, t) / bc2
        r_inv = r_bc1 / (1 - r_bc1) + U                     # 1 / bc1
        isb2 = 1 / math.sqrt(bc2)
        r_isb2 = (1 - r_bc2) ** -0.5 - 1 + 2 * U
    ref = {k: [] for k in FLOAT_FIELDS + ("nonfinite",)}
    bound = {k: [] for k in FLOAT_FIELDS}
    for r, g, gc in zip(recs, grads, gcorr):
        G = g.double().reshape(-1)
        d = tf.optim_sum_depth(G.numel())
        raw_ok = torch.isfinite(G)
        ref["nonfinite"].append(int((~raw_ok).sum()))
        if r["sn"] is not None and not bool(raw_ok.all()):
            x, e = G[:0], G[:0]                             # c is not finite: every element is left out
        else:
            x = gc[raw_ok] * inv
            e = _e_gcorr(r, G)[raw_ok] * inv + gc[raw_ok].abs() * e_inv + U * x.abs()
        ref["grad_sq"].append(float((x * x).sum()))
        bound["grad_sq"].append(_sq_bound(x, e, d))
        ref["grad_absmax"].append(float(x.abs().max()) if x.numel() else 0.0)
        bound["grad_absmax"].append(float(e.max()) if x.numel() else 0.0)
        p = r["param"].double().reshape(-1)
        ref["param_sq"].append(float((p * p).sum()))
        bound["param_sq"].append((d + 1) * U * float((p * p).sum()))
        ref["param_absmax"].append(float(p.abs().max()))
        bound["param_absmax"].append(0.0)
        if t < 1:
            ref["dir_sq"].append(0.0)
            bound["dir_sq"].append(0.0)
            continue
        m, v = r["exp_avg"].double().reshape(-1), r["exp_avg_sq"].double().reshape(-1)
        sv = v.sqrt()
        e_sv = U * sv
        denom = sv * isb2 + eps
        e_den = e_sv * isb2 + sv * isb2 * (r_isb2 + U) + U * denom
        dd = (m / denom) / bc1
        e_d = (m.abs() * e_den / (denom * (denom - e_den).clamp_min(1e-300))) / bc1 + dd.abs() * (r_inv + 3 * U)
        ref["dir_sq"].append(float((dd * dd).sum()))
        bound["dir_sq"].append(_sq_bound(dd, e_d, d))
    ref = {k: torch.tensor(v, dtype=torch.int64 if k == "nonfinite" else torch.float64) for k, v in ref.items()}
    return ref, {k: torch.tensor(v, dtype=torch.float64) for k, v in bound.items()}


def norm_bound(ref, bound):
    """(norm, its bound) of sqrt(sum grad_sq) formed in float64 from fp32 per-tensor values inside their bounds."""
    total, e_total = float(ref["grad_sq"].sum()), float(bound["grad_sq"].sum()) + U * float(ref["grad_sq"].sum())
    root = math.sqrt(total)
    return root, min(e_total / root if root > 0 else 0.0, math.sqrt(e_total))


class Sticky:
    """What the sticky fields and the summary must hold after a sequence of calls (the host initialises: counts 0,
    firsts -1)."""

    def __init__(self, n):
        self.bad_calls = np.zeros(n, dtype=np.int64)
        self.first_bad_call = np.full(n, -1, dtype=np.int64)
        self.summary = [0, 0, -1, -1]

    def after(self, nonfinite):
        bad = np.asarray(nonfinite) > 0
        call = self.summary[0]
        self.bad_calls[bad] += 1
        self.first_bad_call[bad & (self.first_bad_call < 0)] = call
        self.summary[0] += 1
        if bad.any():
            self.summary[1] += 1
            if self.summary[2] < 0:
                self.summary[2], self.summary[3] = call, int(np.flatnonzero(bad)[0])
        return self


def check(got, summary, ref, bound, sticky, strict=True):
    """got: numpy record array of calm_grad_stat (one per tensor), summary: the four int32 — after a call whose reference is
    (ref, bound) and whose expected sticky state is `sticky` (already advanced by this call).  -> (worst, failures)"""
    rep = _Report()
    for k in FLOAT_FIELDS:
        rep.bounded(k, torch.from_numpy(np.asarray(got[k], dtype=np.float64)), ref[k], bound[k])
    want = dict(nonfinite=ref["nonfinite"].numpy(), bad_calls=sticky.bad_calls, first_bad_call=sticky.first_bad_call)
    for k in INT_FIELDS:
        g = np.asarray(got[k], dtype=np.int64)
        if not np.array_equal(g, want[k]):
            at = int(np.flatnonzero(g != want[k])[0])
            rep.fail(k, f"{int((g != want[k]).sum())} tensors differ, first {at}: got {int(g[at])}, expected {int(want[k][at])}")
    if [int(x) for x in summary] != list(sticky.summary):
        rep.fail("summary", f"got {[int(x) for x in summary]}, expected {list(sticky.summary)}")
    return rep.done(strict)
