"""TEST INFRASTRUCTURE: the float64 reference and the bounds of calm_sam_perturb / calm_sam_restore (csrc/sam.hip), built on
tail_f64 as grad_stats_f64 is: the table, the state and the gradients are tail_f64's, the corrected gradient is
optim_reference(...)["gcorr"] and its element-wise error the expression optim_reference charges for it (formed again by
grad_stats_f64._e_gcorr, term for term).  The module knows nothing about who produced what it checks.

No measured tolerance.  From the arithmetic the header states (U = 2^-24, d = tail_f64.optim_sum_depth(numel), D =
ceil(n_tensors / 256) + 9: a running sum's serial adds, six shuffle levels, three adds of the wave sums), with rho, eps, eta
the fp32 values the ABI receives:

    g' = gcorr * inv         e_g = e_gc inv + |gcorr| e_inv + U |g'|           (e_inv = U inv with a scale: the reciprocal)
    t  = |w| + eta           e_t = U t                                         (adaptive only; one addition of exact inputs)
    s  = g'  |  t g'         e_s = e_g  |  t e_g + |g'| e_t + e_t e_g + U |s|
    per tensor sum s^2       sum (2 |s| e_s + e_s^2) + (d + 1) U sum s^2       the elements' errors, one rounding per square,
                                                                               the sum's depth
    total                    the tensors' bounds + D U total
    norm = sqrt(total)       min(e_total / norm, sqrt(e_total)) + U norm
    den = norm + eps         e_den = e_norm + U den
    scale = rho / den        e_scale = scale e_den / (den - e_den) + U (scale + that)
    plain step  scale s      e_step = scale e_s + |s| e_scale + e_scale e_s + U |step|
    adaptive    a = scale t  e_a = scale e_t + t e_scale + e_scale e_t + U a
                step = a s   e_step = a e_s + |s| e_a + e_a e_s + U |step|
    w' = w + step            e_w = e_step + U (|w'| + e_step)                  (an fma commits less)
    length ||w' - w||_2      | ||got - w|| - scale norm | <= ||e_w||_2         (triangle inequality over the table; the
                             reference length is rho norm / (norm + eps) = scale norm; non-adaptive only)

Exact, with no bound: the backup's bits (the parameters before the call), the parameters' bits after the restore (the same),
found_inf, and under a non-finite gradient scale == 0 with every parameter bit unchanged."""
import math

import torch

import tail_f64 as tf
from grad_stats_f64 import _e_gcorr
from tail_f64 import U, _Report


def reference(recs, grads, hp, grad_scale):
    """calm_sam_perturb in float64.  recs / grads as for tail_f64.optim_reference (the state BEFORE the call); hp = (rho,
    eps, eta, adaptive).  -> (ref, bound): ref holds norm, scale, found_inf, length (non-adaptive, else None), and w (the
    parameters before) and p_after as flat float64 concatenations; bound holds norm, scale, p_after, length."""
    rho, eps, eta = (tf.f32(v) for v in hp[:3])
    adaptive = bool(hp[3])
    inv = 1.0 / tf.f32(grad_scale) if grad_scale is not None else 1.0
    e_inv = U * inv if grad_scale is not None else 0.0
    w = torch.cat([r["param"].double().reshape(-1) for r in recs])
    finite = all(bool(torch.isfinite(g.double()).all()) for g in grads)
    ref = dict(w=w, found_inf=0.0 if finite else 1.0, length=None)
    if not finite:
        ref.update(norm=math.nan, scale=0.0, p_after=w)
        return ref, {}
    opt_hp = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 0)                          # (gcorr does not depend on them)
    gcorr = tf.optim_reference(recs, grads, opt_hp, grad_scale, 0)[0]["gcorr"]
    S, E_S, T, E_T, total, e_total = [], [], [], [], 0.0, 0.0
    for r, g, gc in zip(recs, grads, gcorr):
        G = g.double().reshape(-1)
        d = tf.optim_sum_depth(G.numel())
        x = gc * inv
        e_x = _e_gcorr(r, G) * inv + gc.abs() * e_inv + U * x.abs()
        if adaptive:
            t = r["param"].double().reshape(-1).abs() + eta
            e_t = U * t
            s = t * x
            e_s = t * e_x + x.abs() * e_t + e_t * e_x + U * s.abs()
        else:
            t, e_t, s, e_s = torch.ones_like(x), torch.zeros_like(x), x, e_x
        n2 = float((s * s).sum())
        total += n2
        e_total += float((2 * s.abs() * e_s + e_s * e_s).sum()) + (d + 1) * U * n2
        S.append(s), E_S.append(e_s), T.append(t), E_T.append(e_t)
    if not math.isfinite(total) or total > 3.402823466e38:   # (the fp32 sum overflows: no case sits near that border)
        ref.update(found_inf=1.0, norm=math.nan, scale=0.0, p_after=w)
        return ref, {}
    e_total += (tf.cdiv(len(recs), tf.OPT_NT) + 9) * U * total
    norm = math.sqrt(total)
    # |sqrt a - sqrt b| <= |a - b| / sqrt b and <= sqrt |a - b|
    e_norm = min(e_total / norm if norm > 0 else 0.0, math.sqrt(e_total)) + U * norm
    den = norm + eps
    e_den = e_norm + U * den
    scale = rho / den
    e_scale = scale * e_den / (den - e_den)
    e_scale += U * (scale + e_scale)
    s, e_s, t, e_t = torch.cat(S), torch.cat(E_S), torch.cat(T), torch.cat(E_T)
    if adaptive:
        a = scale * t
        e_a = scale * e_t + t * e_scale + e_scale * e_t + U * a
        step = a * s
        e_step = a * e_s + s.abs() * e_a + e_a * e_s + U * step.abs()
    else:
        step = scale * s
        e_step = scale * e_s + s.abs() * e_scale + e_scale * e_s + U * step.abs()
    p_after = w + step
    e_w = e_step + U * (p_after.abs() + e_step)
    ref.update(norm=norm, scale=scale, p_after=p_after)
    bound = dict(norm=e_norm, scale=e_scale, p_after=e_w)
    if not adaptive:
        ref["length"] = scale * norm
        bound["length"] = float(e_w.norm()) + 1e-12 * ref["length"]        # (the float64 evaluation itself)
    return ref, bound


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check(got, ref, bound, strict=True):
    """got: norm, found_inf, scale (floats) and backup, p_after, p_restored (flat fp32 concatenations over the tensors) of
    one perturb / restore pair from the state `ref` was made of.  -> (worst, failures)"""
    rep = _Report()
    w32 = ref["w"].float()
    if not _same_bits(got["backup"], w32):
        rep.fail("backup", f"{int((got['backup'].view(torch.int32) != w32.view(torch.int32)).sum())} elements are not the "
                           "parameters' bits before the call")
    if not _same_bits(got["p_restored"], w32):
        rep.fail("p_restored", f"{int((got['p_restored'].view(torch.int32) != w32.view(torch.int32)).sum())} elements are not "
                               "the parameters' bits before the call")
    if got["found_inf"] != ref["found_inf"]:
        rep.fail("found_inf", f"got {got['found_inf']}, expected {ref['found_inf']}")
    if ref["found_inf"]:
        if got["scale"] != 0.0:
            rep.fail("scale", f"scale {got['scale']!r} under a non-finite gradient, expected 0")
        if not _same_bits(got["p_after"], w32):
            rep.fail("p_after", "parameters changed under a non-finite gradient")
        return rep.done(strict)
    one = lambda x: torch.tensor([float(x)], dtype=torch.float64)              # noqa: E731
    rep.bounded("norm", one(got["norm"]), one(ref["norm"]), one(bound["norm"]))
    rep.bounded("scale", one(got["scale"]), one(ref["scale"]), one(bound["scale"]))
    rep.bounded("p_after", got["p_after"], ref["p_after"], bound["p_after"])
    if ref["length"] is not None:
        length = float((got["p_after"].double() - got["backup"].double()).norm())
        rep.bounded("length", one(length), one(ref["length"]), one(bound["length"]))
    return rep.done(strict)
