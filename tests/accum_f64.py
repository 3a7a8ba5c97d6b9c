"""TEST INFRASTRUCTURE: float64 reference, element-wise bound and fp32 emulation of calm_grad_accum (include/calm_vit.h,
csrc/accum.hip) on the optimizer-step case table of tail_f64.py.  The reference is computed in float64 from the fp32
values the ABI receives; the bound is derived from operation counts the way tail_f64.optim_reference derives e_gcorr.
Nothing here depends on what the code under test returns."""
import functools

import torch

from tail_f64 import OPT_CHUNK, U, _Report, optim_grads, optim_state, optim_sum_depth, optim_table  # noqa: F401


def accum_reference(recs, grads, acc, first):
    """acc' = (first ? 0 : acc) + gcorr per tensor, in float64.  recs: the state the kernel's table points at (param, sn =
    (u, v, sigma, rows, cols) or None), grads / acc: fp32 CPU tensors (acc is ignored with first, whatever it holds).
    -> (ref, bound): lists of flat float64 tensors.

    The bound per element, with U = 2^-24:
      c = <G, W>/sigma    the sum of numel products through a chain of optim_sum_depth(numel) additions, the products'
                          own rounding and the division: (depth + 3) U sum|G W| / sigma (what optim_reference allows c)
      c u_r v_c           two products: 2 U |c u v|, and c's error times |u v|
      G - c u v           the difference: U (|G| + |c u v|)  (a fused multiply-subtract rounds once less)
      (.) * (1 / sigma)   the reciprocal and the product: 2 U |g'|
      acc + g'            the final addition: U |acc'|       (none with first: the value is stored as it is)
    A plain tensor has g' = G exactly, so only the final addition counts, and nothing at all with first."""
    refs, bounds = [], []
    for r, g, a in zip(recs, grads, acc):
        G = g.double().reshape(-1)
        if r["sn"] is None:
            gc, e = G, torch.zeros_like(G)
        else:
            u, v, sigma, rows, cols = r["sn"]
            sg = float(sigma.double())
            uv = torch.outer(u.double(), v.double()).reshape(-1)
            GW = G * r["param"].double().reshape(-1)
            c = float(GW.sum()) / sg
            e_c = (optim_sum_depth(G.numel()) + 3) * U * float(GW.abs().sum()) / sg
            gc = (G - c * uv) / sg
            e = (e_c * uv.abs() + 2 * U * abs(c) * uv.abs() + U * (G.abs() + abs(c) * uv.abs())) / sg + 2 * U * gc.abs()
        if first:
            out = gc
        else:
            out = a.double().reshape(-1) + gc
            e = e + U * out.abs()
        refs.append(out), bounds.append(e)
    return refs, bounds


def check_accum(got, refs, bounds, strict=True):
    """got: the accumulators after the call (fp32, one per tensor).  -> (worst error / bound, failures)"""
    rep = _Report()
    rep.bounded("acc", torch.cat([g.reshape(-1) for g in got]), torch.cat(refs), torch.cat(bounds))
    return rep.done(strict)


def _serial(parts):
    return functools.reduce(lambda a, b: a + b, parts, torch.tensor(0.0, dtype=torch.float32))


def emu_accum(recs, grads, acc, first, fault=None, other=None):
    """fp32 emulation of calm_grad_accum in the kernel's order: <G, W> per chunk, the chunks added in order, c = gw / sigma,
    g' = (G - c u v) * (1 / sigma), acc = first ? g' : acc + g'.  Returns the new accumulators; `acc` is not modified.
    fault: "first_ignored" (adds to the old accumulator although first is set), "no_inv_sigma" (the final 1 / sigma
    dropped), "other_uv" (u, v of `other`, the records of another micro-batch), "one_chunk" (c from the first chunk)."""
    out = []
    for k, (r, g, a) in enumerate(zip(recs, grads, acc)):
        g = g.float().reshape(-1)
        if r["sn"] is not None:
            u, v, sigma, rows, cols = r["sn"]
            if fault == "other_uv":
                u, v = other[k]["sn"][0], other[k]["sn"][1]
            parts = [(x * w).sum() for x, w in zip(g.split(OPT_CHUNK), r["param"].float().reshape(-1).split(OPT_CHUNK))]
            gw = parts[0] if fault == "one_chunk" else _serial(parts)
            c = gw / sigma[0]
            g = g - (c * u)[:, None].mul(v[None, :]).reshape(-1)
            if fault != "no_inv_sigma":
                g = g * (1 / sigma[0])
        if first and fault != "first_ignored":
            out.append(g.clone())
        else:
            out.append(a.float().reshape(-1) + g)
    return out
