"""TEST INFRASTRUCTURE: calm_optim_step_lamb (csrc/optim.hip) emulated in fp32 torch in the header's operation order over
tail_f64's records — passes 1 and 2 as test_tail_f64_cpu.emu_optim forms them (per-chunk partials added in chunk order, the
tensors' norms, the clip), then the moments, r, u, the per-chunk sums of w^2 and u^2 added in chunk order, both roots, the
trust rule, the clip and the subtraction — and the planted faults the float64 checker (lamb_f64.py) must reject, each one
changed line.  Products and sums are separate fp32 operations; a chunk's own sum is torch's (pairwise: a smaller error than
the kernel's serial runs, inside the same bound).  The state is not modified: a call returns what lamb_f64.check takes."""
import functools

import torch

import tail_f64 as tf

CHUNK = tf.OPT_CHUNK
FAULTS = ("norm_without_decay", "trust_per_chunk", "adapt_without_decay", "no_bc1", "no_bc2", "w_norm_after_update",
          "clip_ignored", "u_from_old_m", "neighbour_trust", "squared_norms", "write_on_found_inf")
FMAX = 3.402823466e38


def _f(x):
    return torch.tensor(float(x), dtype=torch.float32)


def _serial(parts):
    return functools.reduce(lambda a, b: a + b, parts, _f(0.0))


def lamb_step(recs, grads, hp, grad_scale, step, lamb_hp, lr_dev=None, groups=None, group_hp=None, trust_before=None,
              fault=None):
    """One call.  Arguments as for lamb_f64.reference; trust_before: the table the call finds (default (0, 0, 1) rows).
    -> dict(p, m, v: flat fp32; norm, found_inf, step; trust: float32 [n, 3])."""
    assert fault is None or fault in FAULTS
    lr0, b1, b2, eps, wd0, max_norm = (_f(x) for x in hp[:6])
    if lr_dev is not None:
        lr0 = _f(lr_dev)
    clip_t, always = _f(lamb_hp[0] or 0.0), bool(lamb_hp[1])
    inv_scale = 1 / _f(grad_scale) if grad_scale is not None else _f(1.0)
    n = len(recs)
    table = trust_before.clone() if trust_before is not None else torch.tensor([[0.0, 0.0, 1.0]] * n)
    # ---- passes 1 and 2: calm_optim_step's
    n2s, cs, uvs, bad = [], [], [], False
    for r, g in zip(recs, grads):
        g = g.float().reshape(-1)
        bad = bad or not bool((g.abs() <= FMAX).all())
        n2, c, uv = _serial([(x * x).sum() for x in g.split(CHUNK)]), None, None
        if r["sn"] is not None:
            u, v, sigma, rows, cols = r["sn"]
            uv = torch.outer(u, v).reshape(-1)
            gw = _serial([(a * b).sum() for a, b in zip(g.split(CHUNK), r["param"].reshape(-1).split(CHUNK))])
            guv = _serial([(a * b).sum() for a, b in zip(g.split(CHUNK), uv.split(CHUNK))])
            uu, vv, sg = (u * u).sum(), (v * v).sum(), sigma[0]
            c = gw / sg
            n2 = (n2 - 2 * c * guv + c * c * uu * vv) / (sg * sg)
        n2s.append(n2.clamp_min(0.0)), cs.append(c), uvs.append(uv)
    norm = torch.stack(n2s).sum().sqrt() * inv_scale
    bad = bad or not bool(norm.abs() <= FMAX)
    P = [r["param"].reshape(-1).clone() for r in recs]
    M = [r["exp_avg"].reshape(-1).clone() for r in recs]
    V = [r["exp_avg_sq"].reshape(-1).clone() for r in recs]
    flat = lambda: dict(p=torch.cat(P), m=torch.cat(M), v=torch.cat(V))       # noqa: E731
    if bad and fault != "write_on_found_inf":
        return dict(flat(), norm=float(norm), found_inf=1.0, step=step, trust=table)
    clip = torch.minimum(_f(1.0), max_norm / (norm + _f(1e-6))) if float(max_norm) > 0 else _f(1.0)
    mul = clip * inv_scale
    t = step if bad else step + 1
    te = _f(max(t, 1))
    bc1, bc2 = 1 - torch.pow(b1, te), 1 - torch.pow(b2, te)
    isb2 = 1 / bc2.sqrt()
    if fault == "no_bc1":
        bc1 = _f(1.0)
    if fault == "no_bc2":
        isb2 = _f(1.0)
    u_of = lambda m, v, w, wd: (m / (v.sqrt() * isb2 + eps)) / bc1 + wd * w   # noqa: E731  (lamb_u)
    prev_trust = _f(1.0)
    for k, (r, g) in enumerate(zip(recs, grads)):
        lr, wd = (lr0, wd0) if groups is None else (_f(group_hp[groups[k]][0]), _f(group_hp[groups[k]][1]))
        g = g.float().reshape(-1)
        if cs[k] is not None:
            g = (g - cs[k] * uvs[k]) * (1 / r["sn"][2][0])
        g = g * mul
        w, m_old = P[k], M[k]
        # ---- pass 3
        m = m_old + (g - m_old) * (1 - b1)
        v = V[k] * b2 + g * g * (1 - b2)
        u = u_of(m, v, w, wd)
        for_norm = u_of(m, v, w, _f(0.0)) if fault == "norm_without_decay" else u
        w2 = [(x * x).sum() for x in w.split(CHUNK)]
        u2 = [(x * x).sum() for x in for_norm.split(CHUNK)]
        # ---- pass 4
        adapt = always or float(wd) != 0.0 or fault == "adapt_without_decay"

        def trust_of(W2, U2):
            wn, un = W2.sqrt(), U2.sqrt()
            if fault == "squared_norms":
                wn, un = W2, U2
            tr = wn / un if adapt and bool(wn > 0) and bool(un > 0) else _f(1.0)
            if float(clip_t) > 0 and fault != "clip_ignored":
                tr = torch.minimum(tr, clip_t)
            return wn, un, tr

        wn, un, trust = trust_of(_serial(w2), _serial(u2))
        table[k] = torch.stack([wn, un, trust])
        used = prev_trust if fault == "neighbour_trust" and k > 0 else trust
        prev_trust = trust
        if fault == "u_from_old_m":
            u = u_of(m_old, v, w, wd)
        if float(lr) != 0.0:
            if fault == "trust_per_chunk":
                P[k] = torch.cat([wc - (lr * trust_of(a, b)[2]) * uc
                                  for wc, uc, a, b in zip(w.split(CHUNK), u.split(CHUNK), w2, u2)])
            else:
                P[k] = w - (lr * used) * u
        if fault == "w_norm_after_update":
            table[k, 0] = (P[k] * P[k]).sum().sqrt()
            _, _, tr2 = trust_of((P[k] * P[k]).sum(), _serial(u2))
            table[k, 2] = tr2
            if float(lr) != 0.0:
                P[k] = w - (lr * tr2) * u
        M[k], V[k] = m, v
    return dict(flat(), norm=float(norm), found_inf=float(bad), step=t, trust=table)
