"""The checker of the distillation entry points (calm_distill_fwd / _bwd): a float64 reference built from torch.logsumexp in
double, the inputs of every case, and the bounds.  Shared by tests/test_distill_cpu.py (on the torch emulation of the entry
points and on its planted faults) and tests/test_distill_gpu.py (on the kernels).

Bounds:
  dlogits, row_stats    helpers.rel_err <= 1e-4 — the project's fp32 kernel tolerance (TOL of tests/test_loss_gpu.py); the
                        row statistics are compared column by column, the teacher argmax exactly;
  loss                  |loss - ref| <= 1e-4 * ((1 - alpha) * CE_ref + w * A_ref): the KL is a sum of terms of both signs, so
                        the bound is relative to the magnitude of what is summed, A_ref = mean_b sum_c q_c |log q_c - log
                        pT_c| in float64 (hard mode: A_ref = D_ref); w = alpha T^2 (soft) or alpha (hard);
  counts                exact."""
import math

import torch

from helpers import rel_err

TOL = 1e-4
# (B, C): one class; below a vector; a short row; the vector path; a tail with every second row misaligned; more partials
# than threads in the final workgroup; a row longer than the register-resident path; the limit
CASES = [(1, 1), (3, 3), (3, 10), (4, 1000), (5, 1001), (257, 1000), (2, 21843), (2, 65536)]
# (B, C, T, alpha, mode, logit scale, teacher dtype) — every case at the defaults, then the variations on a subset
VARIANTS = ([(B, C, 2.0, 0.5, "soft", 1.0, "f32") for B, C in CASES] +
            [(B, C, 1.0, 0.5, "hard", 1.0, "f32") for B, C in CASES] +
            [(4, 1000, T, a, "soft", 1.0, "f32") for T in (0.5, 1.0, 4.0) for a in (0.0, 0.5, 1.0)] +
            [(5, 1001, 1.0, a, "hard", 1.0, "f32") for a in (0.0, 1.0)] +
            [(B, C, 4.0, 0.5, mode, 30.0, "f32") for B, C in ((5, 1001), (2, 21843)) for mode in ("soft", "hard")] +
            [(B, C, 2.0, 0.5, mode, 1.0, "bf16") for B, C in ((3, 10), (4, 1000), (5, 1001), (2, 21843))
             for mode in ("soft", "hard")])


def inputs(B, C, scale=1.0, seed=0, teacher="f32"):
    """Student logits scale * randn, teacher logits of the same scale correlated with them (so that the argmaxes agree on
    some rows and differ on others), CutMix-style targets: two classes per row with weights lam, 1 - lam."""
    g = torch.Generator().manual_seed(seed + 7919 * B + C)
    z = torch.randn(B, C, generator=g) * scale
    t = (0.6 * z + 0.8 * scale * torch.randn(B, C, generator=g))
    if teacher == "bf16":
        t = t.to(torch.bfloat16)
    y = torch.zeros(B, C)
    lam = torch.rand(B, generator=g) * 0.8 + 0.1
    rows = torch.arange(B)
    y[rows, torch.randint(0, C, (B,), generator=g)] += lam
    y[rows, torch.randint(0, C, (B,), generator=g)] += 1.0 - lam
    return z, t, y


def _argmax_lowest(v):
    w = torch.where(torch.isnan(v), torch.full_like(v, -math.inf), v)
    return (w == w.max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)


def reference(z, t, y, T=1.0, alpha=0.5, mode="soft", dloss=1.0):
    """Everything the entry points produce, in float64, from the formulas of include/calm_vit.h."""
    z, t, y = z.double(), t.double(), y.double()
    B, C = z.shape
    lse1 = torch.logsumexp(z, dim=1, keepdim=True)
    lset = torch.logsumexp(z / T, dim=1, keepdim=True)
    lseq = torch.logsumexp(t / T, dim=1, keepdim=True)
    zm, tm = z.max(dim=1, keepdim=True).values, t.max(dim=1, keepdim=True).values
    ysum = y.sum(dim=1, keepdim=True)
    p1, pt, q = torch.exp(z - lse1), torch.exp(z / T - lset), torch.exp(t / T - lseq)
    ce = (y * (lse1 - z)).sum(dim=1)
    k = _argmax_lowest(t)
    if mode == "soft":
        diff = (t / T - lseq) - (z / T - lset)
        terms = torch.where(q == 0, torch.zeros_like(q), q * diff)
        d, a_rows = terms.sum(dim=1), terms.abs().sum(dim=1)
        w, kd = alpha * T * T, alpha * T * (pt - q)
    else:
        d = (lse1 - z.gather(1, k[:, None]))[:, 0]
        a_rows = d
        w, kd = alpha, alpha * (p1 - torch.nn.functional.one_hot(k, C).double())
    rows = (1 - alpha) * ce + w * d
    nan_z, nan_t, nan_y = (torch.isnan(v).any(dim=1) for v in (z, t, y))
    zi = _argmax_lowest(z)
    return {
        "loss": rows.mean(), "row_sum": rows.sum(), "ce_sum": ce.sum(), "d_sum": d.sum(),
        "loss_bound": TOL * float((1 - alpha) * ce.mean() + w * a_rows.mean()), "w": w,
        "dlogits": dloss / B * ((1 - alpha) * (p1 * ysum - y) + kd),
        "row_stats": torch.cat([zm, lse1 - zm, lset - zm / T, tm, lseq - tm / T, k[:, None].double(), ysum], dim=1),
        "agree_y": int(((zi == _argmax_lowest(y)) & ~nan_z & ~nan_y).sum()),
        "agree_t": int(((zi == k) & ~nan_z & ~nan_t).sum()),
    }


STAT_NAMES = ("max z", "log sum exp(z - max)", "log sum exp((z - max)/T)", "max t", "log sum exp((t - max)/T)",
              "argmax t", "sum y")


def check(loss, dlogits, row_stats, ref, label="", strict=True):
    """Compare one forward + backward with the reference: -> (figures, failures); strict raises on the first failure list."""
    B = ref["dlogits"].shape[0]
    rs = torch.as_tensor(row_stats).detach().double().cpu().reshape(B, -1)
    figures = {"loss": abs(float(loss) - float(ref["loss"])), "loss_bound": ref["loss_bound"],
               "dlogits": rel_err(dlogits.detach(), ref["dlogits"])}
    failures = []
    if not figures["loss"] <= ref["loss_bound"]:                   # (a NaN fails)
        failures.append(("loss", figures["loss"], ref["loss_bound"]))
    if not figures["dlogits"] <= TOL:
        failures.append(("dlogits", figures["dlogits"], TOL))
    for i, name in enumerate(STAT_NAMES):
        want, got = ref["row_stats"][:, i], rs[:, i]
        if name == "argmax t":
            e = float((want != got).sum())
            bound = 0.0
        else:
            # a statistic that is 0 in every row (log of one term) is compared absolutely
            e = rel_err(got, want) if float(want.abs().max()) > 0 else float(got.abs().max())
            bound = TOL
        figures[name] = e
        if not e <= bound:
            failures.append((name, e, bound))
    if strict:
        assert not failures, f"{label}: {failures}"
    return figures, failures
