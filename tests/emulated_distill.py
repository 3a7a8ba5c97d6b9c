"""CPU emulation of the distillation entry points (calm_distill_fwd / _bwd) on top of tests/emulated_loss.py: plain torch
in fp32 with the kernels' formulas (every row maximum subtracted before every exponential, pT and q out of one expression,
the non-cancelling cross-entropy), `dmetrics`, `metrics` and the refusals of the C entry points.  `defect=` plants ONE fault
at a time, so that tests/test_distill_cpu.py can show that the float64 checker (tests/distill_f64.py) rejects each of them.
Used by tests/test_distill_*.py only; it is never imported by the package."""
import math

import torch

from emulated_loss import EmulatedLossBackend

ROW_STATS = 8
DEFECTS = ("no_t2", "t2_in_grad", "kl_swapped", "alpha_on_ce", "tail_skipped", "rows_from_256_dropped", "tie_highest")
_REFUSED = "failed: code {} (invalid argument/unsupported shape)"


def _argmax_lowest(v):
    """argmax along dim 1, lowest index among equals, NaN never selected (the kernels' rule); an all -inf row -> 0."""
    w = torch.where(torch.isnan(v), torch.full_like(v, -math.inf), v)
    return (w == w.max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)      # the first True


def _argmax_highest(v):
    w = torch.where(torch.isnan(v), torch.full_like(v, -math.inf), v)
    C = v.shape[1]
    return C - 1 - (w == w.max(dim=1, keepdim=True).values).flip(1).to(torch.int64).argmax(dim=1)


class EmulatedDistillBackend(EmulatedLossBackend):
    def __init__(self, defect=None):
        super().__init__()
        if defect is not None and defect not in DEFECTS:
            raise ValueError(defect)
        self.defect = defect

    # ---- the refusals of the C entry points (before anything is computed) -------------------------------------------------
    @staticmethod
    def _refuse(what, logits, teacher, targets, temperature, alpha, mode, B, C):
        T, a = float(temperature), float(alpha)
        bad = (B <= 0 or C <= 0 or any(t is None for t in (logits, teacher, targets))
               or any(t.stride(0) < C and t.shape[0] > 1 for t in (logits, teacher, targets))
               or not (T > 0 and math.isfinite(T)) or not (0.0 <= a <= 1.0) or mode not in ("soft", "hard")
               or teacher.dtype not in (torch.float32, torch.bfloat16))
        if bad:
            raise RuntimeError(f"{what} " + _REFUSED.format(-1))
        if C > 65536:
            raise RuntimeError(f"{what} " + _REFUSED.format(-3))

    def _cols(self, C):
        """The columns the row sums see (all of them, unless the planted fault skips the last C % 4)."""
        return C - C % 4 if self.defect == "tail_skipped" else C

    def _stats(self, logits, teacher, temperature):
        z, t = logits.float(), teacher.float()                     # bf16 widens exactly
        inv_t = 1.0 / float(temperature)
        n = self._cols(z.shape[1])
        zm = z.max(dim=1, keepdim=True).values
        tm = t.max(dim=1, keepdim=True).values
        ls1 = torch.log(torch.exp(z - zm)[:, :n].sum(dim=1, keepdim=True))
        lst = torch.log(torch.exp((z - zm) * inv_t)[:, :n].sum(dim=1, keepdim=True))
        lsq = torch.log(torch.exp((t - tm) * inv_t)[:, :n].sum(dim=1, keepdim=True))
        k = (_argmax_highest if self.defect == "tie_highest" else _argmax_lowest)(t)
        return z, t, inv_t, zm, tm, ls1, lst, lsq, k

    def distill_fwd(self, logits, teacher, targets, temperature, alpha, mode, row_stats, loss, metrics, dmetrics, B, C):
        self._refuse("calm_distill_fwd", logits, teacher, targets, temperature, alpha, mode, B, C)
        z, t, inv_t, zm, tm, ls1, lst, lsq, k = self._stats(logits, teacher, temperature)
        y = targets.float()
        n = self._cols(C)
        T, a = float(temperature), float(alpha)
        ysum = y[:, :n].sum(dim=1)
        ce = (y * (zm - z))[:, :n].sum(dim=1) + ls1[:, 0] * ysum
        if mode == "soft":
            lq, lp = (t - tm) * inv_t - lsq, (z - zm) * inv_t - lst
            if self.defect == "kl_swapped":
                lq, lp = lp, lq
            q = torch.exp(lq)
            d = torch.where(q == 0, torch.zeros_like(q), q * (lq - lp))[:, :n].sum(dim=1)
            w = a if self.defect == "no_t2" else a * T * T
        else:
            d = (zm[:, 0] - z.gather(1, k[:, None])[:, 0]) + ls1[:, 0]
            d = torch.where(torch.isnan(t).any(dim=1), torch.full_like(d, math.nan), d)
            w = a
        ce_w = a if self.defect == "alpha_on_ce" else 1.0 - a
        rows = ce_w * ce + w * d
        flag = torch.zeros(B)                                      # [7]: NaN where hard mode's argmax skipped a NaN
        if mode == "hard":
            flag = torch.where(torch.isnan(t).any(dim=1), torch.full_like(flag, math.nan), flag)
        row_stats.reshape(B, -1)[:, :ROW_STATS].copy_(torch.cat(
            [zm, ls1, lst, tm, lsq, k[:, None].float(), ysum[:, None], flag[:, None]], dim=1))
        total = rows[:256].sum() if self.defect == "rows_from_256_dropped" else rows.sum()
        loss.copy_(total / B)
        nan_z, nan_t, nan_y = (torch.isnan(v).any(dim=1) for v in (z, t, y))
        zi = _argmax_lowest(z)
        if metrics is not None:
            agree = (zi == _argmax_lowest(y)) & ~nan_z & ~nan_y
            metrics += torch.stack([total, agree.sum().float(), torch.tensor(float(B)), torch.tensor(1.0)]).to(metrics)
        if dmetrics is not None:
            agree_t = (zi == _argmax_lowest(t)) & ~nan_z & ~nan_t
            dmetrics += torch.stack([ce.sum(), d.sum(), agree_t.sum().float(), torch.tensor(float(B))]).to(dmetrics)

    def distill_bwd(self, logits, teacher, targets, temperature, alpha, mode, row_stats, dloss, dlogits, B, C):
        self._refuse("calm_distill_bwd", logits, teacher, targets, temperature, alpha, mode, B, C)
        if tuple(dlogits.shape) != (B, C) or not dlogits.is_contiguous():
            raise ValueError("distill_bwd: dlogits is contiguous [B,C]")
        z, t, y = logits.float(), teacher.float(), targets.float()
        rs = row_stats.reshape(B, -1)
        zm, ls1, lst, tm, lsq, k, ysum = (rs[:, i:i + 1] for i in range(7))
        T, a = float(temperature), float(alpha)
        inv_t = 1.0 / T
        p1 = torch.exp((z - zm) - ls1)
        ce_w = a if self.defect == "alpha_on_ce" else 1.0 - a
        if mode == "soft":
            pt, q = torch.exp((z - zm) * inv_t - lst), torch.exp((t - tm) * inv_t - lsq)
            kd = (q - pt) if self.defect == "kl_swapped" else (pt - q)
            gw = a * T * T if self.defect == "t2_in_grad" else (a / T if self.defect == "no_t2" else a * T)
        else:
            kd = p1 - (torch.arange(C)[None, :] == k.to(torch.int64)).float() + rs[:, 7:8]
            gw = a
        g = dloss.reshape(()) / B * (ce_w * (p1 * ysum - y) + gw * kd)
        if self.defect == "tail_skipped" and C % 4:
            g[:, C - C % 4:] = 0.0
        if self.defect == "rows_from_256_dropped":
            g[256:] = 0.0
        dlogits.copy_(g)

    def distill_scratch_floats(self, B, C):
        return 5 * B
