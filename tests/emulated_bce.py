"""CPU emulation of the binary cross-entropy entry points (calm_bce_fwd / _bwd) on top of tests/emulated_loss.py, in fp32 and
with the formulas the kernels use (|z| * (z >= 0 ? 1 - t : t) + log1p(exp(-|z|)), the two-branch sigmoid) — used by
tests/test_bce_cpu.py only.  It is never imported by the package.  Every step of the two entry points is a method of its
own, so that a planted fault (tests/test_bce_cpu.py) changes exactly one thing."""
import torch

from emulated_loss import EmulatedLossBackend

SUM_CLASSES, THRESHOLD = 1, 2


class EmulatedBceBackend(EmulatedLossBackend):
    @staticmethod
    def _threshold(y, threshold):
        return (y > threshold).to(y.dtype)                          # (strict, compared in fp32)

    def _fwd_targets(self, y, flags, threshold):
        return self._threshold(y, threshold) if flags & THRESHOLD else y

    def _bwd_targets(self, y, flags, threshold):
        return self._threshold(y, threshold) if flags & THRESHOLD else y

    @staticmethod
    def _terms(z, t):
        a = z.abs()
        return a * torch.where(z >= 0, 1.0 - t, t) + torch.log1p(torch.exp(-a))

    @staticmethod
    def _denominator(flags, B, C):
        return float(B) if flags & SUM_CLASSES else float(B) * float(C)

    @staticmethod
    def _agreement_targets(y, t):
        return y                                                    # the ORIGINAL targets

    @staticmethod
    def _metrics_loss(loss, B):
        return loss * B

    @staticmethod
    def _upstream(dloss):
        return dloss.reshape(())

    @staticmethod
    def _classes(z):
        return z                                                    # (a fault drops the tail of every row here)

    def bce_fwd(self, logits, targets, flags, threshold, loss, metrics, B, C):
        z, y = logits.float(), targets.float()
        t = self._fwd_targets(y, flags, threshold)
        value = self._classes(self._terms(z, t)).sum() / self._denominator(flags, B, C)
        loss.copy_(value)
        if metrics is not None:
            finite = ~(torch.isnan(z).any(dim=1) | torch.isnan(y).any(dim=1))
            agree = (z.argmax(dim=1) == self._agreement_targets(y, t).argmax(dim=1)) & finite    # argmax: first maximal value
            metrics += torch.stack([self._metrics_loss(value, B), agree.sum().float(), torch.tensor(float(B)),
                                    torch.tensor(1.0)]).to(metrics)

    def bce_bwd(self, logits, targets, flags, threshold, dloss, dlogits, B, C):
        z, y = logits.float(), targets.float()
        t = self._bwd_targets(y, flags, threshold)
        e = torch.exp(-z.abs())
        s = torch.where(z >= 0, torch.ones_like(e), e) / (1.0 + e)
        g = self._upstream(dloss) / self._denominator(flags, B, C) * ((s - t) + (z - z))
        dlogits.zero_()
        self._classes(dlogits).copy_(self._classes(g))
