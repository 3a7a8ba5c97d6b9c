"""CPU emulation of the loss entry points (calm_soft_ce_fwd / _bwd, calm_huber_tokens_fwd / _bwd, calm_top1_count) on top of
tests/emulated_backend.py, in fp32 and with the formulas the kernels use (row maximum subtracted before the exponential,
sum of non-negative terms for the loss) — used by tests/test_loss_*.py only.  It is never imported by the package."""
import torch

from emulated_backend import EmulatedBackend


class EmulatedLossBackend(EmulatedBackend):
    @staticmethod
    def _row_parts(logits, targets):
        z, y = logits.float(), targets.float()
        m = z.max(dim=1, keepdim=True).values
        ls = torch.log(torch.exp(z - m).sum(dim=1, keepdim=True))
        return z, y, m, ls

    def soft_ce_fwd(self, logits, targets, row_stats, loss, metrics, B, C):
        z, y, m, ls = self._row_parts(logits, targets)
        rows = (y * (m - z)).sum(dim=1) + ls[:, 0] * y.sum(dim=1)
        row_stats.copy_(torch.cat([m, ls], dim=1))
        loss.copy_(rows.sum() / B)
        if metrics is not None:
            finite = ~(torch.isnan(z).any(dim=1) | torch.isnan(y).any(dim=1))
            agree = (z.argmax(dim=1) == y.argmax(dim=1)) & finite        # torch.argmax: first maximal value
            metrics += torch.stack([rows.sum(), agree.sum().float(), torch.tensor(float(B)), torch.tensor(1.0)]).to(metrics)

    def soft_ce_bwd(self, logits, targets, row_stats, dloss, dlogits, B, C):
        z, y = logits.float(), targets.float()
        m, ls = row_stats[:, 0:1], row_stats[:, 1:2]
        dlogits.copy_(dloss.reshape(()) / B * (torch.exp((z - m) - ls) * y.sum(dim=1, keepdim=True) - y))

    @staticmethod
    def _diff(tokens, x, B, S):
        return tokens.reshape(B, S, S, 3).permute(0, 3, 1, 2) - x

    def huber_tokens_fwd(self, tokens, x, delta, loss, B, S):
        if S % 4:
            raise RuntimeError("calm_huber_tokens_fwd failed: code -3 (invalid argument/unsupported shape)")
        d = self._diff(tokens, x, B, S)
        ad = d.abs()
        loss.copy_(torch.where(ad <= delta, 0.5 * d * d, delta * (ad - 0.5 * delta)).sum() / d.numel())

    def huber_tokens_bwd(self, tokens, x, delta, dloss, dtokens, B, S):
        d = self._diff(tokens, x, B, S)
        g = dloss.reshape(()) / d.numel() * d.clamp(-delta, delta)
        dtokens.copy_(g.permute(0, 2, 3, 1).reshape(B, S, 3 * S))

    def top1_count(self, logits, labels, metrics, B, C):
        z = logits.float()
        hit = (z.argmax(dim=1) == labels) & ~torch.isnan(z).any(dim=1)
        metrics[1] += hit.sum().float()
        metrics[2] += float(B)
