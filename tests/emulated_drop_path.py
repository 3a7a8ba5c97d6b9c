"""CPU emulation of calm_drop_path (csrc/dropout.hip) on top of tests/emulated_dropout.py: the keep decision of sample b is
the dropout mask's decision for element index sample0 + b, one factor per row, and the entry point's two separately rounded
fp32 operations — used by tests/test_drop_path_*.py only.  It is never imported by the package."""
import numpy as np
import torch

from emulated_dropout import EmulatedDropoutBackend, keep_mask, threshold_and_scale


def row_factors(key, sample0, B, p):
    """fp32 torch tensor [B]: scale where sample sample0 + b is kept, 0 where it is dropped; key: (seed, offset)."""
    seed, offset = (int(k) for k in key)
    scale = threshold_and_scale(p)[1]
    return torch.from_numpy(np.where(keep_mask(seed, offset, sample0, B, p), scale, np.float32(0.0)).astype(np.float32))


class EmulatedDropPathBackend(EmulatedDropoutBackend):
    def drop_path(self, x, residual, y, B, L, p, key, sample0=0):
        if not 0.0 <= float(np.float32(p)) < 1.0 or B < 0 or L < 0 or sample0 < 0:
            raise RuntimeError("calm_drop_path failed: code -1 (invalid argument/unsupported shape)")
        if B == 0 or L == 0:
            return
        f = row_factors(key, sample0, B, p).to(x.device)
        v = x.reshape(-1)[:B * L].view(B, L).float() * f[:, None]                   # one fp32 rounding (bf16 widens exactly)
        if residual is not None:
            v = v + residual.reshape(-1)[:B * L].view(B, L).float()                 # a second one
        y.view(-1)[:B * L].copy_(v.reshape(-1))                                     # bf16 output: round to nearest even
