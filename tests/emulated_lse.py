"""CPU emulation of the row-LSE entry points of the fp32 attention (calm_attention_fwd_lse, calm_attention_bwd_lse,
calm_attention_bwd_lse_scratch_bytes) on top of tests/emulated_backend.py — used by tests/test_attention_lse_*.py only.
It is never imported by the package."""
import math

import torch

from emulated_backend import EmulatedBackend


class EmulatedLseBackend(EmulatedBackend):
    def attn_fwd_lse(self, q, k, v, w1, b1, s1, w2, b2, s2, out, R, hp, hg, Mk, lse, B, Sq, Skv, H, hd):
        self.attn_fwd(q, k, v, w1, b1, s1, w2, b2, s2, out, R, hp, hg, Mk, None, B, Sq, Skv, H, hd)
        lse.view(B, H, Sq).copy_(torch.logsumexp(self._logits(q, k, Mk, B, Sq, Skv, H, hd), dim=-1))

    @staticmethod
    def _logits(q, k, Mk, B, Sq, Skv, H, hd):
        qh, kh = q.view(B, Sq, H, hd).transpose(1, 2), k.view(B, Skv, H, hd).transpose(1, 2)
        return qh @ kh.transpose(-1, -2) / math.sqrt(hd) + Mk.view(B, 1, Sq, Skv)

    def attn_bwd_lse_scratch_bytes(self, B, Sq, Skv, H, hd):
        if B <= 0 or not self.attn_fwd_supported(Sq, Skv, H, hd):
            return 0
        return 2 * 4 * B * H * Sq * Skv

    def attn_bwd_lse(self, q, k, v, dout, Mk, lse, scratch, dq, dk, dv, dM, B, Sq, Skv, H, hd):
        need = self.attn_bwd_lse_scratch_bytes(B, Sq, Skv, H, hd)
        if need == 0 or scratch.numel() * scratch.element_size() < need:
            raise RuntimeError("calm_attention_bwd_lse failed: invalid argument/unsupported shape")
        # P rebuilt from what the lean forward left behind: no maximum, no sum, no division
        P = torch.exp(self._logits(q, k, Mk, B, Sq, Skv, H, hd) - lse.view(B, H, Sq, 1)).contiguous()
        dS = torch.empty_like(P)
        self.attn_bwd(q, k, v, dout, P, dS, dq, dk, dv, dM, B, Sq, Skv, H, hd)
