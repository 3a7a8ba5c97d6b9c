"""CPU emulation of the folded-route entry points of the fp32 attention backward (calm_attention_bwd_front,
calm_attention_bwd_back, calm_attention_bwd_fold_preferred) on top of tests/emulated_backend.py — used by
tests/test_attention_fold_cpu.py only.  It is never imported by the package."""
import math

from emulated_backend import EmulatedBackend


class EmulatedFoldBackend(EmulatedBackend):
    def __init__(self):
        super().__init__()
        self.fold_calls = []                                     # "front" / "back", in call order

    def attn_bwd_fold_preferred(self, Sq, Skv, H, hd):
        return self.attn_fwd_supported(Sq, Skv, H, hd)

    def attn_bwd_front(self, v, dout, P, dS, dM, B, Sq, Skv, H, hd):
        self.fold_calls.append("front")
        vh, doh = (t.view(B, -1, H, hd).transpose(1, 2) for t in (v, dout))
        Pv = P.view(B, H, Sq, Skv)
        dP = doh @ vh.transpose(-1, -2)
        ds = Pv * (dP - (Pv * dP).sum(dim=-1, keepdim=True))
        dS.view(B, H, Sq, Skv).copy_(ds)
        dM.view(B, Sq, Skv).copy_(ds.sum(dim=1))

    def attn_bwd_back(self, q, k, dout, P, dS, dR, dq, dk, dv, B, Sq, Skv, H, hd):
        self.fold_calls.append("back")
        D = H * hd
        qh, kh, doh = (t.view(B, -1, H, hd).transpose(1, 2) for t in (q, k, dout))
        Pv = P.view(B, H, Sq, Skv)
        X = dS.view(B, H, Sq, Skv) * (1.0 / math.sqrt(hd)) + dR.view(B, 1, Sq, Skv)
        dq.view(B, Sq, D).copy_((X @ kh).transpose(1, 2).reshape(B, Sq, D))
        dk.view(B, Skv, D).copy_((X.transpose(-1, -2) @ qh).transpose(1, 2).reshape(B, Skv, D))
        dv.view(B, Skv, D).copy_((Pv.transpose(-1, -2) @ doh).transpose(1, 2).reshape(B, Skv, D))
