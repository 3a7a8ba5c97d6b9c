"""CPU emulation of the lean inference entry points (calm_attention_infer, calm_attention16_infer) on top of
tests/emulated_backend.py — used by tests/test_infer_*.py only.  It is never imported by the package.

The two methods run the stored emulation into scratch tensors of their own and hand back out and Mk alone, so what they
return equals EmulatedBackend.attn_fwd / attn16_fwd bit for bit — the property the kernels are tested for on the GPU.
The scratch is made with new_zeros: the tests that watch what ops.latent_mask_attention_infer allocates watch
torch.empty."""
from emulated_backend import EmulatedBackend


class EmulatedInferBackend(EmulatedBackend):
    def __init__(self):
        super().__init__()
        self.calls = []                       # (entry point, Sq) in call order

    def attn_fwd(self, *a):
        self.calls.append(("attn_fwd", a[-4]))
        return super().attn_fwd(*a)

    def attn16_fwd(self, *a):
        self.calls.append(("attn16_fwd", a[-3]))
        return super().attn16_fwd(*a)

    def attn_infer(self, q, k, v, w1, b1, s1, w2, b2, s2, out, Mk, B, Sq, Skv, H, hd):
        if not self.attn_fwd_supported(Sq, Skv, H, hd):
            raise RuntimeError("calm_attention_infer failed: code -3 (invalid argument/unsupported shape)")
        self.calls.append(("attn_infer", Sq))
        z = lambda *s: q.new_zeros(s)
        EmulatedBackend.attn_fwd(self, q, k, v, w1, b1, s1, w2, b2, s2, out, z(B, Sq, Skv), z(B, Sq, 2 * Skv),
                                 z(B, Sq, 2 * Skv), Mk, None, B, Sq, Skv, H, hd)

    def attn16_infer(self, q, k, v, w1, b1, s1, w2, b2, s2, out, Mk, B, S, H, hd):
        if not self.attn16_supported(S, H, hd):
            raise RuntimeError("calm_attention16_infer failed: code -3 (invalid argument/unsupported shape)")
        self.calls.append(("attn16_infer", S))
        z = lambda *s: q.new_zeros(s)
        EmulatedBackend.attn16_fwd(self, q, k, v, w1, b1, s1, w2, b2, s2, out, z(B, S, S), z(B, S, 2 * S), z(B, S, 2 * S),
                                   Mk, z(B, S, S), q.new_zeros((B, H, S), dtype=b1.dtype), B, S, H, hd)

    def gemm_describe(self, *args, **kw):
        """One kernel for every launch: the emulation's plan does not depend on C_pre, so a lean forward drops it."""
        return {"family": -1}
