#!/usr/bin/env python3
"""Same-process timing of the stored-P attention backward, core + the two dR products, at the four Small-224 and the four
Base-224 stages (B = 256):
  composite  the batched-GEMM composition (calm_gemm + calm_softmax_bwd_heads) + the two dR GEMMs
  fused      calm_attention_bwd + the two dR GEMMs
  folded     calm_attention_bwd_front + calm_attention_bwd_back (dR folded into the dQ / dK contractions)
The mask-MLP backward between front and back is the same work on every route and is left out.  'today' is what
calm_attention_bwd_preferred picks of the first two; calm_attention_bwd_fold_preferred is set from folded vs today."""
import os, sys, math
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import calm_vit_dte_amd as calm
be = calm.backend.get_backend()


def t_med(fn, n=10, warm=2):
    for _ in range(warm): fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2]


SHAPES = ((256, 224, 6, 112), (256, 176, 6, 88), (256, 128, 6, 64), (256, 80, 6, 40),          # Small-224
          (256, 224, 12, 56), (256, 176, 12, 44), (256, 128, 12, 32), (256, 80, 12, 20))       # Base-224
for B, S, H, hd in SHAPES:
    D = H * hd
    g = lambda *s: torch.randn(*s, device="cuda") * 0.3
    q, k, v, dout = g(B, S, D), g(B, S, D), g(B, S, D), g(B, S, D)
    P = torch.softmax(g(B, H, S, S), dim=-1)
    dR = g(B, S, S) * 0.1
    dS, dq, dk, dv, dM = torch.empty_like(P), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), torch.empty(B, S, S, device="cuda")
    scale = 1 / math.sqrt(hd)
    pb = (H * S * S, S * S)

    def dr_gemms():
        be.gemm(dR, k, dq, S, D, S, (S, 1, S * S, 0), (1, D, S * D, 0), (D, S * D, 0), batch=(B, 1), accumulate=True)
        be.gemm(dR, q, dk, S, D, S, (1, S, S * S, 0), (1, D, S * D, 0), (D, S * D, 0), batch=(B, 1), accumulate=True)

    def composite():
        be.gemm(dout, v, dS, S, S, hd, (D, 1, S * D, hd), (D, 1, S * D, hd), (S,) + pb, batch=(B, H))
        be.gemm(P, dout, dv, S, hd, S, (1, S) + pb, (1, D, S * D, hd), (D, S * D, hd), batch=(B, H))
        be.softmax_bwd_heads(P, dS, dM, B, H, S, S)
        be.gemm(dS, k, dq, S, hd, S, (S, 1) + pb, (1, D, S * D, hd), (D, S * D, hd), batch=(B, H), alpha=scale)
        be.gemm(dS, q, dk, S, hd, S, (1, S) + pb, (1, D, S * D, hd), (D, S * D, hd), batch=(B, H), alpha=scale)
        dr_gemms()

    def fused():
        be.attn_bwd(q, k, v, dout, P, dS, dq, dk, dv, dM, B, S, S, H, hd)
        dr_gemms()

    def folded():
        be.attn_bwd_front(v, dout, P, dS, dM, B, S, S, H, hd)
        be.attn_bwd_back(q, k, dout, P, dS, dR, dq, dk, dv, B, S, S, H, hd)

    tg = t_med(dr_gemms)
    tc, tf, tn = t_med(composite), t_med(fused), t_med(folded)
    t_front = t_med(lambda: be.attn_bwd_front(v, dout, P, dS, dM, B, S, S, H, hd))
    today = tf if be.attn_bwd_preferred(S, S, H, hd) else tc
    print(f"B={B} S={S} H={H} hd={hd}: composite {tc:6.3f}  fused {tf:6.3f}  (dR GEMMs alone {tg:5.3f})  today {today:6.3f}  "
          f"folded {tn:6.3f} ms (front {t_front:5.3f})  today/folded {today / tn:4.2f}x", flush=True)
