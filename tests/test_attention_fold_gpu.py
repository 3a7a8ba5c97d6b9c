"""Folded route of the stored-P attention backward on the MI355X (calm_attention_bwd_front, calm_attention_bwd_back):
the front kernel, then the back kernels with a given random dR, against float64 torch on the CPU — one case per compiled
geometry, B = 2 (batch strides), H >= 2 (the dR registers are reused across the heads), head dims below 16 and not a
multiple of 16, an odd number of 16-column blocks.  fp32, 1e-4 rel (helpers.rel_err), as tests/test_attention_gpu.py."""
import functools
import math

import pytest
import torch

import calm_vit_dte_amd as calm
from helpers import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4

SHAPES = [
    # B, S, H, hd
    (2, 32, 2, 24), (2, 48, 3, 48),
    (2, 80, 3, 40),                      # odd number of 16-column blocks
    (2, 80, 3, 20),                      # hd below 16 + 4: one full and one quarter d-tile
    (2, 128, 2, 64),
    (2, 176, 2, 88), (2, 176, 3, 44),    # hd not a multiple of 16
    (2, 224, 2, 112),
]


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _case(B, S, H, hd):
    """Inputs, the float64 reference and every GPU result of one shape — computed once, shared by the tests, not modified."""
    D = H * hd
    sc = 1.0 / math.sqrt(hd)
    q, k, v, dout = rnd(B, S, D, seed=1) * 0.5, rnd(B, S, D, seed=2) * 0.5, rnd(B, S, D, seed=3), rnd(B, S, D, seed=8)
    P = torch.softmax(rnd(B, H, S, S, seed=9) * 2, dim=-1)
    dR = rnd(B, S, S, seed=10) * 0.05
    # float64 reference
    q6, k6, v6, do6, P6, dR6 = (t.double() for t in (q, k, v, dout, P, dR))
    qh, kh, vh, doh = (t.view(B, S, H, hd).transpose(1, 2) for t in (q6, k6, v6, do6))
    dP = doh @ vh.transpose(-1, -2)
    dS = P6 * (dP - (P6 * dP).sum(dim=-1, keepdim=True))
    X = sc * dS + dR6[:, None]
    merge = lambda t: t.transpose(1, 2).reshape(B, S, D)    # noqa: E731
    ref = {"dS": dS, "dM": dS.sum(dim=1), "dv": merge(P6.transpose(-1, -2) @ doh), "dq": merge(X @ kh),
           "dk": merge(X.transpose(-1, -2) @ qh)}
    # the device
    be = calm.backend.get_backend()
    gq, gk, gv, gdo, gP, gdR = (t.cuda() for t in (q, k, v, dout, P, dR))
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")    # noqa: E731

    def folded():
        o = {n: nan(*s) for n, s in (("dS", (B, H, S, S)), ("dM", (B, S, S)), ("dq", (B, S, D)), ("dk", (B, S, D)),
                                     ("dv", (B, S, D)))}
        be.attn_bwd_front(gv, gdo, gP, o["dS"], o["dM"], B, S, S, H, hd)
        be.attn_bwd_back(gq, gk, gdo, gP, o["dS"], gdR, o["dq"], o["dk"], o["dv"], B, S, S, H, hd)
        return o

    first, second = folded(), folded()
    # the unfolded route of the same build: the two fused launches, then the two dR products as accumulating GEMMs
    u = {n: nan(*s) for n, s in (("dS", (B, H, S, S)), ("dM", (B, S, S)), ("dq", (B, S, D)), ("dk", (B, S, D)),
                                 ("dv", (B, S, D)))}
    be.attn_bwd(gq, gk, gv, gdo, gP, u["dS"], u["dq"], u["dk"], u["dv"], u["dM"], B, S, S, H, hd)
    be.gemm(gdR, gk, u["dq"], S, D, S, (S, 1, S * S, 0), (1, D, S * D, 0), (D, S * D, 0), batch=(B, 1), accumulate=True)
    be.gemm(gdR, gq, u["dk"], S, D, S, (1, S, S * S, 0), (1, D, S * D, 0), (D, S * D, 0), batch=(B, 1), accumulate=True)
    torch.cuda.synchronize()
    return ref, first, second, u


@pytest.mark.parametrize("B,S,H,hd", SHAPES)
def test_front_and_back_against_float64(B, S, H, hd):
    assert calm.backend.get_backend().attn_fwd_supported(S, S, H, hd)
    ref, got, _, _ = _case(B, S, H, hd)
    for name in ("dS", "dM", "dv", "dq", "dk"):
        assert torch.isfinite(got[name]).all(), name            # every element of the NaN-filled outputs was written
        err = rel_err(got[name], ref[name])
        print(f"fold {B}x{S}x{H}x{hd} {name}: {err:.3e}")
        assert err < TOL, name


@pytest.mark.parametrize("B,S,H,hd", SHAPES)
def test_front_is_bit_identical_to_the_unsplit_query_side_and_the_route_repeats(B, S, H, hd):
    _, first, second, unfolded = _case(B, S, H, hd)
    for name in ("dS", "dM", "dv"):                             # the same code: DQ = false only compiles dQ out; dV as before
        assert torch.equal(first[name], unfolded[name]), name
    for name in ("dS", "dM", "dq", "dk", "dv"):                 # no atomics: two runs agree bit for bit
        assert torch.equal(first[name], second[name]), name


@pytest.mark.parametrize("B,S,H,hd", SHAPES)
def test_folded_dq_dk_agree_with_the_unfolded_route(B, S, H, hd):
    _, first, _, unfolded = _case(B, S, H, hd)
    for name in ("dq", "dk"):
        assert torch.isfinite(unfolded[name]).all(), name
        err = rel_err(first[name], unfolded[name])
        print(f"fold vs unfolded {B}x{S}x{H}x{hd} {name}: {err:.3e}")
        assert err < TOL, name


def test_unsupported_shapes_and_missing_tensors_are_refused():
    be = calm.backend.get_backend()
    assert not be.attn_bwd_fold_preferred(36, 36, 3, 36) and not be.attn_bwd_fold_preferred(224, 176, 6, 112)
    e = lambda *s: torch.empty(*s, device="cuda")    # noqa: E731
    B, S, H, hd = 1, 64, 4, 24                                  # no instantiation for 4 key tiles
    D = H * hd
    with pytest.raises(RuntimeError, match="calm_attention_bwd_front"):
        be.attn_bwd_front(e(B, S, D), e(B, S, D), e(B, H, S, S), e(B, H, S, S), e(B, S, S), B, S, S, H, hd)
    with pytest.raises(RuntimeError, match="calm_attention_bwd_back"):
        be.attn_bwd_back(e(B, S, D), e(B, S, D), e(B, S, D), e(B, H, S, S), e(B, H, S, S), e(B, S, S), e(B, S, D),
                         e(B, S, D), e(B, S, D), B, S, S, H, hd)
