"""The two staging forms of calm_attention_bwd_back on the MI355X (calm_attention_set_option, CALM_ATTN_OPT_BACK): the whole
head stripe in LDS ("stripe") against 32-column slabs through a two-slot ring ("ring").  Per shape the front kernel runs
once; the back kernels then run forced to either form from the same dS and dR, into NaN-filled outputs with a guard band
of 64 floats on either side.  Both forms perform the same MFMA chains in the same order, so dq, dk and dv have to agree
bit for bit; they are also held against the float64 reference of tests/test_attention_fold_gpu.py (same inputs, same
formulas, 1e-4 rel).  Shapes: the eight of that test (one per compiled geometry and more), and four for the slab
sequence itself — one head (the last step has no next stripe to request), a single one-tile slab per stripe, four full
slabs, and DT = 3 with a partial last d-tile (the last slab holds one tile, its second chain runs with d2 = 0)."""
import functools
import math

import pytest
import torch

import calm_vit_dte_amd as calm
from helpers import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
GUARD = 64

SHAPES = [
    # B, S, H, hd
    (2, 32, 2, 24), (2, 48, 3, 48), (2, 80, 3, 40), (2, 80, 3, 20), (2, 128, 2, 64), (2, 176, 2, 88), (2, 176, 3, 44),
    (2, 224, 2, 112),                    # tests/test_attention_fold_gpu.py
    (2, 32, 1, 24),                      # one head: no next head to prefetch
    (2, 48, 3, 16),                      # a single one-tile slab per stripe
    (2, 32, 2, 128),                     # four full slabs
    (1, 80, 3, 36),                      # DT = 3: last slab one tile, partial last d-tile
]
NAMES = ("dq", "dk", "dv")


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


class Guarded:
    """[B,S,D] output in the middle of a NaN-filled allocation: GUARD floats in front of it and behind it"""

    def __init__(self, *shape):
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(*shape)

    def guards_untouched(self):
        return bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all())


@functools.lru_cache(maxsize=None)
def _case(B, S, H, hd):
    """Inputs, the float64 reference, and the back kernels' outputs in both forms — computed once, shared, not modified."""
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
    ref = {"dv": merge(P6.transpose(-1, -2) @ doh), "dq": merge(X @ kh), "dk": merge(X.transpose(-1, -2) @ qh)}
    # the device: front once, then back in each form from the same dS and dR
    be = calm.backend.get_backend()
    gq, gk, gv, gdo, gP, gdR = (t.cuda() for t in (q, k, v, dout, P, dR))
    gdS = torch.full((B, H, S, S), float("nan"), device="cuda")
    gdM = torch.full((B, S, S), float("nan"), device="cuda")
    be.attn_bwd_front(gv, gdo, gP, gdS, gdM, B, S, S, H, hd)

    def back(mode):
        o = {n: Guarded(B, S, D) for n in NAMES}
        prev = be.attn_set_option(be.ATTN_OPT_BACK, mode)
        try:
            be.attn_bwd_back(gq, gk, gdo, gP, gdS, gdR, o["dq"].t, o["dk"].t, o["dv"].t, B, S, S, H, hd)
        finally:
            be.attn_set_option(be.ATTN_OPT_BACK, prev)
        return o

    runs = {"stripe": back(be.ATTN_BACK_STRIPE), "ring": back(be.ATTN_BACK_RING), "ring2": back(be.ATTN_BACK_RING)}
    torch.cuda.synchronize()
    return ref, runs


@pytest.mark.parametrize("B,S,H,hd", SHAPES)
def test_ring_and_stripe_agree_bit_for_bit_and_match_float64(B, S, H, hd):
    assert calm.backend.get_backend().attn_fwd_supported(S, S, H, hd)
    ref, runs = _case(B, S, H, hd)
    for form in ("stripe", "ring", "ring2"):
        for name in NAMES:
            out = runs[form][name]
            assert not torch.isnan(out.t).any(), (form, name)     # every element of the NaN-filled output was written
            assert out.guards_untouched(), (form, name)           # ... and nothing outside it
            err = rel_err(out.t, ref[name])
            print(f"back {form} {B}x{S}x{H}x{hd} {name}: {err:.3e}")
            assert err < TOL, (form, name)
    for name in NAMES:
        assert torch.equal(runs["ring"][name].t, runs["stripe"][name].t), name    # the same MFMA chains in the same order
        assert torch.equal(runs["ring2"][name].t, runs["ring"][name].t), name     # and the ring repeats itself


def test_set_option_returns_the_previous_value_and_refuses_unknown_ones():
    be = calm.backend.get_backend()
    prev = be.attn_set_option(be.ATTN_OPT_BACK, be.ATTN_BACK_RING)
    try:
        assert prev == be.ATTN_BACK_TABLE                         # the default
        assert be.attn_set_option(be.ATTN_OPT_BACK, be.ATTN_BACK_STRIPE) == be.ATTN_BACK_RING
        with pytest.raises(ValueError):
            be.attn_set_option(be.ATTN_OPT_BACK, 3)
        with pytest.raises(ValueError):
            be.attn_set_option(1, be.ATTN_BACK_RING)
        assert be.attn_set_option(be.ATTN_OPT_BACK, be.ATTN_BACK_TABLE) == be.ATTN_BACK_STRIPE   # refused calls changed nothing
    finally:
        be.attn_set_option(be.ATTN_OPT_BACK, prev)
