"""64-row fp32 GEMM tiles (gemm_f32_t64_kernel: 64 x 16 nb on v_mfma_f32_16x16x4_f32) against float64 products.
Every case first asks calm_gemm_describe that the launch really plans the 64-row tile (family 0, tile_m 64), and C sits
inside a NaN-filled guard band: every element of C must be written and nothing around it.  The products are exact
fp32 multiplies accumulated in fp32, so the tolerance is fp32 rounding: 2e-6 x sqrt(K / 1024) of the largest output
(x4 with the epilogue operands).  The fp32 pipe takes no bf16 tensor (the dispatcher refuses one), so C is fp32 here."""
import pytest
import torch

import calm_vit_dte_amd as calm
from gemm_f64 import GUARD_ROWS, Guarded      # C inside a NaN-filled guard band: shared with the per-instance checker
from helpers import rel_err

pytestmark = pytest.mark.gpu


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _operand(rows, K, batch, kcontig, seed):
    b0, b1 = batch
    if kcontig:
        return rnd(b0, b1, rows, K, seed=seed), (K, 1, b1 * rows * K, rows * K)
    return rnd(b0, b1, K, rows, seed=seed), (1, rows, b1 * rows * K, rows * K)


def _product(A, B, akc, bkc):
    a = A.double() if akc else A.double().transpose(-1, -2)
    b = B.double() if bkc else B.double().transpose(-1, -2)
    return a @ b.transpose(-1, -2)


def _plan64(hip, *args, **kw):
    plan = hip.gemm_describe(*args, **kw)
    assert plan["family"] == 0 and plan["tile_m"] == 64 and plan["tile_n"] % 16 == 0, plan
    return plan


CASES = [
    # M, N, K, batch, a_kcontig, b_kcontig
    (40, 528, 176, (64, 1), True, False),       # the M = 40 mode-B latent products: 16-row strips, N = 11 x 48
    (80, 240, 80, (32, 1), False, False),       # per-image 80 x 240 x 80
    (176, 528, 176, (16, 1), True, False),
    (224, 112, 224, (4, 6), False, False),      # per-image, per-head: both batch strides
    (176, 40, 120, (32, 1), True, True),        # N = 40, K tail of 8
    (4000, 240, 240, (1, 1), True, True),       # large-M, narrow and short; ragged M
    (4000, 120, 264, (1, 1), True, False),      # N = 120, K tail of 8
    (2056, 80, 164, (1, 1), False, True),       # row-contiguous A with k-contiguous B, K tail of 4
    (1000, 112, 72, (2, 3), True, True),        # batches, ragged M
    (1000, 240, 75, (1, 1), True, True),        # K odd: one-element staging
    (302, 120, 96, (8, 1), False, False),       # M % 4 != 0 with row-contiguous A: one-element staging
]


@pytest.mark.parametrize("M,N,K,batch,akc,bkc", CASES)
@pytest.mark.parametrize("epi", ["plain", "gelu_bwd", "gelu_pre", "accumulate", "unaligned"])
def test_tile64_gemm_against_float64(M, N, K, batch, akc, bkc, epi):
    hip = calm.backend.get_backend()
    b0, b1 = batch
    A, a = _operand(M, K, batch, akc, 1)
    B, b = _operand(N, K, batch, bkc, 2)
    ref = _product(A, B, akc, bkc)
    tol = 2e-6 * max(1.0, (K / 1024) ** 0.5)
    c0 = rnd(b0, b1, M, N, seed=7)
    C = Guarded(b0, b1, M, N, shift=1 if epi == "unaligned" else 0, init=c0 if epi == "accumulate" else None)
    kw = dict(batch=batch, split_k=1)
    pre = None
    if epi in ("gelu_bwd", "unaligned"):
        bias, cs, res, aux = rnd(N, seed=3), rnd(N, seed=4), rnd(b0, b1, M, N, seed=5), rnd(b0, b1, M, N, seed=6)
        AUX = Guarded(b0, b1, M, N, shift=1 if epi == "unaligned" else 0, init=aux.cuda())   # aux has C's strides
        kw.update(alpha=0.5, inv_scale=torch.tensor([1.3]).cuda(), bias=bias.cuda(), col_scale=cs.cuda(),
                  residual=res.cuda(), r=(N, b1 * M * N, M * N), act=2, aux=AUX.buf[GUARD_ROWS * AUX.ld + 4 + (epi == "unaligned"):])
        x = aux.double()
        gelu_grad = 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-x * x / 2) / (2 * torch.pi) ** 0.5
        ref = ((ref * (0.5 / 1.3) + bias.double()) * gelu_grad) * cs.double() + res.double()
        tol *= 4
    elif epi == "gelu_pre":
        bias = rnd(N, seed=3)
        pre = Guarded(b0, b1, M, N)
        kw.update(bias=bias.cuda(), act=1, C_pre=pre.buf[GUARD_ROWS * pre.ld + 4:])
        ref = ref + bias.double()
    elif epi == "accumulate":
        kw.update(accumulate=True)
        ref = ref + c0.double()
    args = (A.cuda(), B.cuda(), C.buf[GUARD_ROWS * C.ld + 4 + (epi == "unaligned"):], M, N, K, a, b, C.strides)
    _plan64(hip, *args, **kw)
    hip.gemm(*args, **kw)
    got = C.check()
    if epi == "gelu_pre":
        assert rel_err(pre.check(), ref) < tol
        ref = torch.nn.functional.gelu(ref)
    assert rel_err(got, ref) < tol


def _wgrad(M, N, K, seed=1):
    """weight-gradient layout (both operands row-contiguous): G = dY^T X over K tokens"""
    return rnd(K, M, seed=seed), rnd(K, N, seed=seed + 1), (1, M, 0, 0), (1, N, 0, 0)


@pytest.mark.parametrize("M,N,K", [(240, 240, 20480), (80, 160, 20480), (192, 120, 32768)])
@pytest.mark.parametrize("deterministic", [0, 1])
def test_tile64_split_k_atomics_and_workspace(M, N, K, deterministic):
    """k-split weight gradients: fp32 atomics onto a zeroed C, or (deterministic mode) per-slice partial tiles in the
    workspace + the fixed-order reduction — then bitwise equal across repeats."""
    hip = calm.backend.get_backend()
    dy, x, a, b = _wgrad(M, N, K)
    ref = dy.double().T @ x.double()
    prev = hip.gemm_set_option(hip.GEMM_OPT_DETERMINISTIC, deterministic)
    try:
        outs = []
        for _ in range(2 if deterministic else 1):
            C = Guarded(1, 1, M, N)
            args = (dy.cuda(), x.cuda(), C.buf[GUARD_ROWS * C.ld + 4:], M, N, K, a, b, C.strides)
            plan = _plan64(hip, *args)
            assert plan["k_slices"] > 1, plan
            hip.gemm(*args)
            outs.append(C.check())
    finally:
        hip.gemm_set_option(hip.GEMM_OPT_DETERMINISTIC, prev)
    assert rel_err(outs[0], ref[None, None]) < 2e-6 * (K / 1024) ** 0.5
    if deterministic:
        assert torch.equal(outs[0], outs[1])


def test_tile64_batch_reduced_sum():
    """reduce_batch: C = sum_b A_b B_b^T (the per-image products summed into one weight gradient), k-slices over the
    concatenated reduction combined with atomics"""
    hip = calm.backend.get_backend()
    S2, S, D, nb = 80, 240, 128, 64
    dy, x = rnd(nb, S2, D, seed=1), rnd(nb, S, D, seed=2)
    ref = torch.einsum("bik,bjk->ij", dy.double(), x.double())
    C = Guarded(1, 1, S2, S)
    args = (dy.cuda(), x.cuda(), C.buf[GUARD_ROWS * C.ld + 4:], S2, S, D, (D, 1, S2 * D, 0), (D, 1, S * D, 0), C.strides)
    _plan64(hip, *args, batch=(nb, 1), reduce_batch=True)
    hip.gemm(*args, batch=(nb, 1), reduce_batch=True)
    assert rel_err(C.check()[0, 0], ref) < 2e-6 * (D * nb / 1024) ** 0.5


def test_tile64_grouped_projections_input_and_weight_gradients():
    """Grouped launches: three projections of one activation (per-group sigma), their input gradient as one pass over the
    concatenated reduction (accumulators re-scaled at the group boundaries), and their weight gradients k-split per group."""
    hip = calm.backend.get_backend()
    M, D = 4000, 240
    x = rnd(M, D, seed=1).cuda()
    ws = [(rnd(D, D, seed=10 + i) * D ** -0.5).cuda() for i in range(3)]
    sig = [1.0 + 0.3 * i for i in range(3)]
    sg = [torch.tensor([s], device="cuda") for s in sig]
    lin = (D, 1, 0, 0)
    outs = [Guarded(1, 1, M, D) for _ in range(3)]
    views = [o.buf[GUARD_ROWS * o.ld + 4:] for o in outs]
    c = outs[0].strides
    _plan64(hip, x, ws, views, M, D, D, lin, lin, c, batch=(3, 1), inv_scale=sg, split_k=1)
    hip.gemm(x, ws, views, M, D, D, lin, lin, c, batch=(3, 1), inv_scale=sg, split_k=1)
    for i in range(3):
        assert rel_err(outs[i].check()[0, 0], (x.double() @ ws[i].double().T).cpu() / sig[i]) < 2e-6

    dys = [rnd(M, D, seed=20 + i).cuda() for i in range(3)]
    dx = Guarded(1, 1, M, D)
    args = (dys, ws, dx.buf[GUARD_ROWS * dx.ld + 4:], M, D, D, lin, (1, D, 0, 0), dx.strides)
    _plan64(hip, *args, batch=(3, 1), inv_scale=sg, reduce_batch=True, split_k=1)
    hip.gemm(*args, batch=(3, 1), inv_scale=sg, reduce_batch=True, split_k=1)
    ref = sum(dys[i].double() @ ws[i].double() / sig[i] for i in range(3))
    assert rel_err(dx.check()[0, 0], ref.cpu()) < 4e-6

    Gs = [Guarded(1, 1, D, D) for _ in range(3)]
    gv = [g.buf[GUARD_ROWS * g.ld + 4:] for g in Gs]
    args = (dys, x, gv, D, D, M, (1, D, 0, 0), (1, D, 0, 0), Gs[0].strides)
    plan = _plan64(hip, *args, batch=(3, 1))
    assert plan["k_slices"] > 1, plan
    hip.gemm(*args, batch=(3, 1))
    for i in range(3):
        assert rel_err(Gs[i].check()[0, 0], (dys[i].double().T @ x.double()).cpu()) < 2e-6 * (M / 1024) ** 0.5


def test_tile64_propagates_nan():
    hip = calm.backend.get_backend()
    M, N, K, nb = 80, 240, 80, 16
    A, B = rnd(nb, M, K, seed=1), rnd(nb, N, K, seed=2)
    A[3, 17, 74] = float("nan")
    C = torch.zeros(nb, M, N, device="cuda")
    args = (A.cuda(), B.cuda(), C, M, N, K, (K, 1, M * K, 0), (K, 1, N * K, 0), (N, M * N, 0))
    _plan64(hip, *args, batch=(nb, 1), split_k=1)
    hip.gemm(*args, batch=(nb, 1), split_k=1)
    bad = torch.isnan(C)
    assert bad[3, 17].all() and int(bad.sum()) == N
