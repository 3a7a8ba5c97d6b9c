"""calm_attention16_fwd / calm_attention16_bwd (csrc/attention_bf16.hip and its two headers) against the staged
float64 reference of tests/attn16_f64.py, at one shape per compiled (NP, HDP) instance — all 48 — plus the smallest and
largest legal shapes, the shapes on either side of the pipelined / register-staged dispatch boundary, other head counts
and batch sizes (the XCD-paired order at B % 8 == 0 and a ragged B = 9), and the register-staged kernels of the 14
pipelined-capable instances in a child process.  The only reference is float64 torch on the CPU: the emulation is not
imported here.  Bounds are element-wise and derived in attn16_f64.py; none is a normalised max-norm.

Memory: every output is the interior of a guard buffer (Out of test_rowwise_f64_gpu.py: guards and interior prefilled
with a payload NaN; guards must be unchanged, every interior element written).  Every input sits between NaN fences
(a multiple of 8 bf16 / 4 fp32 elements, so bases stay 16-byte aligned): a read past a tensor's end that reaches
arithmetic shows as a NaN in an output, and every output is asserted finite by its bound.

Worst error / bound per output on an MI355X over every case of this file (87 runs of forward + backward, both kernel
generations), recorded from the run that accompanied this file — the assertions do not depend on these figures:
    out 0.83   dq 0.83   dk 0.90   dv 0.87        (bf16 outputs of a product with a bf16-rounded operand)
    lse 0.10   delta 0.075                        (fp32 outputs)
    R, hp, hg, Mk, dM: every element within one bf16 ulp of the rounded reference; of the counted elements (fp32
    bound <= 1/32 ulp) at least 99.9 % equal it (lowest share: hp 0.9990, R / Mk 0.9997, hg / dM 0.9998; the floor
    is 0.99).  The counted share of a tensor falls with S (the bound grows with the dot length): Mk 0.1 %..100 %,
    hg 1.7 %..98 %, dM 26 %..99 %.
Wall time of the file: 11 s, 5 s of it the child process.

Found by this file: with D = H hd % 8 == 4 the pipelined forward's phase 1 (whole rows of q and k as 16-byte chunks on
both sides of R = q k^T) read four elements past every row, at the last row of the tensor past its end — the NaN fence
turned R, and everything after it, of the last image into NaN.  launch_fwd16_t now sends those shapes to the
register-staged forward; the cases stay here as the regression test.
"""
import os
import subprocess
import sys

import pytest
import torch

import calm_vit_dte_amd as calm
import attn16_f64 as A
from test_rowwise_f64_gpu import Out

pytestmark = pytest.mark.gpu

DEV = "cuda"
FENCE = 64                          # elements before and after every input: 128 bytes of bf16, 256 of fp32
SWEEP = A.sweep_cases()
B_SWEEP, H_SWEEP = 2, 3             # H odd: with hd % 8 == 4 the last row of the last image starts at an address that
                                    # is only 8-byte aligned and ends at the tensor's end
HEADS = [(176, 1, 44), (176, 12, 44), (288, 1, 72), (288, 12, 72)]      # pipelined / register-staged instance
BATCHES = [(B, S, hd) for S, hd in ((176, 44), (288, 72)) for B in (1, 9, 16)]
# the register-staged kernels of the pipelined-capable instances (CALM_ATTN16_V2=0 CALM_ATTN16_BWD2=0), and the extras
# on and just past the dispatch boundary
FALLBACK_SWEEP = [c for c in SWEEP if A.pipelined_capable(*c)]
FALLBACK_EXTRA = [(8, 4), (32, 32), (64, 64), (224, 64), (232, 64), (224, 68)]


@pytest.fixture(scope="module")
def hip():
    return calm.backend.get_backend()


def fenced(t):
    """Device copy of t with FENCE NaN elements of its dtype before and after it in the same allocation."""
    buf = torch.full((2 * FENCE + t.numel(),), float("nan"), dtype=t.dtype, device=DEV)
    view = buf[FENCE:FENCE + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return view


def run_forward(hip, ins, B, S, H, hd):
    """-> (dict of CPU outputs, dict of the device tensors the backward consumes); guards checked"""
    D = H * hd
    bf = torch.bfloat16
    outs = dict(out=Out((B, S, D), bf), R=Out((B, S, S), bf), hp=Out((B, S, 2 * S), bf), hg=Out((B, S, 2 * S), bf),
                Mk=Out((B, S, S), bf), MkT=Out((B, S, S), bf), lse=Out((B, H, S)))
    dev_ins = [fenced(t) if t.numel() > 1 else t.to(DEV) for t in ins]
    hip.attn16_fwd(*dev_ins, *[outs[n].t for n in A.FWD_NAMES], B, S, H, hd)
    torch.cuda.synchronize()
    got = {n: o.check() for n, o in outs.items()}
    return got, dev_ins


def run_backward(hip, dev_ins, got, dout, B, S, H, hd):
    D = H * hd
    bf = torch.bfloat16
    outs = dict(delta=Out((B, H, S)), dq=Out((B, S, D), bf), dk=Out((B, S, D), bf), dv=Out((B, S, D), bf),
                dM=Out((B, S, S), bf))
    q, k, v = dev_ins[:3]
    saved = [fenced(got[n]) for n in ("out", "Mk", "MkT", "lse")]
    hip.attn16_bwd(q, k, v, saved[0], fenced(dout), saved[1], saved[2], saved[3], *[outs[n].t for n in A.BWD_NAMES],
                   B, S, H, hd)
    torch.cuda.synchronize()
    return {n: o.check() for n, o in outs.items()}


def _report(tag, worst):
    print(f"attn16_f64 {tag} " + " ".join(f"{k}={v:.4g}" for k, v in sorted(worst.items())))


def forward_backward(hip, B, S, H, hd, seed=None):
    assert hip.attn16_supported(S, H, hd)
    ins, dout = A.make_inputs(B, S, H, hd, seed=S + hd if seed is None else seed)
    got, dev_ins = run_forward(hip, ins, B, S, H, hd)
    wf, _ = A.check_forward(ins, got, B, S, H, hd)
    bw = run_backward(hip, dev_ins, got, dout, B, S, H, hd)          # the backward consumes this forward's tensors
    wb, _ = A.check_backward(ins, got, dout, bw, B, S, H, hd)
    _report(f"B={B} S={S} H={H} hd={hd}", {**wf, **wb})


@pytest.mark.parametrize("S,hd", SWEEP, ids=[f"{S}-{hd}" for S, hd in SWEEP])
def test_attention16_instance_sweep(hip, S, hd):
    """One ragged shape per compiled (NP, HDP) instance, forward then backward.  Under CALM_ATTN16_V2=0 /
    CALM_ATTN16_BWD2=0 (the child of the fallback test below) the same node ids run the register-staged kernels."""
    forward_backward(hip, B_SWEEP, S, H_SWEEP, hd)


STRADDLE = [c for c in SWEEP + [(8, 4)] if A.pipelined_capable(*c) and c[1] % 8 == 4]


@pytest.mark.parametrize("S,hd", STRADDLE, ids=[f"{S}-{hd}" for S, hd in STRADDLE])
def test_attention16_pipelined_forward_with_straddling_heads(hip, S, hd):
    """hd % 8 == 4 at the pipelined-capable instances with H = 4: D = H hd is a multiple of 8, which is what the
    pipelined forward needs (launch_fwd16_t sends D % 8 == 4 — the sweep's H = 3 at these head dims — to the
    register-staged forward: phase 1 of the pipelined one stages whole rows of D columns as 16-byte chunks).  Here its
    per-head 16-byte chunks straddle two heads and the last one ends at the tensor's end."""
    assert (4 * hd) % 8 == 0
    forward_backward(hip, B_SWEEP, S, 4, hd)


@pytest.mark.parametrize("S,hd", A.EXTRA_SHAPES, ids=[f"{S}-{hd}" for S, hd in A.EXTRA_SHAPES])
def test_attention16_extra_shapes(hip, S, hd):
    """Smallest and largest legal shape, full (unpadded) tiles, and S = 224 / 232, hd = 64 / 68: the last pipelined
    shape and the first register-staged one in either direction."""
    forward_backward(hip, B_SWEEP, S, H_SWEEP, hd)


@pytest.mark.parametrize("S,H,hd", HEADS)
def test_attention16_head_counts(hip, S, H, hd):
    forward_backward(hip, 2, S, H, hd)


@pytest.mark.parametrize("B,S,hd", BATCHES)
def test_attention16_batch_orders(hip, B, S, hd):
    """B = 16 takes the XCD-paired workgroup order, B = 9 the plain order with a ragged last group, B = 1 one image."""
    forward_backward(hip, B, S, 3, hd)


def test_attention16_register_staged_kernels_of_the_pipelined_instances_in_a_child_process():
    """CALM_ATTN16_V2=0 CALM_ATTN16_BWD2=0 (read once per process, hence a fresh child; one child, no retry): the 14
    instances with NP <= 7 and HDP <= 64 and the boundary extras again.  Which generation ran cannot be observed from
    Python: that the child runs attn16_fwd_kernel / attn16_bwd_q_kernel / attn16_bwd_kv_kernel follows from the
    dispatch rule in launch_fwd16_t / launch_bwd16_t (k1 and kq stay null when the switch is off)."""
    assert len(FALLBACK_SWEEP) == 14
    here = os.path.abspath(__file__)
    nodes = [f"{here}::test_attention16_instance_sweep[{S}-{hd}]" for S, hd in FALLBACK_SWEEP] + \
            [f"{here}::test_attention16_extra_shapes[{S}-{hd}]" for S, hd in FALLBACK_EXTRA]
    env = dict(os.environ, CALM_ATTN16_V2="0", CALM_ATTN16_BWD2="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x"] + nodes, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and f"{len(nodes)} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


def test_attention16_supported_is_the_header_rule(hip):
    """include/calm_vit.h: every shape with S % 8 == 0, S <= 384, hd % 4 == 0, hd <= 128 is supported.  Host only.
    (calm_attention16_supported consults the register-staged forward's LDS size only, not the backward geometries:
    that a supported answer is never followed by CALM_E_UNSUPP is what the sweep shows, fwd and bwd, at its cases.)"""
    wrong = [(S, H, hd) for S in range(1, 401) for hd in range(1, 137) for H in (1, 12)
             if hip.attn16_supported(S, H, hd) != (S % 8 == 0 and S <= 384 and hd % 4 == 0 and hd <= 128)]
    assert not wrong, wrong[:10]
    assert not hip.attn16_supported(0, 1, 4) and not hip.attn16_supported(8, 0, 4) and not hip.attn16_supported(8, 1, 0)


@pytest.mark.parametrize("S,hd", [(176, 44), (288, 72)])
def test_attention16_non_finite_values_propagate(hip, S, hd):
    """The header's "NaN/Inf propagate", one cause per image so that each effect has one possible source.
    Image 0: a NaN in one q element reaches that query row of R, hp, hg, Mk (the mask is shared: every head), out, lse
    and dq; every other row of the forward stays finite.
    Image 1: no NaN anywhere; an inf in one dout element (row i1, head h1, column d1).  Its forward is finite and
    inside every bound.  dv[:, h1, d1] = sum_i P[i, j] dO[i, d1] is non-finite for every key j, and the other columns
    and heads of dv stay finite.  delta[h1, i1] is infinite, so dS[i1, :] of head h1 is, and with it dk of head h1
    (every key), dq[i1] of head h1 and dM[i1, :]; dk and dq of the other heads and every other row of dM stay finite.
    Image 2: untouched, inside every bound forward and backward."""
    B, H = 3, 3
    i0, i1, h1, d1 = 5, S - 3, 1, hd - 1
    ins, dout = A.make_inputs(B, S, H, hd, seed=11)
    ins[0][0, i0, 2 * hd + 1] = float("nan")
    dout[1, i1, h1 * hd + d1] = float("inf")
    got, dev_ins = run_forward(hip, ins, B, S, H, hd)
    fin = lambda t: torch.isfinite(t.float())
    rest = [i for i in range(S) if i != i0]
    for n in ("R", "hp", "hg", "Mk", "out"):
        assert torch.isnan(got[n][0, i0].float()).all(), n
        assert fin(got[n][0, rest]).all(), n
    assert torch.isnan(got["lse"][0, :, i0]).all() and fin(got["lse"][0][:, rest]).all()
    bw = run_backward(hip, dev_ins, got, dout, B, S, H, hd)
    assert not fin(bw["dq"][0, i0]).any()
    # image 1: the inf alone
    head = slice(h1 * hd, (h1 + 1) * hd)
    others = [c for c in range(H * hd) if not h1 * hd <= c < (h1 + 1) * hd]
    assert all(fin(got[n][1]).all() for n in A.FWD_NAMES)
    dv, dk, dq, dM, delta = (bw[n][1] for n in ("dv", "dk", "dq", "dM", "delta"))
    assert not fin(dv[:, h1 * hd + d1]).any()
    assert fin(dv[:, [c for c in range(H * hd) if c != h1 * hd + d1]]).all()
    assert not fin(dk[:, head]).any() and fin(dk[:, others]).all()
    assert not fin(dq[i1, head]).any() and fin(dq[i1, others]).all()
    assert fin(dq[[i for i in range(S) if i != i1]]).all()
    assert not fin(dM[i1]).any() and fin(dM[[i for i in range(S) if i != i1]]).all()
    assert not fin(delta[h1, i1]) and int((~fin(delta)).sum()) == 1
    # images 1 (forward) and 2 (forward and backward) against the bounds
    one = lambda t, b: t[b:b + 1] if t.dim() == 3 and t.shape[0] == B else t
    for b in (1, 2):
        ins_b = tuple(one(t, b) for t in ins)
        got_b = {n: t[b:b + 1] for n, t in got.items()}
        A.check_forward(ins_b, got_b, 1, S, H, hd)
        if b == 2:
            A.check_backward(ins_b, got_b, dout[b:b + 1], {n: t[b:b + 1] for n, t in bw.items()}, 1, S, H, hd)


def test_attention16_every_compiled_instance_is_reached():
    """The sweep's ids cover the 48 (NP, HDP) pairs of with_shape16, the child's list the 14 pipelined-capable ones."""
    every = {(NP, HDP) for NP in range(1, 13) for HDP in (32, 64, 96, 128)}
    assert {A.instance_of(*c) for c in SWEEP} == every and len(SWEEP) == 48
    assert {A.instance_of(*c) for c in FALLBACK_SWEEP} == {i for i in every if i[0] <= 7 and i[1] <= 64}
    assert (8, 44) in SWEEP
