"""calm_dropout on the MI355X: the kernel against the numpy emulation bit for bit (every vector / tail / unaligned path,
all four high words of counter and key in use, NaN / inf), the two reference-minted block fixtures on the HIP path, the
bf16 pipeline against the emulation of its rounding points, eval() bit-identity, reproducibility under torch.manual_seed
and replays of a captured graph drawing new keys."""
import math

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import weights as W
from emulated_dropout import EmulatedDropoutBackend, keep_mask
from make_golden_dropout import DROPOUT_BLOCKS
from test_dropout_cpu import check_against_fixture, run_dropout_fixture
from helpers import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-3                          # the project's fp32 bound (TOL of test_model_gpu.py)
BF16_VS_EMULATION_BLOCK = 3e-3      # as in test_realsize_gpu.py: one block against the emulation of the same rounding points
SEED, OFFSET, E0 = 0x0123456789ABCDEF, (1 << 32) + 7, 1 << 34
SIZES = (1, 3, 4, 5, 8, 9, 31, 1024, 4099, 65541)
# name -> (dtype, with residual, in place)
COMBOS = {"f32_to_f32": (torch.float32, False, False), "f32_res_to_f32": (torch.float32, True, False),
          "bf16_in_place": (torch.bfloat16, False, True), "f32_in_place": (torch.float32, False, True)}


@pytest.fixture(autouse=True)
def _restore():
    yield
    calm.backend.set_matmul_precision("fp32")
    calm.ops.set_noise_override(None)
    calm.ops.set_dropout_key_override(None)


def _bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _assert_same_bits(got, ref, what):
    """Equal as integers; where the reference is NaN the result must be NaN (IEEE 754 fixes neither sign nor payload of a
    generated NaN: inf * 0 is 0x7FC00000 on gfx950 and 0xFFC00000 on an x86 host)."""
    got, ref = got.cpu(), ref.cpu()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), what
    assert torch.equal(_bits(got)[~nan], _bits(ref)[~nan]), what


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("combo", list(COMBOS))
def test_kernel_matches_the_emulation_bit_for_bit(combo, p):
    dtype, with_res, in_place = COMBOS[combo]
    be, emu = calm.backend.get_backend(), EmulatedDropoutBackend()
    key = torch.tensor([SEED, OFFSET], dtype=torch.int64, device="cuda")
    lead = 4 // torch.empty(0, dtype=dtype).element_size()            # elements in 4 bytes: the unaligned base
    for n in SIZES:
        keep = keep_mask(SEED, OFFSET, E0, n, p)
        x = torch.from_numpy(W.make_input((n,), n, "x")).to(dtype)
        # one NaN and one inf on a dropped and on a kept position (where the mask has such positions left)
        kept, dropped = np.flatnonzero(keep), np.flatnonzero(~keep)
        for idx, val in ((kept[:1], float("nan")), (kept[1:2], float("inf")), (dropped[:1], float("nan")),
                         (dropped[1:2], float("-inf"))):
            x[torch.from_numpy(idx)] = val
        r = torch.from_numpy(W.make_input((n,), n, "r")) if with_res else None
        ref = torch.empty(n, dtype=dtype)
        emu.dropout(x, r, ref, n, p, (SEED, OFFSET), e0=E0)
        if p > 0 and n >= 31:
            assert torch.isnan(ref[torch.from_numpy(dropped[:2])]).all()           # a dropped NaN / inf is NaN, not 0
            assert (ref[torch.from_numpy(dropped[2:])] == (r[torch.from_numpy(dropped[2:])] if with_res else 0)).all()
        for off in (0, lead):                                        # 16-byte aligned bases, then bases 4 bytes further on
            xs = torch.zeros(n + off, dtype=dtype, device="cuda")[off:].copy_(x)
            rs = torch.zeros(n + off, device="cuda")[off:].copy_(r) if with_res else None
            ys = xs if in_place else torch.full((n + off + 8,), 7.0, dtype=dtype, device="cuda")[off:off + n]
            assert xs.data_ptr() % 16 == (4 if off else 0)
            be.dropout(xs, rs, ys, n, p, key, e0=E0)
            _assert_same_bits(ys, ref, (combo, p, n, off))
            if not in_place:                                         # nothing written past the n-th element
                whole = torch.as_strided(ys, (n + 8,), (1,))
                assert (whole[n:] == 7.0).all(), (combo, p, n, off)


def test_mask_does_not_depend_on_storage_type_or_split():
    """The same (seed, offset, e) gives the same decision in fp32 and bf16, and two calls that cover one logical tensor
    (the second with e0 advanced by a multiple of 4) give what one call gives."""
    be = calm.backend.get_backend()
    key = torch.tensor([SEED, OFFSET], dtype=torch.int64, device="cuda")
    n, p = 4099, 0.5
    x = torch.ones(n, device="cuda")
    y32, y16 = torch.empty_like(x), torch.empty(n, dtype=torch.bfloat16, device="cuda")
    be.dropout(x, None, y32, n, p, key, e0=E0)
    be.dropout(x.bfloat16(), None, y16, n, p, key, e0=E0)
    assert torch.equal(y32 == 0, y16 == 0)
    assert torch.equal((y32 != 0).cpu(), torch.from_numpy(keep_mask(SEED, OFFSET, E0, n, p)))
    y2 = torch.empty_like(x)
    be.dropout(x[:1028], None, y2[:1028], 1028, p, key, e0=E0)
    be.dropout(x[1028:], None, y2[1028:], n - 1028, p, key, e0=E0 + 1028)
    assert torch.equal(y2, y32)


@pytest.mark.parametrize("name", list(DROPOUT_BLOCKS))
def test_block_with_dropout_fp32_matches_reference_fixture(name):
    out = run_dropout_fixture(name, "fp32", "cuda")
    check_against_fixture(*out, tol=TOL, label=f"{name} HIP fp32")


def test_block_with_dropout_bf16_pipeline_against_emulation():
    g, kw, blk, y, kl, xq, xkv = run_dropout_fixture("A", "bf16", "cuda")
    with calm.backend.use_backend(EmulatedDropoutBackend()):
        _, _, blk_e, y_e, kl_e, xq_e, _ = run_dropout_fixture("A", "bf16", "cpu")
    ey, edx = rel_err(y, y_e), rel_err(xq.grad, xq_e.grad)
    print(f"\n[A bf16 pipeline vs emulation] y {ey:.2e} dxq {edx:.2e}")
    assert ey < BF16_VS_EMULATION_BLOCK
    assert edx < 6 * BF16_VS_EMULATION_BLOCK


def _fresh_block(kw, dropout):
    vt = calm.Vi_Tools_CNN_less_V2
    blk = vt.VMLA_Block(mlp_dim=2 * kw["dim2"], force_reduce=False, dropout=dropout, **kw)
    shapes = {k: tuple(v.shape) for k, v in blk.state_dict().items()}
    blk.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_params(shapes, 77).items()})
    return blk.cuda()


def test_eval_mode_is_bit_identical_to_a_block_without_dropout():
    kw = DROPOUT_BLOCKS["A"]["kw"]
    a, b = _fresh_block(kw, 0.25).eval(), _fresh_block(kw, 0.0).eval()
    b.load_state_dict(a.state_dict())
    x = torch.from_numpy(W.make_input((2, kw["seq_length"], kw["dim1"]), 5, "xq")).cuda()
    with torch.no_grad():
        assert torch.equal(a(x, mask=True), b(x, mask=True))


def test_training_repeats_under_one_seed_and_differs_under_another():
    """Default key source and default latent noise (torch's device generator): the reducing cross block draws both."""
    vt = calm.Vi_Tools_CNN_less_V2
    kw = DROPOUT_BLOCKS["B"]["kw"]
    blk = _fresh_block(kw, 0.1).train()
    state = {k: v.clone() for k, v in blk.state_dict().items()}
    xq0 = torch.from_numpy(W.make_input((2, kw["seq_length"], kw["dim1"]), 5, "xq")).cuda()
    xkv0 = torch.from_numpy(W.make_input((2, kw["seq_length"], kw["dim1"]), 6, "xkv")).cuda()
    be = calm.backend.get_backend()
    prev = be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, 1)          # weight gradients without atomics: every bit compares
    runs = []
    try:
        for seed in (11, 11, 12):
            blk.load_state_dict(state)                               # the training forward advances u, v
            for prm in blk.parameters():
                prm.grad = None
            xq, xkv = xq0.clone().requires_grad_(True), xkv0.clone().requires_grad_(True)
            torch.manual_seed(seed)
            y = blk(xq, input_kv=xkv, state_manager=vt.ResidualStateManager(mode="sum"), mask=True)
            (y * y).sum().backward()
            runs.append((y.detach().clone(), xq.grad.clone(), xkv.grad.clone(),
                         {n: prm.grad.clone() for n, prm in blk.named_parameters()}))
    finally:
        be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, prev)
    a, b, c = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert not [n for n in a[3] if not torch.equal(a[3][n], b[3][n])]
    assert not torch.equal(a[0], c[0])


def test_captured_graph_draws_a_new_mask_on_every_replay():
    n, p = 4096, 0.5
    x = torch.from_numpy(W.make_input((n,), 1, "x")).abs().add(1.0).cuda()          # no zero in the input ...
    res = torch.zeros(n, device="cuda")                                             # ... so a zero in y is a dropped element
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                   # warm-up outside the capture
        calm.ops.DropoutAddFn.apply(x, res, p, calm.ops.draw_dropout_key(x.device))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = calm.ops.DropoutAddFn.apply(x, res, p, calm.ops.draw_dropout_key(x.device))
    patterns = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        patterns.append((y == 0).cpu())
        kept = ~patterns[-1]
        assert torch.equal(y.cpu()[kept], (x.cpu() * 2.0)[kept])
    assert not torch.equal(patterns[0], patterns[1])
    for z in patterns:
        assert abs(float(z.float().mean()) - p) < 4 * math.sqrt(p * (1 - p) / n)
