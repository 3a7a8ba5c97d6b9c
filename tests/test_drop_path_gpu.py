"""calm_drop_path on the MI355X: the kernel against the numpy emulation bit for bit (vector and element-wise kernels, a
strided grid, unaligned bases, the high words of seed, offset and sample0 in use, NaN / inf), VMLA_Block on the HIP path
against the same block on the emulated backend, eval() bit-identity, reproducibility under torch.manual_seed, replays of a
captured graph drawing new masks, and train(drop_path=) eager and captured against the loop that sets the rates itself."""
import math
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import weights as W
from emulated_drop_path import EmulatedDropPathBackend
from emulated_dropout import KeyStream, keep_mask
from helpers import CONFIGS, block_fixture_params, load_golden, rel_err
from make_golden_dropout import DROPOUT_BLOCKS
from test_drop_path_cpu import ALL_DROPPED, ALL_KEPT, MIXED, P, block_inputs, make_block, run_block
from test_host_logic_cpu import build_model

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
vt = calm.Vi_Tools_CNN_less_V2
TOL = 1e-3                          # the project's fp32 bound (TOL of test_model_gpu.py)
BF16_VS_EMULATION_BLOCK = 3e-3      # as in test_dropout_gpu.py: one block against the emulation of the same rounding points
SEED, OFFSET, SAMPLE0 = 0x0123456789ABCDEF, (1 << 32) + 7, (1 << 34) + 3
# (B, L): one element; a short odd row; fp32 rows off the 16-byte grid (element-wise kernel); a multiple of 4 but not of 8
# (vector kernel for fp32, element-wise for bf16); samples across three Philox groups; more than one chunk per row; 2052
# (sample, chunk) pairs of fp32 units, four more than the capped grid launches, with 684 chunks per row (the walk's carry);
# 2100 one-chunk rows, more than the capped grid for every storage type
SHAPES = ((1, 1), (1, 7), (5, 6), (5, 12), (9, 8), (4, 1032), (3, 700008), (2100, 8))
# name -> (x dtype, residual dtype or None, y dtype, in place)
F32, BF16 = torch.float32, torch.bfloat16
COMBOS = {"f32_to_f32": (F32, None, F32, False), "f32_res_to_f32": (F32, F32, F32, False),
          "bf16_in_place": (BF16, None, BF16, True), "f32_bf16res_to_bf16": (F32, BF16, BF16, False),
          "backward_f32_in_place": (F32, None, F32, True)}


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


def _shifted(t, lead, fill=0.0, tail=0):
    """`t` copied to the device at a base `lead` elements behind a 16-byte aligned one, `tail` guard elements behind it."""
    buf = torch.full((lead + t.numel() + tail,), fill, dtype=t.dtype, device="cuda")
    view = buf[lead:lead + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("combo", list(COMBOS))
def test_kernel_matches_the_emulation_bit_for_bit(combo, p):
    xt, rt, yt, in_place = COMBOS[combo]
    be, emu = calm.backend.get_backend(), EmulatedDropPathBackend()
    key = torch.tensor([SEED, OFFSET], dtype=torch.int64, device="cuda")
    for B, L in SHAPES:
        keep = keep_mask(SEED, OFFSET, SAMPLE0, B, p)
        x = torch.from_numpy(W.make_input((B, L), B + L, "x")).to(xt)
        # one NaN and one inf in a kept and in a dropped sample (where the mask has such samples and the row has room)
        kept, dropped = np.flatnonzero(keep), np.flatnonzero(~keep)
        for rows, vals in ((kept[:1], (float("nan"), float("inf"))), (dropped[:1], (float("nan"), float("-inf")))):
            for b in rows:
                x[b, 0], x[b, L - 1] = vals
        r = torch.from_numpy(W.make_input((B, L), B + L, "r")).to(rt) if rt is not None else None
        ref = torch.empty(B, L, dtype=yt)
        emu.drop_path(x, r, ref, B, L, p, (SEED, OFFSET), sample0=SAMPLE0)
        for b in dropped[:1]:
            assert torch.isnan(ref[b, 0]) and torch.isnan(ref[b, L - 1])         # a dropped NaN / inf is NaN, not 0
            if L > 2:
                assert torch.equal(ref[b, 1:L - 1].float(), (r[b, 1:L - 1].float() if r is not None else torch.zeros(L - 2)))
        for lead_bytes in (0, 4):                                    # 16-byte aligned bases, then bases 4 bytes further on
            lead = lambda dt: lead_bytes // torch.empty(0, dtype=dt).element_size()       # noqa: E731
            _, xs = _shifted(x, lead(xt))
            rs = _shifted(r, lead(rt))[1] if r is not None else None
            ybuf, ys = (None, xs) if in_place else _shifted(torch.empty(B, L, dtype=yt), lead(yt), fill=7.0, tail=8)
            assert xs.data_ptr() % 16 == lead_bytes and ys.data_ptr() % 16 == lead_bytes
            be.drop_path(xs, rs, ys, B, L, p, key, sample0=SAMPLE0)
            _assert_same_bits(ys, ref, (combo, p, B, L, lead_bytes))
            if not in_place:                                         # nothing written in front of or behind the B * L elements
                assert (ybuf[:lead(yt)] == 7.0).all() and (ybuf[lead(yt) + B * L:] == 7.0).all(), (combo, p, B, L, lead_bytes)


def test_mask_does_not_depend_on_storage_type_or_split():
    """The same (seed, offset, sample) gives the same decision in fp32 and bf16, for any row length, and two calls that cover
    one batch (the second with sample0 advanced by 3, no multiple of 4) give what one call gives."""
    be = calm.backend.get_backend()
    key = torch.tensor([SEED, OFFSET], dtype=torch.int64, device="cuda")
    B, L, p, cut = 203, 24, 0.5, 3
    x = torch.ones(B, L, device="cuda")
    y32, y16, y7 = torch.empty_like(x), torch.empty(B, L, dtype=torch.bfloat16, device="cuda"), torch.empty(B, 7, device="cuda")
    be.drop_path(x, None, y32, B, L, p, key, sample0=SAMPLE0)
    be.drop_path(x.bfloat16(), None, y16, B, L, p, key, sample0=SAMPLE0)
    be.drop_path(x[:, :7].contiguous(), None, y7, B, 7, p, key, sample0=SAMPLE0)
    keep = torch.from_numpy(keep_mask(SEED, OFFSET, SAMPLE0, B, p))
    for y in (y32, y16, y7):
        assert torch.equal((y != 0).all(dim=1).cpu(), keep) and torch.equal((y == 0).all(dim=1).cpu(), ~keep)
    y2 = torch.empty_like(x)
    be.drop_path(x[:cut], None, y2[:cut], cut, L, p, key, sample0=SAMPLE0)
    be.drop_path(x[cut:], None, y2[cut:], B - cut, L, p, key, sample0=SAMPLE0 + cut)
    assert torch.equal(y2, y32)


def test_drop_rate_is_within_four_sigma():
    be = calm.backend.get_backend()
    key = torch.tensor([SEED, OFFSET], dtype=torch.int64, device="cuda")
    B, L, p = 4096, 4, 0.5
    y = torch.empty(B, L, device="cuda")
    be.drop_path(torch.ones(B, L, device="cuda"), None, y, B, L, p, key, sample0=SAMPLE0)
    dropped = float((y == 0).all(dim=1).float().mean())
    print(f"dropped {dropped:.6f}")
    assert abs(dropped - p) < 4 * math.sqrt(p * (1 - p) / B)


# ---- the module ------------------------------------------------------------------------------------------------------------------
def _hip_and_emulated(name, precision, seed, dropout=0.0, state=None):
    kw = DROPOUT_BLOCKS[name]["kw"]
    hip = run_block(make_block(kw, dropout=dropout, drop_path=P, state=state).cuda().train(), kw, KeyStream(seed), device="cuda",
                    precision=precision)
    with calm.backend.use_backend(EmulatedDropPathBackend()):
        emu = run_block(make_block(kw, dropout=dropout, drop_path=P, state=state).train(), kw, KeyStream(seed),
                        precision=precision)
    return hip, emu


@pytest.mark.parametrize("name, dropout", [("A", 0.0), ("B", 0.0), ("A", 0.25)], ids=["A", "B_cross", "A_with_dropout"])
def test_block_fp32_matches_the_block_on_the_emulated_backend(name, dropout):
    (y, dx, grads, _), (ye, dxe, ge, _) = _hip_and_emulated(name, "fp32", MIXED, dropout)
    figs = {"y": rel_err(y, ye), "dx": rel_err(dx, dxe)}
    figs.update({n: rel_err(grads[n], ge[n]) for n in ge if ge[n] is not None and float(ge[n].abs().max()) > 0})
    worst = sorted(figs.items(), key=lambda kv: -kv[1])[:4]
    print(f"\n[{name} HIP fp32 vs emulation] " + ", ".join(f"{k} {v:.2e}" for k, v in worst))
    assert all(v < TOL for v in figs.values()), {k: v for k, v in figs.items() if not v < TOL}


def test_block_bf16_pipeline_against_emulation():
    """The block test_dropout_gpu.py holds to these bounds: fixture A with the weights minted for it."""
    state = block_fixture_params("A", load_golden("block_drop_A"))[1]
    (y, dx, _, _), (ye, dxe, _, _) = _hip_and_emulated("A", "bf16", MIXED, state=state)
    ey, edx = rel_err(y, ye), rel_err(dx, dxe)
    print(f"\n[A bf16 pipeline vs emulation] y {ey:.2e} dxq {edx:.2e}")
    assert ey < BF16_VS_EMULATION_BLOCK
    assert edx < 6 * BF16_VS_EMULATION_BLOCK


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_block_with_every_sample_dropped_is_the_identity_on_the_device(precision):
    kw = DROPOUT_BLOCKS["A"]["kw"]
    keys = KeyStream(ALL_DROPPED)
    y, dx, grads, gy = run_block(make_block(kw, drop_path=P).cuda().train(), kw, keys, device="cuda", precision=precision)
    assert keys.n == 2
    assert torch.equal(y, block_inputs(kw, device="cuda")[0]) and torch.equal(dx, gy)
    assert not [n for n, g in grads.items() if g is not None and not (g == 0).all()]
    yk = run_block(make_block(kw, drop_path=P).cuda().train(), kw, KeyStream(ALL_KEPT), device="cuda", precision=precision)[0]
    assert not torch.equal(yk, y)


def test_eval_mode_is_bit_identical_to_a_block_without_drop_path():
    kw = DROPOUT_BLOCKS["A"]["kw"]
    a, b = make_block(kw, drop_path=P).cuda().eval(), make_block(kw).cuda().eval()
    x = block_inputs(kw, device="cuda")[0]
    with torch.no_grad():
        assert torch.equal(a(x, mask=True), b(x, mask=True))


def test_training_repeats_under_one_seed_and_differs_under_another():
    """Default key source and default latent noise (torch's device generator): the reducing cross block draws both."""
    kw = DROPOUT_BLOCKS["B"]["kw"]
    blk = make_block(kw, drop_path=P).cuda().train()
    state = {k: v.clone() for k, v in blk.state_dict().items()}
    xq0, xkv0 = block_inputs(kw, device="cuda")
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


def test_captured_graph_draws_a_new_per_sample_mask_on_every_replay():
    B, L, p = 4096, 4, 0.5
    x = torch.from_numpy(W.make_input((B, L), 1, "x")).abs().add(1.0).cuda()        # no zero in the input ...
    res = torch.zeros(B, L, device="cuda")                                          # ... so a zero row in y is a dropped sample
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                   # warm-up outside the capture
        calm.ops.DropPathAddFn.apply(x, res, p, calm.ops.draw_dropout_key(x.device))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = calm.ops.DropPathAddFn.apply(x, res, p, calm.ops.draw_dropout_key(x.device))
    patterns = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        gone = (y == 0).all(dim=1).cpu()
        assert torch.equal((y != 0).all(dim=1).cpu(), ~gone)                         # whole rows, never parts of one
        assert torch.equal(y.cpu()[~gone], (x.cpu() * 2.0)[~gone])
        patterns.append(gone)
    assert not torch.equal(patterns[0], patterns[1])
    for z in patterns:
        assert abs(float(z.float().mean()) - p) < 4 * math.sqrt(p * (1 - p) / B)


# ---- train(drop_path=) -----------------------------------------------------------------------------------------------------------
NAME = "tiny32_cls"


def _train(hand=None, **kw):
    cfg = CONFIGS[NAME]
    gen = torch.Generator().manual_seed(3)
    data = torch.utils.data.TensorDataset(torch.randn(16, 3, cfg.seq_length, cfg.seq_length, generator=gen),
                                          torch.randint(0, cfg.out_features, (16,), generator=gen))
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    m = build_model(NAME, load_golden(NAME), "cpu")
    if hand is not None:
        vt.set_drop_path(m, hand)
    return trainer.train(m, "fused", use_gpu=True, dataset=data, epochs=1, batch_size=4, num_classes=cfg.out_features,
                         log_every=1000, max_steps=3, **kw)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_train_with_drop_path_equals_the_loop_that_sets_the_rates_itself(graph):
    be = calm.backend.get_backend()
    prev = be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, 1)
    try:
        out, hand, plain = _train(drop_path=0.2, graph=graph), _train(hand=0.2, graph=graph), _train(graph=graph)
    finally:
        be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, prev)
    a, b, c = out.state_dict(), hand.state_dict(), plain.state_dict()
    assert not [k for k in a if not torch.equal(a[k], b[k])]
    assert any(not torch.equal(a[k], c[k]) for k in a)               # ... and stochastic depth moved the run
    assert [r for _, r in vt.drop_path_rates(out)] == [0.2 * i / 23 for i in range(24)]
    assert all(bool(torch.isfinite(v).all()) for v in a.values())
