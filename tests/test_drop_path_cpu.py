"""Stochastic depth without a GPU: the emulation of calm_drop_path (tests/emulated_drop_path.py) against the dropout mask it
is defined by, the C-ABI surface (exported, declared, bound, argument checks), ops.DropPathAddFn against torch autograd,
set_drop_path's tables, VMLA_Block on the emulated backend under injected keys (all samples dropped, all kept, mixed, eval,
rate 0, with the block's dropout on), and train(drop_path=) on one and two gloo ranks against a loop that calls set_drop_path
itself, with snapshots and every refusal."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import calm_vit_dte_amd as calm
import weights as W
from emulated_backend import EmulatedBackend
from emulated_drop_path import EmulatedDropPathBackend, row_factors
from emulated_dropout import KeyStream, keep_mask, threshold_and_scale
from helpers import rel_err
from importlib import import_module
from make_golden_dropout import DROPOUT_BLOCKS
from test_host_logic_cpu import build_model
from test_snapshot_cpu import _TinySet

trainer = import_module("calm_vit_dte_amd.trainer")
vt = calm.Vi_Tools_CNN_less_V2
TOL = 1e-3                 # the project's fp32 bound
SEED, OFFSET, SAMPLE0 = 0x0123456789ABCDEF, (1 << 32) + 7, (1 << 34) + 3
# KeyStream seeds found with the emulation for B = 4, p = 0.5 and a block without dropout, whose two drop-path sites draw the
# keys (seed, 0) and (seed, 1): every sample dropped at both, every sample kept at both, samples 1 and 2 kept at both
ALL_DROPPED, ALL_KEPT, MIXED, MIXED_KEEP = 86, 210, 12, [False, True, True, False]
P = 0.5


@pytest.fixture(autouse=True)
def _restore():
    yield
    calm.backend.set_matmul_precision("fp32")
    calm.ops.set_noise_override(None)
    calm.ops.set_dropout_key_override(None)


# ---- the emulation -------------------------------------------------------------------------------------------------------------
def test_the_fixed_key_streams_are_what_the_comments_say():
    for seed, want in ((ALL_DROPPED, [False] * 4), (ALL_KEPT, [True] * 4), (MIXED, MIXED_KEEP)):
        for site in (0, 1):
            assert keep_mask(seed, site, 0, 4, P).tolist() == want


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_decisions_are_the_dropout_mask_of_the_sample_indices(p):
    B, L = 37, 6
    x = torch.from_numpy(W.make_input((B, L), 1, "x")).abs() + 1.0               # no zero in the input
    y = torch.empty_like(x)
    EmulatedDropPathBackend().drop_path(x, None, y, B, L, p, (SEED, OFFSET), sample0=SAMPLE0)
    keep = torch.from_numpy(keep_mask(SEED, OFFSET, SAMPLE0, B, p))
    assert keep.any() and not keep.all()
    assert torch.equal((y != 0).all(dim=1), keep) and torch.equal((y == 0).all(dim=1), ~keep)
    scale = float(threshold_and_scale(p)[1])
    assert torch.equal(y[keep], x[keep] * scale)
    assert torch.equal(row_factors((SEED, OFFSET), SAMPLE0, B, p) != 0, keep)


def test_p_zero_is_the_plain_sum():
    x, r = torch.from_numpy(W.make_input((5, 7), 1, "x")), torch.from_numpy(W.make_input((5, 7), 2, "r"))
    y = torch.empty_like(x)
    EmulatedDropPathBackend().drop_path(x, r, y, 5, 7, 0.0, (SEED, OFFSET))
    assert torch.equal(y, x + r)


def test_a_split_batch_with_sample0_advanced_equals_one_call():
    B, L, p, cut = 11, 5, 0.5, 3                                                 # 3: not a multiple of 4
    x, r = torch.from_numpy(W.make_input((B, L), 1, "x")), torch.from_numpy(W.make_input((B, L), 2, "r"))
    emu = EmulatedDropPathBackend()
    one, two = torch.empty_like(x), torch.empty_like(x)
    emu.drop_path(x, r, one, B, L, p, (SEED, OFFSET), sample0=SAMPLE0)
    emu.drop_path(x[:cut], r[:cut], two[:cut], cut, L, p, (SEED, OFFSET), sample0=SAMPLE0)
    emu.drop_path(x[cut:], r[cut:], two[cut:], B - cut, L, p, (SEED, OFFSET), sample0=SAMPLE0 + cut)
    assert torch.equal(one, two)
    assert not torch.equal(one, x * 2.0 + r) and not torch.equal(one, r)         # some kept, some dropped


def test_the_drop_rate_of_the_gpu_test_key_is_within_four_sigma():
    n, p = 4096, 0.5
    dropped = 1.0 - keep_mask(SEED, OFFSET, SAMPLE0, n, p).mean()
    print(f"dropped {dropped:.6f}")
    assert abs(dropped - p) < 4 * np.sqrt(p * (1 - p) / n)


# ---- the C-ABI surface -----------------------------------------------------------------------------------------------------------
_P = 0x7f0000010000                                                  # a fake, 16-byte aligned device address
_VALID = [_P, _P, _P, 8, 1024, 0, 0.25, _P, 0, 0, 0, None]         # x, residual, y, B, L, sample0, p, key, x/r/y type, stream
_REFUSED = [({0: None}, "null x"), ({2: None}, "null y"), ({7: None}, "null key"),
            ({3: -1}, "B < 0"), ({4: -1}, "L < 0"), ({5: -1}, "sample0 < 0"),
            ({6: -0.1}, "p below 0"), ({6: 1.0}, "p = 1"), ({6: 1.5}, "p above 1"), ({6: float("nan")}, "p NaN"),
            ({8: 2}, "x_type fp8"), ({9: 3}, "r_type fp8"), ({10: 2}, "y_type fp8"), ({10: -1}, "y_type negative"),
            ({3: 0, 0: None}, "null x at B = 0"), ({4: 0, 6: 1.0}, "p = 1 at L = 0")]


def test_calm_drop_path_is_exported_declared_bound_and_refuses_bad_arguments():
    """Every call below is turned down by the argument checks (or has B == 0 / L == 0, which returns before any launch): no
    kernel runs and the fake addresses are never dereferenced."""
    import test_abi_cpu as abi
    from calm_vit_dte_amd import _lib as binding
    assert "calm_drop_path" in abi._declared()
    assert hasattr(ctypes.CDLL(abi.LIB), "calm_drop_path")
    res, args = binding.SIGNATURES["calm_drop_path"]
    assert res is ctypes.c_int32 and len(args) == len(_VALID)
    assert [a for a in args[3:6]] == [ctypes.c_int64] * 3 and args[6] is ctypes.c_float
    assert binding.ABI_VERSION == 7                                  # an addition: the version does not move
    lib = binding.load()
    for change, what in _REFUSED:
        a = list(_VALID)
        for i, v in change.items():
            a[i] = v
        assert lib.calm_drop_path(*a) == binding.E_INVAL, what
    for empty in ({3: 0}, {4: 0}, {3: 0, 1: None}, {4: 0, 5: 3}):
        a = list(_VALID)
        for i, v in empty.items():
            a[i] = v
        assert lib.calm_drop_path(*a) == 0, empty                    # nothing to do


def test_hip_backend_checks_the_key_before_the_call():
    be = calm.backend.HipBackend.__new__(calm.backend.HipBackend)    # no library, no device: the check comes first
    x = torch.zeros(2, 4)
    for key in (None, torch.zeros(2, dtype=torch.int64), torch.zeros(2)):
        with pytest.raises(TypeError, match="drop_path expects its key"):
            be.drop_path(x, None, x, 2, 4, 0.5, key)


# ---- ops.DropPathAddFn against torch autograd ---------------------------------------------------------------------------------
def test_drop_path_add_fn_matches_torch_autograd():
    B, S, D, p = 9, 5, 8, 0.5
    x = torch.from_numpy(W.make_input((B, S, D), 1, "x")).requires_grad_(True)
    r = torch.from_numpy(W.make_input((B, S, D), 2, "r")).requires_grad_(True)
    gy = torch.from_numpy(W.make_input((B, S, D), 3, "gy"))
    with calm.backend.use_backend(EmulatedDropPathBackend()):
        y = calm.ops.DropPathAddFn.apply(x, r, p, KeyStream(SEED)("cpu"))
        (y * gy).sum().backward()
    f = row_factors((SEED, 0), 0, B, p)
    xr, rr = x.detach().clone().requires_grad_(True), r.detach().clone().requires_grad_(True)
    yr = xr * f[:, None, None] + rr
    (yr * gy).sum().backward()
    assert (f == 0).any() and (f != 0).any()
    assert torch.equal(y.detach(), yr.detach())
    assert torch.equal(x.grad, xr.grad) and torch.equal(r.grad, rr.grad)
    assert torch.equal((x.grad == 0).all(dim=2).all(dim=1), f == 0)              # the backward regenerated the forward's mask


def test_plain_emulated_backends_have_no_drop_path():
    """The kernel is not optional: a backend without the entry point fails, it does not skip the drop."""
    x = torch.zeros(2, 4)
    with calm.backend.use_backend(EmulatedBackend()), pytest.raises(AttributeError, match="drop_path"):
        calm.ops.DropPathAddFn.apply(x, x, 0.5, KeyStream(1)("cpu"))


# ---- set_drop_path ---------------------------------------------------------------------------------------------------------------
def test_set_drop_path_tables_order_and_refusals():
    m = build_model("tiny32_cls", None)
    ed = "autoencoder."
    order = [f"{ed}{stage}.{part}" for stage in ([f"encoder_blocks.{i}" for i in range(3)]
                                                 + ["block_bottle_neck_1", "block_bottle_neck_2"]
                                                 + [f"decoder_blocks.{i}" for i in range(3)])
             for part in ("encoder", "decoder", "cross")]
    assert [n for n, _ in vt.drop_path_rates(m)] == order and len(order) == 24
    assert all(r == 0.0 for _, r in vt.drop_path_rates(m))           # off by default
    table = vt.set_drop_path(m, 0.23)
    assert [n for n, _ in table] == order
    assert [r for _, r in table] == [0.23 * i / 23 for i in range(24)]            # timm's rule
    assert dict(m.named_modules())[order[-1]].drop_path == 0.23 and dict(m.named_modules())[order[0]].drop_path == 0.0
    assert [r for _, r in vt.set_drop_path(m, 0.1, schedule="uniform")] == [0.1] * 24
    assert vt.set_drop_path(m, 0.1, "linear") == vt.drop_path_rates(m)
    sub = m.autoencoder.decoder_blocks[2]
    assert [r for _, r in vt.set_drop_path(sub, 0.3)] == [0.0, 0.15, 0.3]         # any module: its own blocks
    assert vt.set_drop_path(sub.cross, 0.4) == [("", 0.4)]                        # a single block gets the rate
    assert all(r == 0.0 for _, r in vt.set_drop_path(m, 0)) and vt.VMLA_Block.drop_path == 0.0
    for bad in (1.0, -0.1, 1.5, float("nan"), "0.1", None, True):
        with pytest.raises(ValueError, match="0 <= rate < 1"):
            vt.set_drop_path(m, bad)
    with pytest.raises(ValueError, match='"linear" or "uniform"'):
        vt.set_drop_path(m, 0.1, schedule="cosine")
    assert all(r == 0.0 for _, r in vt.drop_path_rates(m))           # a refused call changes nothing


# ---- the module ------------------------------------------------------------------------------------------------------------------
_KW_A = DROPOUT_BLOCKS["A"]["kw"]                                    # dim1 == dim2, no sequence change, with an MLP
assert _KW_A["dim1"] == _KW_A["dim2"] and _KW_A["seq_length"] == _KW_A["seq_len_new"]


def make_block(kw, dropout=0.0, drop_path=0.0, state=None, use_mlp=True):
    blk = vt.VMLA_Block(mlp_dim=2 * kw["dim2"], force_reduce=False, dropout=dropout, use_mlp=use_mlp, **kw)
    if state is None:
        shapes = {k: tuple(v.shape) for k, v in blk.state_dict().items()}
        state = {k: torch.from_numpy(v) for k, v in W.make_params(shapes, 77).items()}
    blk.load_state_dict({k: v.clone() for k, v in state.items()})
    if drop_path:
        blk.drop_path = drop_path
    return blk


def block_inputs(kw, B=4, device="cpu"):
    xq = torch.from_numpy(W.make_input((B, kw["seq_length"], kw["dim1"]), 5, "xq")).to(device)
    xkv = torch.from_numpy(W.make_input((B, kw["seq_length"], kw["dim1"]), 6, "xkv")).to(device) if kw["is_cross"] else None
    return xq, xkv


def run_block(blk, kw, keys, B=4, device="cpu", precision="fp32", noise_seed=9):
    """One forward + backward of `blk` under the injected keys and noise on whatever backend is installed:
    (y, dxq, {name: grad}, gy)."""
    xq, xkv = block_inputs(kw, B, device)
    xq.requires_grad_(True)
    calm.backend.set_matmul_precision(precision)
    calm.ops.set_dropout_key_override(keys)
    calm.ops.set_noise_override(W.NoiseStream(noise_seed))
    try:
        y = blk(xq, input_kv=xkv, state_manager=vt.ResidualStateManager(mode="sum"), mask=True)
        gy = torch.from_numpy(W.make_input(tuple(y.shape), 8, "gy")).to(device)
        if blk.training:
            (y * gy).sum().backward()
    finally:
        calm.ops.set_dropout_key_override(None)
        calm.ops.set_noise_override(None)
        calm.backend.set_matmul_precision("fp32")
    return y.detach(), xq.grad, {n: prm.grad for n, prm in blk.named_parameters()}, gy


def test_block_with_every_sample_dropped_is_the_identity_with_zero_branch_gradients():
    blk = make_block(_KW_A, drop_path=P).train()
    keys = KeyStream(ALL_DROPPED)
    with calm.backend.use_backend(EmulatedDropPathBackend()):
        y, dx, grads, gy = run_block(blk, _KW_A, keys)
    assert keys.n == 2                                               # one key per site
    assert torch.equal(y, block_inputs(_KW_A)[0])                    # bit for bit
    assert torch.equal(dx, gy)
    assert grads["ls_att"] is not None and grads["ls_mlp"] is not None and grads["mlp.0.weight_orig"] is not None
    assert not [n for n, g in grads.items() if g is not None and not (g == 0).all()]


def _scaled_reference(kw, scale):
    """The block without drop-path whose ls_att / ls_mlp carry the factor of a kept sample."""
    ref = make_block(kw).train()
    with torch.no_grad():
        ref.ls_att.mul_(scale)
        ref.ls_mlp.mul_(scale)
    return ref


def test_block_with_every_sample_kept_is_the_block_with_scaled_layer_scales():
    scale = float(threshold_and_scale(P)[1])
    drawn = KeyStream(ALL_KEPT)
    with calm.backend.use_backend(EmulatedDropPathBackend()):
        y, dx, grads, _ = run_block(make_block(_KW_A, drop_path=P).train(), _KW_A, drawn)
        yr, dxr, gr, _ = run_block(_scaled_reference(_KW_A, scale), _KW_A, KeyStream(ALL_KEPT))
    assert drawn.n == 2
    figs = {"y": rel_err(y, yr), "dx": rel_err(dx, dxr)}
    figs.update({n: rel_err(grads[n], gr[n]) for n in grads if n not in ("ls_att", "ls_mlp") and gr[n] is not None})
    figs.update({n: rel_err(grads[n], gr[n] * scale) for n in ("ls_att", "ls_mlp")})   # d/d(ls) of (scale ls) is scale times it
    print({k: f"{v:.1e}" for k, v in sorted(figs.items(), key=lambda kv: -kv[1])[:4]})
    assert all(v < TOL for v in figs.values()), {k: v for k, v in figs.items() if not v < TOL}


def test_block_with_a_mixed_mask_keeps_and_drops_whole_samples():
    keep = torch.tensor(MIXED_KEEP)
    with calm.backend.use_backend(EmulatedDropPathBackend()):
        y, dx, _, gy = run_block(make_block(_KW_A, drop_path=P).train(), _KW_A, KeyStream(MIXED))
        yk, dxk, _, _ = run_block(make_block(_KW_A, drop_path=P).train(), _KW_A, KeyStream(ALL_KEPT))
    x = block_inputs(_KW_A)[0]
    assert torch.equal(y[~keep], x[~keep]) and torch.equal(dx[~keep], gy[~keep])
    assert torch.equal(y[keep], yk[keep]) and torch.equal(dx[keep], dxk[keep])
    assert not torch.equal(yk[~keep], x[~keep])


def test_block_without_an_mlp_drops_its_attention_site_only():
    blk = make_block(_KW_A, drop_path=P, use_mlp=False).train()
    keys = KeyStream(ALL_DROPPED)
    with calm.backend.use_backend(EmulatedDropPathBackend()):
        y, _, grads, _ = run_block(blk, _KW_A, keys)
        ln = blk.ln_2(block_inputs(_KW_A)[0])
    assert keys.n == 1 and torch.equal(y, ln.detach())               # ln_2(skip path): the branch is gone
    assert (grads["ls_att"] == 0).all()


def test_eval_mode_and_rate_zero_are_the_block_as_it_is_and_draw_no_key():
    a, b = make_block(_KW_A, drop_path=P), make_block(_KW_A)
    drawn = []
    keys = lambda device: drawn.append(1) or KeyStream(1)(device)    # noqa: E731
    with calm.backend.use_backend(EmulatedDropPathBackend()):
        ya, yb = run_block(a.eval(), _KW_A, keys)[0], run_block(b.eval(), _KW_A, keys)[0]
        assert torch.equal(ya, yb) and not drawn
        a.drop_path = 0.0
        out_a, out_b = run_block(a.train(), _KW_A, keys), run_block(b.train(), _KW_A, keys)
    assert not drawn
    assert torch.equal(out_a[0], out_b[0]) and torch.equal(out_a[1], out_b[1])
    assert all(torch.equal(out_a[2][n], out_b[2][n]) for n in out_b[2] if out_b[2][n] is not None)
    with calm.backend.use_backend(EmulatedBackend()):                # ... on a backend that has neither kernel, too
        assert torch.equal(run_block(make_block(_KW_A).train(), _KW_A, keys)[0], out_b[0])


def test_with_the_blocks_dropout_on_the_site_order_is_dropout_then_drop_path():
    """Keys: attention dropout, attention drop-path, MLP dropout, MLP drop-path.  With every sample kept by the drop-path
    keys (offsets 1 and 3) the block equals the dropout-only block with scaled layer scales under the dropout keys
    (offsets 0 and 2); with every sample dropped it is the identity."""
    kept = next(s for s in range(1, 4000) if keep_mask(s, 1, 0, 4, P).all() and keep_mask(s, 3, 0, 4, P).all())
    gone = next(s for s in range(1, 4000) if not keep_mask(s, 1, 0, 4, P).any() and not keep_mask(s, 3, 0, 4, P).any())
    scale = float(threshold_and_scale(P)[1])

    class EvenKeys(KeyStream):                                       # the dropout-only block draws offsets 0, 2
        def __call__(self, device):
            key = torch.tensor([self.seed, 2 * self.n], dtype=torch.int64, device=device)
            self.n += 1
            return key

    with calm.backend.use_backend(EmulatedDropPathBackend()):
        keys = KeyStream(kept)
        y, dx, grads, _ = run_block(make_block(_KW_A, dropout=0.25, drop_path=P).train(), _KW_A, keys)
        ref = make_block(_KW_A, dropout=0.25).train()
        with torch.no_grad():
            ref.ls_att.mul_(scale)
            ref.ls_mlp.mul_(scale)
        yr, dxr, gr, _ = run_block(ref, _KW_A, EvenKeys(kept))
        assert keys.n == 4
        figs = {"y": rel_err(y, yr), "dx": rel_err(dx, dxr), "mlp.0": rel_err(grads["mlp.0.weight_orig"], gr["mlp.0.weight_orig"]),
                "out_proj": rel_err(grads["out_proj.weight_orig"], gr["out_proj.weight_orig"])}
        print(figs)
        assert all(v < TOL for v in figs.values()), figs
        y0, dx0, _, gy = run_block(make_block(_KW_A, dropout=0.25, drop_path=P).train(), _KW_A, KeyStream(gone))
    assert torch.equal(y0, block_inputs(_KW_A)[0]) and torch.equal(dx0, gy)


# ---- train(drop_path=) ---------------------------------------------------------------------------------------------------------
def _train(seed=50, n=8, epochs=1, hand=None, **kw):
    """train() on tiny32_cls with the emulated backend; hand=(rate, schedule): the caller's own set_drop_path in front of a
    train() that is not told about stochastic depth."""
    torch.manual_seed(seed)
    m = build_model("tiny32_cls", None).train()
    if hand is not None:
        vt.set_drop_path(m, *hand)
    with calm.backend.use_backend(EmulatedDropPathBackend()):
        return trainer.train(m, "fused", None, use_gpu=False, dataset=_TinySet(n), epochs=epochs, batch_size=4,
                             num_classes=10, collate_fn="mix", num_workers=0, log_every=1000, **kw)


def _same_bits(a, b, what):
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{what}: differs at {k}"


def _differ(a, b):
    return any(not torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))


@pytest.mark.timeout(600)
def test_train_with_drop_path_equals_the_loop_that_sets_the_rates_itself(capsys):
    out = _train(drop_path=0.4)
    assert "drop_path: linear over 24 blocks, rates 0.0000 .. 0.4000" in capsys.readouterr().out
    assert [r for _, r in vt.drop_path_rates(out)] == [0.4 * i / 23 for i in range(24)]      # the returned model keeps them
    _same_bits(out, _train(hand=(0.4, "linear")), "train(drop_path=0.4) against set_drop_path + train()")
    plain = _train()
    assert _differ(out, plain) and all(r == 0.0 for _, r in vt.drop_path_rates(plain))
    uni = _train(drop_path={"rate": 0.4, "schedule": "uniform"})
    assert "drop_path: uniform over 24 blocks, rates 0.4000 .. 0.4000" in capsys.readouterr().out
    _same_bits(uni, _train(hand=(0.4, "uniform")), "the uniform schedule")
    assert _differ(uni, out)
    _same_bits(plain, _train(drop_path={"rate": 0.0}), "rate 0 against a run that never mentions the argument")


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kw", [dict(accumulate=2, n=16), dict(lamb=True)], ids=["accumulate", "lamb"])
def test_train_with_drop_path_under_a_window_and_under_lamb(kw):
    out = _train(drop_path=0.4, **kw)
    _same_bits(out, _train(hand=(0.4, "linear"), **kw), f"train(drop_path=0.4, {kw})")
    assert all(bool(torch.isfinite(p).all()) for p in out.parameters())


@pytest.mark.timeout(600)
def test_snapshot_header_refusals_and_exact_resume(tmp_path):
    fa, fb, fc, fd = (str(tmp_path / f"{n}.snap") for n in "abcd")
    a = _train(epochs=2, drop_path=0.4, snapshot_path=fa)
    _train(epochs=2, drop_path=0.4, snapshot_path=fb, max_steps=2)
    head = trainer.TrainState.read_header(fb)[0]["host"]
    assert head["progress"]["step"] == 2 and head["drop_path"] == [0.4 * i / 23 for i in range(24)]
    c = _train(seed=51, epochs=2, drop_path=0.4, snapshot_path=fc, resume=fb)
    _same_bits(a, c, "the resumed run")
    with pytest.raises(ValueError, match="written with drop_path rates 0 .. 0.4, this model runs without drop_path"):
        _train(epochs=2, snapshot_path=fc, resume=fb)
    with pytest.raises(ValueError, match="written with drop_path rates 0 .. 0.4, this model runs with drop_path rates 0 .. 0.2"):
        _train(epochs=2, drop_path=0.2, snapshot_path=fc, resume=fb)
    _train(epochs=2, snapshot_path=fd, max_steps=2)
    assert "drop_path" not in trainer.TrainState.read_header(fd)[0]["host"]
    with pytest.raises(ValueError, match="written without drop_path, this model runs with drop_path rates"):
        _train(epochs=2, drop_path=0.4, snapshot_path=fc, resume=fd)


def test_train_refusals_come_before_any_process_group():
    data = torch.utils.data.TensorDataset(torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,)))
    lin = torch.nn.Linear(4, 4)
    kw = dict(use_gpu=False, dataset=data, epochs=1, batch_size=2, num_classes=10)
    for bad in (1.0, -0.1, float("nan"), {"rate": 1.5}):
        with pytest.raises(ValueError, match=r'drop_path\["rate"\] is a probability'):
            trainer.train(lin, "fused", drop_path=bad, **kw)
    with pytest.raises(ValueError, match='"linear" or "uniform"'):
        trainer.train(lin, "fused", drop_path={"rate": 0.1, "schedule": "cosine"}, **kw)
    for bad in ({"rate": 0.1, "mode": "row"}, {"schedule": "linear"}):
        with pytest.raises(ValueError, match='drop_path takes the keys "rate"'):
            trainer.train(lin, "fused", drop_path=bad, **kw)
    for bad in (True, "0.1", [0.1]):
        with pytest.raises(ValueError, match="drop_path is None, a rate or a dict"):
            trainer.train(lin, "fused", drop_path=bad, **kw)
    assert not torch.distributed.is_initialized()


# ---- two gloo ranks ------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _two_rank_worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    run = _train(n=16, drop_path=0.4, destroy_process_group=False)
    hand = _train(n=16, hand=(0.4, "linear"), destroy_process_group=False)
    torch.save(dict(run=run.state_dict(), hand=hand.state_dict()), os.path.join(outdir, f"rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_train_with_drop_path_on_two_gloo_ranks(tmp_path):
    mp.spawn(_two_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(2))
    for k in r0["run"]:
        assert torch.equal(r0["run"][k], r0["hand"][k]), f"train(drop_path=) differs from the hand-written loop at {k}"
        assert torch.equal(r0["run"][k], r1["run"][k]), f"the ranks diverged at {k}"
