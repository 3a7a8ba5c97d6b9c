"""Dropout without a GPU: the numpy Philox of tests/emulated_dropout.py against known answers, the threshold / drop-rate
arithmetic, the C-ABI surface of calm_dropout (exported, declared, bound, argument checks), and the host logic
(ops.DropoutAddFn, ops.MlpFn with p > 0, VMLA_Block) on the emulated backend — against plain-torch autograd compositions
and against the two block fixtures minted from the reference (tests/golden/make_golden_dropout.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import weights as W
from emulated_backend import EmulatedBackend
from emulated_dropout import (EmulatedDropoutBackend, KeyStream, dropout_words, keep_mask, multiplier, philox4x32_10,
                              threshold_and_scale)
from helpers import block_fixture_params, load_golden, rel_err
from make_golden_dropout import DROPOUT_BLOCKS, KEY_SEED, NOISE_SEED

TOL = 1e-5                 # the project's bound for CPU restatements
SEED, OFFSET, N = 0x0123456789ABCDEF, 7, 1 << 20


@pytest.fixture(autouse=True)
def _restore():
    yield
    calm.backend.set_matmul_precision("fp32")
    calm.ops.set_noise_override(None)
    calm.ops.set_dropout_key_override(None)


# ---- the random bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter, key, out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(counter, key, out):
    assert " ".join(f"{int(w):08x}" for w in philox4x32_10(counter, key)) == out


def test_words_follow_the_counter_layout():
    """word(e) = output word e & 3 of the call for group e >> 2, all four 32-bit halves of (group, offset) in use."""
    off, e0 = (1 << 32) + 7, (1 << 34) + 4
    w = dropout_words(SEED, off, e0, 9)
    for j in (0, 3, 4, 8):
        e = e0 + j
        ref = philox4x32_10(((e >> 2) & 0xffffffff, (e >> 2) >> 32, off & 0xffffffff, off >> 32),
                            (SEED & 0xffffffff, SEED >> 32))
        assert int(w[j]) == int(ref[e & 3])
    assert np.array_equal(dropout_words(SEED, off, e0 + 4, 5), w[4:])               # a second call continues the first


@pytest.mark.parametrize("p, thr, frac", [(0.1, 429496736, 0.0999689), (0.25, 1073741824, 0.2500887),
                                          (0.5, 2147483648, 0.4999323)])
def test_threshold_and_drop_rate(p, thr, frac):
    assert threshold_and_scale(p)[0] == thr
    assert threshold_and_scale(p)[1] == np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    dropped = 1.0 - keep_mask(SEED, OFFSET, 0, N, p).mean()
    print(f"p {p}: dropped {dropped:.7f}")
    assert abs(dropped - frac) < 5e-8
    assert abs(dropped - p) < 4 * math.sqrt(p * (1 - p) / N)


def test_mask_is_a_function_of_seed_and_offset():
    a = keep_mask(SEED, OFFSET, 0, N, 0.25)
    assert np.array_equal(a, keep_mask(SEED, OFFSET, 0, N, 0.25))
    assert not np.array_equal(a, keep_mask(SEED, OFFSET + 1, 0, N, 0.25))
    assert not np.array_equal(a, keep_mask(SEED + 1, OFFSET, 0, N, 0.25))


def test_p_zero_keeps_everything_exactly():
    assert keep_mask(SEED, OFFSET, 0, 4096, 0.0).all()
    x, r = torch.from_numpy(W.make_input((4099,), 1, "x")), torch.from_numpy(W.make_input((4099,), 2, "r"))
    y = torch.empty_like(x)
    EmulatedDropoutBackend().dropout(x, r, y, x.numel(), 0.0, (SEED, OFFSET))
    assert torch.equal(y, x + r)


# ---- the C-ABI surface ---------------------------------------------------------------------------------------------------
_P = 0x7f0000010000                                                  # a fake, 16-byte aligned device address
_VALID = [_P, _P, _P, 1024, 0, 0.25, _P, 0, 0, 0, None]            # x, residual, y, n, e0, p, key, x/r/y type, stream
_REFUSED = [({0: None}, "null x"), ({2: None}, "null y"), ({6: None}, "null key"),
            ({5: -0.1}, "p below 0"), ({5: 1.0}, "p = 1"), ({5: 1.5}, "p above 1"), ({5: float("nan")}, "p NaN"),
            ({4: -4}, "negative e0"), ({4: 2}, "e0 % 4 != 0"), ({4: 1027}, "e0 % 4 != 0"),
            ({7: 2}, "x_type fp8"), ({8: 3}, "r_type fp8"), ({9: 2}, "y_type fp8"), ({9: -1}, "y_type negative"),
            ({3: 0, 0: None}, "null x at n = 0"), ({3: 0, 5: 1.0}, "p = 1 at n = 0")]


def test_calm_dropout_is_exported_declared_bound_and_refuses_bad_arguments():
    """Every call below is turned down by the argument checks (or is n == 0, which returns before any launch): no kernel
    runs and the fake addresses are never dereferenced."""
    import test_abi_cpu as abi
    from calm_vit_dte_amd import _lib as binding
    assert "calm_dropout" in abi._declared()
    assert hasattr(ctypes.CDLL(abi.LIB), "calm_dropout")
    res, args = binding.SIGNATURES["calm_dropout"]
    assert res is ctypes.c_int32 and len(args) == len(_VALID)
    assert binding.ABI_VERSION == 7                                  # an addition: the version does not move
    lib = binding.load()
    for change, what in _REFUSED:
        a = list(_VALID)
        for i, v in change.items():
            a[i] = v
        assert lib.calm_dropout(*a) == binding.E_INVAL, what
    a = list(_VALID)
    a[3] = 0
    assert lib.calm_dropout(*a) == 0                                  # n == 0: nothing to do
    a[1] = None
    assert lib.calm_dropout(*a) == 0                                  # ... with the residual absent, too


# ---- ops on the emulated backend against plain-torch autograd -----------------------------------------------------------
def _sn_weight(name, rows, cols):
    """(w, u, v, sigma) of a spectral-normed layer after a few power iterations; sigma = u^T W v as the package holds it."""
    w = torch.from_numpy(W.make_tensor(name + ".weight_orig", (rows, cols), 11))
    u = torch.from_numpy(W.make_tensor(name + ".weight_u", (rows,), 11))
    for _ in range(8):
        v = torch.nn.functional.normalize(w.t() @ u, dim=0)
        u = torch.nn.functional.normalize(w @ v, dim=0)
    return w.requires_grad_(True), u, v, torch.dot(u, w.detach() @ v).reshape(1)


def test_dropout_add_fn_matches_torch_autograd():
    rows, n, p = 48, 96, 0.25
    x = torch.from_numpy(W.make_input((rows, n), 1, "x")).requires_grad_(True)
    r = torch.from_numpy(W.make_input((rows, n), 2, "r")).requires_grad_(True)
    gy = torch.from_numpy(W.make_input((rows, n), 3, "gy"))
    keys = KeyStream(SEED)
    with calm.backend.use_backend(EmulatedDropoutBackend()):
        y = calm.ops.DropoutAddFn.apply(x, r, p, keys("cpu"))
        (y * gy).sum().backward()
    m = multiplier((SEED, 0), 0, rows * n, p).view(rows, n)
    xr, rr = x.detach().clone().requires_grad_(True), r.detach().clone().requires_grad_(True)
    yr = xr * m + rr
    (yr * gy).sum().backward()
    assert (m == 0).any() and (m != 0).any()
    assert torch.equal(y.detach(), yr.detach())
    assert rel_err(x.grad, xr.grad) < TOL and rel_err(r.grad, rr.grad) < TOL
    assert torch.equal(x.grad == 0, m == 0)                         # the backward regenerated the forward's mask


def test_mlp_fn_with_dropout_matches_torch_autograd():
    rows, K, Hd, p = 48, 96, 192, 0.25
    N = K
    w1, u1, v1, s1 = _sn_weight("mlp.0", Hd, K)
    w2, u2, v2, s2 = _sn_weight("mlp.3", N, Hd)
    b1 = torch.from_numpy(W.make_tensor("mlp.0.bias", (Hd,), 11)).requires_grad_(True)
    b2 = None                          # (no caller combines a second bias with LayerScale: the block MLP has no biases)
    ls = torch.from_numpy(W.make_tensor("ls_mlp", (N,), 11)).requires_grad_(True)
    x = torch.from_numpy(W.make_input((rows, K), 1, "x")).requires_grad_(True)
    res = torch.from_numpy(W.make_input((rows, N), 2, "r")).requires_grad_(True)
    gy = torch.from_numpy(W.make_input((rows, N), 3, "gy"))
    leaves = (x, w1, b1, w2, ls, res)
    key = KeyStream(SEED)("cpu")
    with calm.backend.use_backend(EmulatedDropoutBackend()):
        y = calm.ops.MlpFn.apply(x, w1, b1, w2, b2, ls, res, u1, v1, s1, u2, v2, s2, p, key)
        (y * gy).sum().backward()
    got = [t.grad.clone() for t in leaves]
    for t in leaves:
        t.grad = None
    m = multiplier((SEED, 0), 0, rows * Hd, p).view(rows, Hd)
    sig = lambda w, u, v: torch.dot(u, w @ v)                         # sigma is a function of the weight (u, v constants)
    h = torch.nn.functional.gelu(x @ (w1 / sig(w1, u1, v1)).t() + b1) * m
    yr = (h @ (w2 / sig(w2, u2, v2)).t()) * ls + res
    (yr * gy).sum().backward()
    assert rel_err(y.detach(), yr.detach()) < TOL
    for name, a, t in zip(("dx", "dW1", "db1", "dW2", "d_ls", "dres"), got, leaves):
        assert rel_err(a, t.grad) < TOL, name
    # thirteen positional arguments, as every existing caller passes: no dropout, no key needed
    with calm.backend.use_backend(EmulatedDropoutBackend()), torch.no_grad():
        y0 = calm.ops.MlpFn.apply(x, w1, b1, w2, b2, ls, res, u1, v1, s1, u2, v2, s2)
        h0 = torch.nn.functional.gelu(x @ (w1 / s1).t() + b1)
        assert rel_err(y0, (h0 @ (w2 / s2).t()) * ls + res) < TOL


# ---- the module ------------------------------------------------------------------------------------------------------------
_KW_A = DROPOUT_BLOCKS["A"]["kw"]


def _block(kw, dropout, state=None):
    vt = calm.Vi_Tools_CNN_less_V2
    blk = vt.VMLA_Block(mlp_dim=2 * kw["dim2"], force_reduce=False, dropout=dropout, **kw)
    if state is None:
        shapes = {k: tuple(v.shape) for k, v in blk.state_dict().items()}
        state = {k: torch.from_numpy(v) for k, v in W.make_params(shapes, 77).items()}
    blk.load_state_dict({k: v.clone() for k, v in state.items()})
    return blk


def test_block_constructor_accepts_dropout_in_range():
    blk = _block(_KW_A, 0.25)
    assert blk.dropout.p == 0.25 and blk.mlp[2].p == 0.25
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="0 <= dropout < 1"):
            _block(_KW_A, bad)


def _run(blk, x, keys=None, noise=None):
    calm.ops.set_dropout_key_override(keys)
    calm.ops.set_noise_override(noise)
    try:
        with calm.backend.use_backend(EmulatedDropoutBackend()), torch.no_grad():
            return blk(x, mask=True)
    finally:
        calm.ops.set_dropout_key_override(None)
        calm.ops.set_noise_override(None)


def test_block_in_eval_mode_ignores_dropout_bit_for_bit():
    a, b = _block(_KW_A, 0.25), _block(_KW_A, 0.0)
    b.load_state_dict(a.state_dict())
    x = torch.from_numpy(W.make_input((2, _KW_A["seq_length"], _KW_A["dim1"]), 5, "xq"))
    drawn = []
    keys = lambda device: drawn.append(1) or KeyStream(1)(device)
    ya, yb = _run(a.eval(), x, keys), _run(b.eval(), x, keys)
    assert torch.equal(ya, yb) and not drawn                        # no key is drawn when dropout is inactive
    yt = _run(b.train(), x, keys)                                   # p == 0 in training mode: the same path
    assert not drawn and torch.isfinite(yt).all()


def test_setting_p_on_the_dropout_modules_takes_effect():
    """The torch idiom: `for m in model.modules(): if isinstance(m, nn.Dropout): m.p = ...` on a dropout=0 block."""
    blk = _block(_KW_A, 0.0).train()
    x = torch.from_numpy(W.make_input((2, _KW_A["seq_length"], _KW_A["dim1"]), 5, "xq"))
    state = {k: v.clone() for k, v in blk.state_dict().items()}      # (a training forward moves u / v)
    y0 = _run(blk, x, KeyStream(3))
    drops = [m for m in blk.modules() if isinstance(m, torch.nn.Dropout)]
    assert len(drops) == 2
    outs = []
    for setting in ((0.1, 0.0), (0.0, 0.1), (0.1, 0.1)):
        blk.load_state_dict(state)
        blk.dropout.p, blk.mlp[2].p = setting
        keys = KeyStream(3)
        outs.append(_run(blk, x, keys))
        assert keys.n == sum(s > 0 for s in setting)                # one key per active site
        assert not torch.equal(outs[-1], y0)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    blk.load_state_dict(state)
    for m in drops:
        m.p = 0.0
    assert torch.equal(_run(blk, x, KeyStream(3)), y0)


# ---- the fixtures minted from the reference ------------------------------------------------------------------------------
def run_dropout_fixture(name, precision="fp32", device="cpu"):
    """One training forward + backward of the package's VMLA_Block on fixture `name` under the fixture's keys and noise (on
    whatever backend is installed): (fixture, kwargs, block, y, kl, xq, xkv)."""
    vt = calm.Vi_Tools_CNN_less_V2
    g = load_golden("block_drop_" + name)
    spec = DROPOUT_BLOCKS[name]
    kw, B = spec["kw"], spec["batch"]
    assert float(g["p"]) == np.float32(spec["p"])
    shapes, P = block_fixture_params(name, g)
    blk = vt.VMLA_Block(mlp_dim=2 * kw["dim2"], force_reduce=False, dropout=spec["p"], **kw)
    assert {k: tuple(v.shape) for k, v in blk.state_dict().items()} == shapes
    blk.load_state_dict({k: v.clone() for k, v in P.items()})
    blk = blk.to(device).train()
    S, D1 = kw["seq_length"], kw["dim1"]
    xq = torch.from_numpy(W.make_input((B, S, D1), 5, "xq")).to(device).requires_grad_(True)
    xkv = torch.from_numpy(W.make_input((B, S, D1), 6, "xkv")).to(device).requires_grad_(True) if kw["is_cross"] else None
    sm = vt.ResidualStateManager(mode="sum")
    calm.backend.set_matmul_precision(precision)
    calm.ops.set_noise_override(W.NoiseStream(NOISE_SEED))
    calm.ops.set_dropout_key_override(KeyStream(KEY_SEED))
    try:
        y = blk(xq, input_kv=xkv, state_manager=sm, mask=True)
        gy = torch.from_numpy(W.make_input(tuple(y.shape), 8, "gy")).to(device)
        kl = sm.get_kl_loss()
        ((y * gy).sum() + 0.5 * kl).backward()
    finally:
        calm.ops.set_noise_override(None)
        calm.ops.set_dropout_key_override(None)
    return g, kw, blk, y.detach(), kl, xq, xkv


def check_against_fixture(g, kw, blk, y, kl, xq, xkv, tol, label=""):
    """y, kl, the input gradients, every recorded parameter gradient (norms of all, the small ones in full) and the power
    iteration vectors within `tol` (max-abs error over max-abs reference); prints each figure before it asserts."""
    params, sd = dict(blk.named_parameters()), blk.state_dict()
    figs = {"y": rel_err(y, g["y"]), "kl": abs(float(kl.detach() if torch.is_tensor(kl) else kl) - float(g["kl"])) / max(1.0, abs(float(g["kl"]))),
            "dxq": rel_err(xq.grad, g["dxq"])}
    if kw["is_cross"]:
        figs["dxkv"] = rel_err(xkv.grad, g["dxkv"])
    for n, ref in zip([str(s) for s in g["grad_names"]], g["grad_norms"]):
        figs["norm/" + n] = abs(float(params[n].grad.norm()) - float(ref)) / max(abs(float(ref)), 1e-6)
    for key in g.files:
        if key.startswith("grad/"):
            figs[key] = rel_err(params[key[5:]].grad, g[key])
        if key.startswith("post/"):
            figs[key] = rel_err(sd[key[5:]], g[key])
    worst = sorted(figs.items(), key=lambda kv: -kv[1])[:4]
    print(f"\n[{label}] y {figs['y']:.2e} dxq {figs['dxq']:.2e} worst " + ", ".join(f"{k} {v:.2e}" for k, v in worst))
    for k, v in figs.items():
        assert v < tol, (k, v)


@pytest.mark.parametrize("name", list(DROPOUT_BLOCKS))
def test_block_with_dropout_matches_reference_fixture_on_the_emulated_backend(name):
    with calm.backend.use_backend(EmulatedDropoutBackend()):
        out = run_dropout_fixture(name)
    assert (out[2].mlp[2].p, out[2].dropout.p) == (DROPOUT_BLOCKS[name]["p"],) * 2
    check_against_fixture(*out, tol=TOL, label=f"{name} emulated fp32")


def test_plain_emulated_backend_has_no_dropout():
    """The kernel is not optional: a backend without the entry point fails, it does not skip the dropout."""
    blk = _block(_KW_A, 0.25).train()
    x = torch.from_numpy(W.make_input((1, _KW_A["seq_length"], _KW_A["dim1"]), 5, "xq"))
    calm.ops.set_dropout_key_override(KeyStream(1))
    with calm.backend.use_backend(EmulatedBackend()), pytest.raises(AttributeError, match="dropout"):
        blk(x, mask=True)
