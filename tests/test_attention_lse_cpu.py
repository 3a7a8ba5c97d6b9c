"""Row-LSE mode of the fp32 attention (train without the saved probabilities) on a host without a GPU: the three C-ABI
additions are declared, exported and bound, the scratch query answers from host code, the storage switch behaves, and
the host logic of ops.LatentMaskAttentionLseFn — what it saves, what it returns, where the model takes it and where it
falls back — is checked over the torch emulation of the entry points (tests/emulated_lse.py)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import calm_vit_dte_amd as calm
import weights as W
from emulated_lse import EmulatedLseBackend
from helpers import CONFIGS, load_golden, rel_err
from test_attention_gpu import SHAPES, _inputs
from test_host_logic_cpu import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "calm_vit.h")
NAMES = ("calm_attention_fwd_lse", "calm_attention_bwd_lse_scratch_bytes", "calm_attention_bwd_lse")
TOL = 1e-4                                    # the project's fp32 kernel tolerance (normalised inf-norm, helpers.rel_err)


@pytest.fixture(autouse=True)
def _restore_storage():
    prev = calm.backend.get_attention_storage()
    yield
    calm.backend.set_attention_storage(prev)
    calm.ops.set_noise_override(None)


def test_entry_points_are_declared_exported_and_bound_and_the_scratch_query_is_host_code():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(calm_\w+)\s*\(", text, flags=re.M))
    binding = calm._lib
    lib = binding.load()                                       # resolves every bound symbol, checks the ABI version
    for n in NAMES:
        assert n in declared, n
        assert n in binding.SIGNATURES, n
        assert hasattr(lib, n), n
    assert int(re.search(r"#define\s+CALM_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 7   # additions only
    query = lib.calm_attention_bwd_lse_scratch_bytes
    assert query.restype is ctypes.c_int64
    for B, S, H, hd in SHAPES:
        need = int(query(B, S, S, H, hd))
        assert need > 0, (B, S, H, hd)
        assert need % 16 == 0 and need <= 2 * 4 * B * H * S * S   # never more than the two [B,H,Sq,Skv] planes
    for Sq, Skv, H, hd in ((36, 36, 3, 36), (64, 64, 4, 24), (224, 176, 6, 112)):
        assert int(query(2, Sq, Skv, H, hd)) == 0, (Sq, Skv, H, hd)
    assert int(query(0, 80, 80, 6, 40)) == 0


def test_storage_switch_default_round_trip_unknown_name_and_environment():
    be = calm.backend
    if not os.environ.get("CALM_ATTN_STORAGE"):
        assert be.get_attention_storage() == "probs"
    be.set_attention_storage("lse")
    assert be.get_attention_storage() == "lse"
    be.set_attention_storage("probs")
    assert be.get_attention_storage() == "probs"
    with pytest.raises(ValueError, match="unknown attention storage"):
        be.set_attention_storage("logits")
    assert be.get_attention_storage() == "probs"               # a refused name changes nothing
    code = "import calm_vit_dte_amd as c; print('storage=' + c.backend.get_attention_storage())"
    for value, expect in (("lse", "lse"), ("probs", "probs"), (None, "probs")):
        env = {k: v for k, v in os.environ.items() if k != "CALM_ATTN_STORAGE"}
        if value is not None:
            env["CALM_ATTN_STORAGE"] = value
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert f"storage={expect}" in r.stdout
    env = dict(os.environ, CALM_ATTN_STORAGE="everything")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "unknown attention storage" in r.stderr


def _fn_args(B, S, H, hd, requires_grad=True):
    q, k, v, w1, b1, s1, w2, b2, s2 = _inputs(B, S, H, hd)
    leaves = [t.clone().requires_grad_(requires_grad) for t in (q, k, v, w1, b1, w2, b2)]
    q, k, v, w1, b1, w2, b2 = leaves
    g = torch.Generator().manual_seed(11)
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, generator=g), dim=0)   # noqa: E731
    u1, v1, u2, v2 = unit(2 * S), unit(S), unit(S), unit(2 * S)
    return leaves, (q, k, v, w1, b1, w2, b2, u1, v1, s1, u2, v2, s2, H)


def _run(fn, B, S, H, hd):
    leaves, args = _fn_args(B, S, H, hd)
    dout = torch.randn(B, S, H * hd, generator=torch.Generator().manual_seed(8))
    with calm.backend.use_backend(EmulatedLseBackend()):
        out = fn.apply(*args)
        out.backward(dout)
    return out.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("B,S,H,hd", [(2, 80, 6, 40), (2, 48, 3, 48)])
def test_lean_function_gives_the_output_and_the_seven_gradients_of_the_stored_one(B, S, H, hd):
    out_p, grads_p = _run(calm.ops.LatentMaskAttentionFn, B, S, H, hd)
    out_l, grads_l = _run(calm.ops.LatentMaskAttentionLseFn, B, S, H, hd)
    assert rel_err(out_l, out_p) < TOL
    for name, a, b in zip(("dq", "dk", "dv", "dW1", "db1", "dW2", "db2"), grads_l, grads_p):
        assert a is not None and b is not None, name
        assert torch.isfinite(a).all(), name
        assert rel_err(a, b) < TOL, name


def test_lean_function_saves_the_row_lse_and_nothing_of_the_size_of_the_probabilities():
    B, S, H, hd = 2, 80, 6, 40                                  # B*H*S*S = 76 800; B*S*2S = 25 600, 2S*S = 12 800
    big, small = B * H * S * S, B * H * S
    saved = {}
    for fn in (calm.ops.LatentMaskAttentionFn, calm.ops.LatentMaskAttentionLseFn):
        sizes = []
        _, args = _fn_args(B, S, H, hd)
        with calm.backend.use_backend(EmulatedLseBackend()), \
                torch.autograd.graph.saved_tensors_hooks(lambda t: (sizes.append(t.numel()), t)[1], lambda t: t):
            fn.apply(*args)
        saved[fn] = sizes
    stored, lean = saved[calm.ops.LatentMaskAttentionFn], saved[calm.ops.LatentMaskAttentionLseFn]
    assert big in stored                                        # the hook does see the probabilities where they are kept
    assert big not in lean and max(lean) < big
    assert small in lean and small not in stored
    assert B * S * S in lean                                    # the mask takes the place of the probabilities


def _nano_pass(storage):
    name = "nano48_cls"
    g = load_golden(name)
    cfg = CONFIGS[name]
    calm.backend.set_attention_storage(storage)
    m = build_model(name, g).train()
    x = torch.from_numpy(W.make_input((2, 3, cfg.seq_length, cfg.seq_length), 2)).requires_grad_(True)
    be = EmulatedLseBackend()
    calls = {"lse": [], "probs": []}
    fwd_lse, fwd = be.attn_fwd_lse, be.attn_fwd

    def count_lse(*a):
        calls["lse"].append(a[-4])                              # Sq
        return fwd_lse(*a)

    def count_probs(*a):
        if a[14] is not None:                                   # P asked for: the stored-P function's own call
            calls["probs"].append(a[-4])
        return fwd(*a)
    be.attn_fwd_lse, be.attn_fwd = count_lse, count_probs
    calm.ops.set_noise_override(W.NoiseStream(7))
    try:
        with calm.backend.use_backend(be):
            y, kl = m(x)
            gy = torch.from_numpy(W.make_input(tuple(y.shape), 3, "gy"))
            ((y * gy).sum() + 0.5 * kl).backward()
    finally:
        calm.ops.set_noise_override(None)
    return y.detach(), float(kl.detach()), x.grad, {n: p.grad for n, p in m.named_parameters()}, calls


def test_nano48_model_in_lse_mode_takes_the_fused_stage_lean_and_falls_back_elsewhere():
    y_p, kl_p, dx_p, grads_p, calls_p = _nano_pass("probs")
    y_l, kl_l, dx_l, grads_l, calls_l = _nano_pass("lse")
    assert not calls_p["lse"] and calls_p["probs"]
    assert calls_l["lse"] and set(calls_l["lse"]) == set(calls_p["probs"]) == {48}   # the fused stage, and only it
    assert not calls_l["probs"]
    assert rel_err(y_l, y_p) < TOL and abs(kl_l - kl_p) < TOL * max(1.0, abs(kl_p))
    assert rel_err(dx_l, dx_p) < TOL
    for n in grads_p:
        assert grads_l[n] is not None, n
        assert rel_err(grads_l[n], grads_p[n]) < TOL, n
    # and the lean run still meets the reference fixture like the stored one does
    g = load_golden("nano48_cls")
    assert rel_err(y_l, g["train/y"]) < 2e-5 and rel_err(dx_l, g["train/dx"]) < 1e-4
