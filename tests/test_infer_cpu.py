"""Lean inference forward on a host without a GPU: the two C-ABI additions are declared, exported and bound and refuse bad
arguments from host code, the switch behaves, VMLA_Block takes the lean path exactly when the switch is on and grad is
off, ops.latent_mask_attention_infer allocates the output and the mask scratch and nothing else, Predictor / evaluate
restore what they change — all over the torch emulation of the entry points (tests/emulated_infer.py) — and every GELU
GEMM of the four real-size configs plans one kernel instance with and without C_pre (calm_gemm_describe, host code)."""
import ctypes
import os
import re
import subprocess
import sys
from importlib import import_module

import pytest
import torch

import calm_vit_dte_amd as calm
import weights as W
from emulated_infer import EmulatedInferBackend
from helpers import CONFIGS, REAL_SIZE_CFGS, load_golden, load_inventory
from test_attention_gpu import SHAPES, _inputs
from test_host_logic_cpu import build_model

trainer = import_module("calm_vit_dte_amd.trainer")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "calm_vit.h")
NAMES = ("calm_attention_infer", "calm_attention16_infer")
# GELU GEMMs whose plan changes when C_pre is dropped: a lean forward keeps a scratch C_pre for them
KEEP_LIST = set()


@pytest.fixture(autouse=True)
def _restore_switch():
    prev = calm.backend.get_lean_inference()
    yield
    calm.backend.set_lean_inference(prev)
    calm.ops.set_noise_override(None)


def test_entry_points_are_declared_exported_and_bound_under_abi_7():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(calm_\w+)\s*\(", text, flags=re.M))
    lib = calm._lib.load()
    for n in NAMES:
        assert n in declared and n in calm._lib.SIGNATURES and hasattr(lib, n), n
    assert int(re.search(r"#define\s+CALM_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 7   # additions only
    assert len(calm._lib.SIGNATURES["calm_attention_infer"][1]) == 17
    assert len(calm._lib.SIGNATURES["calm_attention16_infer"][1]) == 16


def test_argument_refusals_come_from_host_code_before_any_launch():
    """A null tensor or B <= 0 is CALM_E_INVAL, a shape without an instantiation or B > 65535 is CALM_E_UNSUPP — answered
    before the stream is touched, so this runs without a GPU.  The addresses are fake and never dereferenced."""
    lib = calm._lib.load()
    INVAL, UNSUPP = calm._lib.E_INVAL, calm._lib.E_UNSUPP
    ptrs = [0x1000 * (i + 1) for i in range(11)]
    f32, f16 = lib.calm_attention_infer, lib.calm_attention16_infer
    for i in range(11):                                         # q k v w1 b1 s1 w2 b2 s2 out Mk
        bad = list(ptrs)
        bad[i] = None
        assert f32(*bad, 2, 80, 80, 6, 40, None) == INVAL, i
        assert f16(*bad, 2, 80, 6, 40, None) == INVAL, i
    for B in (0, -1):
        assert f32(*ptrs, B, 80, 80, 6, 40, None) == INVAL and f16(*ptrs, B, 80, 6, 40, None) == INVAL
    for Sq, Skv, H, hd in ((36, 36, 3, 36), (64, 64, 4, 24), (224, 176, 6, 112), (80, 80, 6, 42), (80, 80, 2, 132)):
        assert not lib.calm_attention_fwd_supported(Sq, Skv, H, hd)
        assert f32(*ptrs, 2, Sq, Skv, H, hd, None) == UNSUPP, (Sq, Skv, H, hd)
    for S, H, hd in ((36, 3, 36), (392, 3, 32), (80, 6, 42), (80, 2, 132)):
        assert not lib.calm_attention16_supported(S, H, hd)
        assert f16(*ptrs, 2, S, H, hd, None) == UNSUPP, (S, H, hd)
    assert f32(*ptrs, 65536, 80, 80, 6, 40, None) == UNSUPP and f16(*ptrs, 65536, 80, 6, 40, None) == UNSUPP


def test_switch_default_round_trip_and_environment():
    be = calm.backend
    if not os.environ.get("CALM_LEAN_INFERENCE"):
        assert be.get_lean_inference() is False
    be.set_lean_inference(True)
    assert be.get_lean_inference() is True
    with torch.no_grad():
        assert be.lean_forward()
    with torch.enable_grad():
        assert not be.lean_forward()                            # grad enabled: never, whatever the switch says
    be.set_lean_inference(False)
    with torch.no_grad():
        assert not be.lean_forward()
    code = "import calm_vit_dte_amd as c; print('lean=' + str(c.backend.get_lean_inference()))"
    for value, expect in (("1", True), ("0", False), (None, False)):
        env = {k: v for k, v in os.environ.items() if k != "CALM_LEAN_INFERENCE"}
        if value is not None:
            env["CALM_LEAN_INFERENCE"] = value
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert f"lean={expect}" in r.stdout


def _attn_args(B, S, H, hd):
    q, k, v, w1, b1, s1, w2, b2, s2 = _inputs(B, S, H, hd)
    return q, k, v, w1, b1, w2, b2, s1, s2, H


def _watch_empty(monkeypatch):
    shapes = []
    real = torch.empty

    def empty(*size, **kw):
        shapes.append(tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size))
        return real(*size, **kw)
    monkeypatch.setattr(torch, "empty", empty)
    return shapes


@pytest.mark.parametrize("B,S,H,hd", [(2, 80, 6, 40), (2, 48, 3, 48)])
def test_infer_op_equals_the_stored_forward_and_allocates_out_and_mask_only(monkeypatch, B, S, H, hd):
    be = EmulatedInferBackend()
    q, k, v, w1, b1, w2, b2, s1, s2, _ = args = _attn_args(B, S, H, hd)
    unit = torch.ones(1)
    with calm.backend.use_backend(be):
        ref = calm.ops.LatentMaskAttentionFn.apply(q, k, v, w1, b1, w2, b2, unit, unit, s1, unit, unit, s2, H)
        shapes = _watch_empty(monkeypatch)
        with torch.no_grad():
            out = calm.ops.latent_mask_attention_infer(*args)
    monkeypatch.undo()
    assert torch.equal(out, ref)
    assert sorted(shapes) == sorted([(B, S, H * hd), (B * S, S)])      # out, Mk: no R, hp, hg, P, lse
    assert [c[0] for c in be.calls] == ["attn_fwd", "attn_infer"]


def test_infer_op_takes_the_bf16_kernel_for_bf16_tensors_without_R_hp_hg_MkT(monkeypatch):
    B, S, H, hd = 2, 40, 3, 24
    be = EmulatedInferBackend()
    q, k, v, w1, b1, w2, b2, s1, s2, _ = _attn_args(B, S, H, hd)
    q, k, v = q.bfloat16(), k.bfloat16(), v.bfloat16()
    for w in (w1, w2):
        setattr(w, calm.spectral_norm.W16_ATTR, w.bfloat16())
    prev = calm.backend.get_matmul_precision()
    calm.backend.set_matmul_precision("bf16")
    try:
        unit = torch.ones(1)
        with calm.backend.use_backend(be):
            ref = calm.ops.LatentMaskAttention16Fn.apply(q, k, v, w1, b1, w2, b2, unit, unit, s1, unit, unit, s2, H)
            shapes = _watch_empty(monkeypatch)
            with torch.no_grad():
                out = calm.ops.latent_mask_attention_infer(q, k, v, w1, b1, w2, b2, s1, s2, H)
        monkeypatch.undo()
    finally:
        calm.backend.set_matmul_precision(prev)
    assert out.dtype == torch.bfloat16 and torch.equal(out, ref)
    assert sorted(shapes) == sorted([(B, S, H * hd), (B * S, S)])
    assert [c[0] for c in be.calls] == ["attn16_fwd", "attn16_infer"]


def test_infer_op_composes_unsupported_fp32_shapes_without_the_pre_activation(monkeypatch):
    B, S, H, hd = 2, 36, 3, 36                                   # Nano-48's inner stage: no fused instantiation
    be = EmulatedInferBackend()
    assert not be.attn_fwd_supported(S, S, H, hd)
    q, k, v, w1, b1, w2, b2, s1, s2, _ = args = _attn_args(B, S, H, hd)
    unit = torch.ones(1)
    calm.backend.set_lean_inference(True)
    with calm.backend.use_backend(be):
        ref = calm.ops.LatentMaskAttentionFn.apply(q, k, v, w1, b1, w2, b2, unit, unit, s1, unit, unit, s2, H)
        shapes = _watch_empty(monkeypatch)
        with torch.no_grad():
            out = calm.ops.latent_mask_attention_infer(*args)
    monkeypatch.undo()
    assert torch.equal(out, ref)
    assert shapes.count((B * S, 2 * S)) == 1                      # the hidden state feeds the next GEMM; hp is gone
    assert not any(c[0] in ("attn_infer", "attn_fwd") for c in be.calls)


def test_infer_op_refuses_to_run_where_autograd_would_record():
    q, k, v, w1, b1, w2, b2, s1, s2, H = _attn_args(2, 80, 6, 40)
    q.requires_grad_(True)
    with calm.backend.use_backend(EmulatedInferBackend()), pytest.raises(RuntimeError, match="no_grad"):
        calm.ops.latent_mask_attention_infer(q, k, v, w1, b1, w2, b2, s1, s2, H)


def _nano(be, lean, grad):
    name = "nano48_cls"
    cfg = CONFIGS[name]
    m = build_model(name, load_golden(name)).eval()
    x = torch.from_numpy(W.make_input((2, 3, cfg.seq_length, cfg.seq_length), 2))
    calm.backend.set_lean_inference(lean)
    with calm.backend.use_backend(be), torch.set_grad_enabled(grad):
        y, _ = m(x)
    return y.detach()


def test_model_takes_the_lean_path_only_with_the_switch_on_and_grad_off():
    taken = {}
    ys = {}
    for lean in (False, True):
        for grad in (False, True):
            be = EmulatedInferBackend()
            ys[lean, grad] = _nano(be, lean, grad)
            taken[lean, grad] = {c[0] for c in be.calls}
    assert taken[True, False] == {"attn_infer"}                  # the fused stage; the other stages are composed
    for key in ((False, False), (False, True), (True, True)):
        assert taken[key] == {"attn_fwd"}, key
    for key in ys:
        assert torch.equal(ys[key], ys[False, False]), key


def test_predictor_and_evaluate_are_lean_whatever_the_switch_and_restore_flag_and_switch():
    name = "nano48_cls"
    cfg = CONFIGS[name]
    m = build_model(name, load_golden(name)).train()
    x = torch.from_numpy(W.make_input((2, 3, cfg.seq_length, cfg.seq_length), 2))
    labels = torch.tensor([1, 3])
    be = EmulatedInferBackend()
    with calm.backend.use_backend(be):
        pred = trainer.Predictor(m)
        y, kl = pred(x)
        assert m.training and calm.backend.get_lean_inference() is False
        assert {c[0] for c in be.calls} == {"attn_infer"}
        m.eval()
        with torch.no_grad():
            y_ref, _ = m(x)
        assert torch.equal(y, y_ref) and not y.requires_grad
        m.train()
        acc = trainer.evaluate(m, [(x, labels)])
        del be.calls[:]
        assert trainer.evaluate(m, [(x, labels)], lean=True) == acc
        assert {c[0] for c in be.calls} == {"attn_infer"} and m.training
        with pytest.raises(ValueError, match="example_x"):
            trainer.Predictor(m, graph=True)
        pred.close()


# ---- calm_gemm_describe: the GELU launches of the real-size models plan one instance with and without C_pre ------------
def _gelu_gemm_shapes(name, batch):
    """(M, N, K) of every GELU forward GEMM of a config: the block MLPs (MlpFn), the mask MLP of the composed attention
    path and the classifier head, read off the state-dict inventory (mlp.0 [mlp_dim, dim], linear_mask.0 [2S, S])."""
    inv = load_inventory(name)
    shapes = set()
    for key, shp in inv.items():
        if key.endswith("linear_mask.0.weight_orig"):
            S = shp[1]
            shapes.add((batch * S, shp[0], S))                  # mask MLP: rows = tokens, K = keys
            mlp = inv.get(key.replace("linear_mask.0", "mlp.0"))
            if mlp is not None:
                shapes.add((batch * S, mlp[0], mlp[1]))
        elif re.search(r"(^|\.)head\.0\.weight_orig$", key) or key.endswith("cls_head.0.weight_orig"):
            shapes.add((batch, shp[0], shp[1]))
    return sorted(shapes)


def _plan(lib, M, N, K, st, dtype, with_pre):
    b = calm._lib
    g = b.GemmArgs()
    g.A, g.B, g.C = 0x100000, 0x200000, 0x300000
    g.bias = 0x500000
    g.inv_scale = 0x600000
    g.M, g.N, g.K = M, N, K
    g.a_rs, g.a_cs, g.b_rs, g.b_cs, g.c_rs, g.r_rs = K, 1, K, 1, N, N
    g.batch0 = g.batch1 = 1
    g.alpha = 1.0
    g.dtype = dtype
    g.a_type = g.b_type = g.c_type = st
    g.act = b.ACT_GELU
    g.split_k = 1
    if with_pre:
        g.C_pre = 0x400000
    plan = b.GemmPlan()
    rc = lib.calm_gemm_describe(ctypes.byref(g), ctypes.byref(plan))
    return rc, tuple(getattr(plan, n) for n, _ in b.GemmPlan._fields_)


@pytest.mark.parametrize("name", REAL_SIZE_CFGS)
def test_gelu_gemms_of_the_real_size_configs_plan_one_instance_with_and_without_c_pre(name):
    lib = calm._lib.load()
    b = calm._lib
    shapes = [s for batch in (1, 8, 256) for s in _gelu_gemm_shapes(name, batch)]
    assert len(shapes) >= 12, shapes
    differ = set()
    for M, N, K in shapes:
        for st, dtype in ((b.ST_F32, 0), (b.ST_BF16, 1)):
            if st == b.ST_BF16 and (K % 8 or N % 8):
                continue                                        # bf16 tensors need 16-byte rows: such a launch runs on fp32
            with_pre, without = _plan(lib, M, N, K, st, dtype, True), _plan(lib, M, N, K, st, dtype, False)
            assert with_pre[0] == 0 and without[0] == 0, (M, N, K, st)
            if with_pre != without:
                differ.add((M, N, K, st))
    assert differ <= KEEP_LIST, sorted(differ - KEEP_LIST)


def test_pre_activation_is_dropped_only_without_grad_and_training_with_the_switch_on_still_trains():
    """Inside autograd.Function.forward grad mode is always off, so whether a forward is lean is decided where apply()
    is called: with grad enabled every GELU GEMM still gets its C_pre and the backward runs, switch on or off."""
    name = "nano48_cls"
    cfg = CONFIGS[name]
    g = load_golden(name)
    x0 = torch.from_numpy(W.make_input((2, 3, cfg.seq_length, cfg.seq_length), 2))
    seen, grads = {}, {}
    for lean in (False, True):
        for grad in (False, True):
            be = EmulatedInferBackend()
            pres = []
            real = be.gemm

            def gemm(*a, _real=real, _pres=pres, **kw):
                if kw.get("act") == calm.backend.ACT_GELU:
                    _pres.append(kw.get("C_pre") is not None)
                return _real(*a, **kw)
            be.gemm = gemm
            m = build_model(name, g).train()
            x = x0.clone().requires_grad_(grad)
            calm.backend.set_lean_inference(lean)
            calm.ops.set_noise_override(W.NoiseStream(7))
            with calm.backend.use_backend(be), torch.set_grad_enabled(grad):
                y, kl = m(x)
                if grad:
                    ((y * y).sum() + 0.5 * kl).backward()
                    grads[lean] = [x.grad] + [p.grad for p in m.parameters()]
            calm.ops.set_noise_override(None)
            seen[lean, grad] = pres
    assert seen[True, False] and not any(seen[True, False])           # lean: no GELU launch keeps a pre-activation
    for key in ((False, False), (False, True), (True, True)):
        assert seen[key] and all(seen[key]), key
    assert all(a is not None and torch.equal(a, b) for a, b in zip(grads[True], grads[False]))
