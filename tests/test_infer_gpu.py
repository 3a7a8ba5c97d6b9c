"""Lean inference forward on the MI355X: calm_attention_infer / calm_attention16_infer against the stored forwards they
are cut from (bit equality of out and Mk, guard bands, every instance of both bf16 kernel generations), what
ops.latent_mask_attention_infer allocates, the switch in the model (logits bit for bit, gradients untouched) and
trainer.Predictor / evaluate (graph replay against the eager lean forward).

The reference everywhere is the stored forward of the same build on the same inputs, compared with torch.equal on the
bit patterns: the lean kernels are the stored kernels with stores compiled out, so any difference at all is a defect.
The stored forwards themselves are tested against float64 in test_attention16_f64_gpu.py / test_attention_gpu.py.

Memory case (fp32, B=8, S=224, H=12, hd=56), counted from the shapes: out 4 816 896 + Mk 1 605 632 bytes; the stored
forward adds R, hp, hg, P = 4 (5 + H) S^2 B = 27 295 744 bytes, 33.7 MB in all (the issue's "34 MB")."""
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import attn16_f64 as A
import weights as W
from helpers import CONFIGS, load_golden, rel_err
from test_attention16_f64_gpu import B_SWEEP, H_SWEEP, fenced
from test_attention_gpu import SHAPES, _inputs
from test_host_logic_cpu import build_model
from test_rowwise_f64_gpu import Out

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
ops = calm.ops
DEV = "cuda"
TOL = 1e-3                                    # the project's fp32 tolerance against the reference fixtures

# bf16: one shape per compiled (NP, HDP) instance and the extras at the B and H of test_attention16_f64_gpu.py; with
# H = 3 the shapes with hd % 8 == 4 have D % 8 == 4 and take the register-staged kernel, so the 14 pipelined-capable
# instances run once more with H = 4 (D % 8 == 0: the pipelined kernel for certain)
SWEEP16 = [(S, H_SWEEP, hd) for S, hd in dict.fromkeys(A.sweep_cases() + A.EXTRA_SHAPES)]    # ((64, 64) is in both lists)
PIPELINED16 = [(S, H, hd) for S, hd in A.sweep_cases() if A.pipelined_capable(S, hd) for H in (H_SWEEP, 4)]
CASES16 = SWEEP16 + [c for c in PIPELINED16 if c[1] == 4]
ids16 = lambda cases: [f"{S}-{H}-{hd}" for S, H, hd in cases]      # noqa: E731


@pytest.fixture(scope="module")
def hip():
    return calm.backend.get_backend()


@pytest.fixture(autouse=True)
def _restore_switch():
    prev = calm.backend.get_lean_inference()
    yield
    calm.backend.set_lean_inference(prev)
    ops.set_noise_override(None)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------------------------------------------ fp32 kernel
@pytest.mark.parametrize("B,S,H,hd", SHAPES)
def test_fp32_infer_equals_the_stored_forward_bit_for_bit_inside_guards(hip, B, S, H, hd):
    assert hip.attn_fwd_supported(S, S, H, hd)
    t = [x.to(DEV) for x in _inputs(B, S, H, hd)]
    D = H * hd
    e = lambda *s: torch.empty(*s, device=DEV)
    out, Mk = e(B, S, D), e(B, S, S)
    hip.attn_fwd(*t, out, e(B, S, S), e(B, S, 2 * S), e(B, S, 2 * S), Mk, e(B, H, S, S), B, S, S, H, hd)
    lean_out, lean_Mk = Out((B, S, D)), Out((B, S, S))
    hip.attn_infer(*t, lean_out.t, lean_Mk.t, B, S, S, H, hd)
    torch.cuda.synchronize()
    got_out, got_Mk = lean_out.check(), lean_Mk.check()          # guards intact, every element written
    assert torch.isfinite(got_out).all()
    assert torch.equal(bits(got_out), bits(out.cpu())) and torch.equal(bits(got_Mk), bits(Mk.cpu()))


def test_fp32_infer_reports_unsupported_shapes_without_writing(hip):
    for B, S, H, hd in ((1, 36, 3, 36), (1, 64, 4, 24)):
        assert not hip.attn_fwd_supported(S, S, H, hd)
        t = [x.to(DEV) for x in _inputs(B, S, H, hd)]
        out, Mk = Out((B, S, H * hd)), Out((B, S, S))
        with pytest.raises(RuntimeError, match="calm_attention_infer failed: code -3"):
            hip.attn_infer(*t, out.t, Mk.t, B, S, S, H, hd)
        torch.cuda.synchronize()
        for o in (out, Mk):
            o.check(written=False)
            assert torch.equal(bits(o.buf).cpu(), o.before)       # nothing ran
    t = [x.to(DEV) for x in _inputs(1, 80, 6, 40)]
    with pytest.raises(ValueError):
        hip.attn_infer(*t[:9], torch.empty(1, 80, 240, device=DEV), None, 1, 80, 80, 6, 40)


# ------------------------------------------------------------------------------------------------------ bf16 kernels
def _bf16_case(hip, S, H, hd):
    B = B_SWEEP
    assert hip.attn16_supported(S, H, hd)
    D = H * hd
    ins, _ = A.make_inputs(B, S, H, hd, seed=S + hd)
    dev = [fenced(t) if t.numel() > 1 else t.to(DEV) for t in ins]
    bf = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=DEV)
    out, Mk = bf(B, S, D), bf(B, S, S)
    hip.attn16_fwd(*dev, out, bf(B, S, S), bf(B, S, 2 * S), bf(B, S, 2 * S), Mk, bf(B, S, S),
                   torch.empty(B, H, S, device=DEV), B, S, H, hd)
    lean_out, lean_Mk = Out((B, S, D), torch.bfloat16), Out((B, S, S), torch.bfloat16)
    hip.attn16_infer(*dev, lean_out.t, lean_Mk.t, B, S, H, hd)
    torch.cuda.synchronize()
    got_out, got_Mk = lean_out.check(), lean_Mk.check()
    assert torch.isfinite(got_out.float()).all() and torch.isfinite(got_Mk.float()).all()
    assert torch.equal(bits(got_out), bits(out.cpu())) and torch.equal(bits(got_Mk), bits(Mk.cpu()))


@pytest.mark.parametrize("S,H,hd", CASES16, ids=ids16(CASES16))
def test_bf16_infer_equals_the_stored_forward_bit_for_bit_inside_guards(hip, S, H, hd):
    """Every compiled (NP, HDP) instance and the extra shapes.  Under CALM_ATTN16_V2=0 (the child of the test below) the
    same node ids run the register-staged kernels."""
    _bf16_case(hip, S, H, hd)


def test_bf16_infer_on_the_register_staged_kernels_of_the_pipelined_instances_in_a_child_process():
    """CALM_ATTN16_V2=0 is read once per process, hence one fresh child (no retry): the 14 pipelined-capable instances at
    H = 3 and H = 4, 28 runs, stored and lean both on attn16_fwd_kernel (launch_fwd16_t: k1 stays null)."""
    assert len(PIPELINED16) == 28
    here = os.path.abspath(__file__)
    name = "test_bf16_infer_equals_the_stored_forward_bit_for_bit_inside_guards"
    nodes = [f"{here}::{name}[{i}]" for i in ids16(PIPELINED16)]
    env = dict(os.environ, CALM_ATTN16_V2="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x"] + nodes, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and f"{len(nodes)} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


def test_bf16_infer_never_takes_the_experimental_v3_pair_in_a_child_process():
    """With CALM_ATTN16_V3=1 the stored forward runs the v3 pair (un-normalised probabilities rounded: other bits) while
    the lean one keeps the pipelined kernel — so lean under V3=1 must equal the stored forward of THIS process."""
    S, H, hd = 80, 4, 20
    ins, _ = A.make_inputs(2, S, H, hd, seed=3)
    dev = [t.to(DEV) for t in ins]
    bf = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=DEV)
    out, Mk = bf(2, S, H * hd), bf(2, S, S)
    calm.backend.get_backend().attn16_fwd(*dev, out, bf(2, S, S), bf(2, S, 2 * S), bf(2, S, 2 * S), Mk, bf(2, S, S),
                                          torch.empty(2, H, S, device=DEV), 2, S, H, hd)
    torch.cuda.synchronize()
    code = ("import sys, torch; sys.path[:0] = [%r, %r]\n"
            "import calm_vit_dte_amd as calm, attn16_f64 as A\n"
            "ins, _ = A.make_inputs(2, %d, %d, %d, seed=3)\n"
            "dev = [t.cuda() for t in ins]\n"
            "bf = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device='cuda')\n"
            "out, Mk = bf(2, %d, %d), bf(2, %d, %d)\n"
            "calm.backend.get_backend().attn16_infer(*dev, out, Mk, 2, %d, %d, %d)\n"
            "torch.cuda.synchronize()\n"
            "print('BITS', out.view(torch.int16).cpu().numpy().tobytes().hex())\n"
            % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)),
               S, H, hd, S, H * hd, S, S, S, H, hd))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CALM_ATTN16_V3="1"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [ln for ln in r.stdout.splitlines() if ln.startswith("BITS ")][0][5:]
    assert got == out.view(torch.int16).cpu().numpy().tobytes().hex()


# ------------------------------------------------------------------------------------------------------------ memory
def test_infer_op_peak_allocation_is_out_plus_mask():
    B, S, H, hd = 8, 224, 12, 56
    D = H * hd
    q, k, v, w1, b1, s1, w2, b2, s2 = [x.to(DEV) for x in _inputs(B, S, H, hd)]
    unit = torch.ones(1, device=DEV)
    out_b, mk_b, saved_b = 4 * B * S * D, 4 * B * S * S, 4 * (5 + H) * S * S * B
    slack = 4 << 20
    peaks = {}
    with torch.no_grad():
        for form in ("lean", "stored"):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            if form == "lean":
                out = ops.latent_mask_attention_infer(q, k, v, w1, b1, w2, b2, s1, s2, H)
            else:
                out = ops.LatentMaskAttentionFn.apply(q, k, v, w1, b1, w2, b2, unit, unit, s1, unit, unit, s2, H)
            torch.cuda.synchronize()
            peaks[form] = torch.cuda.max_memory_allocated() - base
            del out
    print(f"\n[infer memory] lean peak {peaks['lean']} stored peak {peaks['stored']} bytes")
    assert peaks["lean"] <= out_b + mk_b + slack, peaks                   # 6 422 528 + 4 MiB = 10.6 MB
    assert peaks["stored"] >= out_b + mk_b + saved_b, peaks               # 33.7 MB


# ------------------------------------------------------------------------------------------------------------- model
def _eval_logits(m, x, lean, autocast):
    calm.backend.set_lean_inference(lean)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y, kl = m(x)
    torch.cuda.synchronize()
    return y.detach().clone(), torch.as_tensor(kl).detach().clone()


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["nano48_cls", "tiny32_cls"])
def test_model_logits_with_the_switch_on_equal_those_with_it_off(name, autocast):
    g = load_golden(name)
    cfg = CONFIGS[name]
    m = build_model(name, g, "cuda").eval()
    x = torch.from_numpy(W.make_input((2, 3, cfg.seq_length, cfg.seq_length), 2)).cuda()
    lean_calls = []
    be = calm.backend.get_backend()
    real32, real16 = be.attn_infer, be.attn16_infer
    be.attn_infer = lambda *a: (lean_calls.append("fp32"), real32(*a))[1]
    be.attn16_infer = lambda *a: (lean_calls.append("bf16"), real16(*a))[1]
    try:
        y_off, kl_off = _eval_logits(m, x, False, autocast)
        assert not lean_calls
        y_on, kl_on = _eval_logits(m, x, True, autocast)
    finally:
        del be.attn_infer, be.attn16_infer
    assert lean_calls                                                    # the lean kernels did run
    assert torch.equal(bits(y_on), bits(y_off)) and torch.equal(kl_on, kl_off)
    if not autocast:
        assert rel_err(y_on, g["eval/y"]) < TOL


@pytest.mark.parametrize("name", ["nano48_cls", "tiny32_cls"])
def test_gradients_do_not_depend_on_the_switch(name):
    """Grad enabled: the switch changes nothing.  k-split weight gradients through the fixed-order workspace reduction
    (GEMM_OPT_DETERMINISTIC), as in test_determinism_gpu.py, so that two runs can be compared bit for bit at all."""
    g = load_golden(name)
    cfg = CONFIGS[name]
    be = calm.backend.get_backend()
    prev = be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, 1)
    runs = []
    try:
        for lean in (False, True):
            calm.backend.set_lean_inference(lean)
            m = build_model(name, g, "cuda").train()
            x = torch.from_numpy(W.make_input((2, 3, cfg.seq_length, cfg.seq_length), 2)).cuda().requires_grad_(True)
            ops.set_noise_override(W.NoiseStream(7))
            y, kl = m(x)
            gy = torch.from_numpy(W.make_input(tuple(y.shape), 3, "gy")).cuda()
            ((y * gy).sum() + 0.5 * kl).backward()
            ops.set_noise_override(None)
            torch.cuda.synchronize()
            runs.append((y.detach(), x.grad, {n: p.grad for n, p in m.named_parameters()}))
    finally:
        be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, prev)
    (y0, dx0, g0), (y1, dx1, g1) = runs
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    differing = [n for n in g0 if g1[n] is None or not torch.equal(g0[n], g1[n])]
    assert not differing, differing[:8]
    assert rel_err(y1, g["train/y"]) < TOL and rel_err(dx1, g["train/dx"]) < TOL


# --------------------------------------------------------------------------------------------------------- Predictor
def _batches(cfg, n, bs, seed=5):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.standard_normal((bs, 3, cfg.seq_length, cfg.seq_length)).astype(np.float32)).cuda()
            for _ in range(n)]


@pytest.mark.parametrize("autocast", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_predictor_graph_replay_equals_eager_lean_and_sees_weight_updates(autocast):
    name = "nano48_cls"
    cfg = CONFIGS[name]
    m = build_model(name, load_golden(name), "cuda").train()
    xs = _batches(cfg, 3, 4)
    eager = trainer.Predictor(m, autocast_dtype=autocast)
    graphed = trainer.Predictor(m, example_x=xs[0], autocast_dtype=autocast, graph=True)
    assert graphed.graph is not None and m.training and calm.backend.get_lean_inference() is False
    for x in xs:
        (y_g, _), (y_e, _) = graphed(x), eager(x)
        assert torch.equal(bits(y_g), bits(y_e))
    first = graphed(xs[0])[0]
    with torch.no_grad():                                           # an in-place update, as an optimizer step makes
        for p in m.parameters():
            p.mul_(1.03125)
    (y_g, _), (y_e, _) = graphed(xs[0]), eager(xs[0])
    assert torch.equal(bits(y_g), bits(y_e)) and not torch.equal(y_g, first)
    ragged = xs[1][:3]                                              # another shape: eagerly, lean
    replays = []
    real = graphed.graph.replay
    graphed.graph.replay = lambda: (replays.append(1), real())[1]
    assert torch.equal(bits(graphed(ragged)[0]), bits(eager(ragged)[0])) and not replays
    graphed(xs[2])
    assert replays == [1]
    graphed.close()
    assert graphed.graph is None
    assert torch.equal(bits(graphed(xs[2])[0]), bits(eager(xs[2])[0]))
    assert m.training and calm.backend.get_lean_inference() is False


def test_evaluate_lean_graph_returns_the_accuracy_of_evaluate():
    name = "nano48_cls"
    cfg = CONFIGS[name]
    m = build_model(name, load_golden(name), "cuda").train()
    xs = _batches(cfg, 3, 4, seed=9)
    xs[-1] = xs[-1][:3]                                             # a ragged last batch
    with torch.no_grad():
        m.eval()
        labels = [m(x)[0].reshape(x.shape[0], -1).argmax(dim=1) for x in xs]
        m.train()
    labels[1] = (labels[1] + 1) % cfg.out_features                  # some misses
    data = list(zip(xs, labels))
    acc = trainer.evaluate(m, data)
    assert 0.0 < acc < 1.0
    assert trainer.evaluate(m, data, lean=True) == acc
    assert trainer.evaluate(m, data, lean=True, graph=True) == acc
    assert trainer.evaluate(m, data, graph=True, autocast_dtype=None) == acc
    assert m.training and calm.backend.get_lean_inference() is False
