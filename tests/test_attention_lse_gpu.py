"""Row-LSE mode of the fp32 attention on the MI355X, through the C-ABI (calm_attention_fwd_lse /
calm_attention_bwd_lse) at the ten shapes of tests/test_attention_gpu.py, then at function, model and training-step
level.  References are float64 on the CPU; tolerances are the project's: 1e-4 for a kernel, 1e-3 for a model against
its reference fixture."""
import math
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import weights as W
from helpers import CONFIGS, load_golden, rel_err, rel_err_elem
from test_attention_gpu import SHAPES, _inputs, rnd
from test_host_logic_cpu import build_model

pytestmark = pytest.mark.gpu
TOL = 1e-4                    # fp32 kernel against float64 (the tolerance of tests/test_attention_gpu.py)
MODEL_TOL = 1e-3              # north_star: 1e-3 rel fp32 (tests/test_realsize_gpu.py)
trainer = import_module("calm_vit_dte_amd.trainer")


@pytest.fixture(autouse=True)
def _restore_mode():
    prev = calm.backend.get_attention_storage()
    yield
    calm.backend.set_attention_storage(prev)
    calm.ops.set_noise_override(None)


def _reference64(ins, dout, B, S, H, hd):
    """The attention of Vi_Tools:288-299 and the backward of its core in float64: (out, R, hp, hg, Mk, lse) and
    (dq, dk, dv, dM)."""
    q, k, v, w1, b1, s1, w2, b2, s2 = (t.double() for t in ins)
    D = H * hd
    raw = q @ k.transpose(1, 2)
    pre = raw @ (w1 / s1).t() + b1
    act = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
    mask = act @ (w2 / s2).t() + b2
    qh, kh, vh = (t.view(B, S, H, hd).transpose(1, 2) for t in (q, k, v))
    sc = 1.0 / math.sqrt(hd)
    logits = qh @ kh.transpose(-1, -2) * sc + mask[:, None]
    lse = torch.logsumexp(logits, dim=-1)
    P = torch.exp(logits - lse[..., None])
    out = (P @ vh).transpose(1, 2).reshape(B, S, D)
    doh = dout.double().view(B, S, H, hd).transpose(1, 2)
    dP = doh @ vh.transpose(-1, -2)
    dS = P * (dP - (P * dP).sum(dim=-1, keepdim=True))
    back = lambda t: t.transpose(1, 2).reshape(B, S, D)   # noqa: E731
    grads = (back(dS @ kh * sc), back(dS.transpose(-1, -2) @ qh * sc), back(P.transpose(-1, -2) @ doh), dS.sum(dim=1))
    return (out, raw, pre, act, mask, lse), grads


def _forward_lse(hip, t, B, S, H, hd, fill=None):
    D = H * hd
    e = (lambda *s: torch.full(s, fill, device="cuda")) if fill is not None else (lambda *s: torch.empty(*s, device="cuda"))
    out, R, hp, hg, Mk, lse = e(B, S, D), e(B, S, S), e(B, S, 2 * S), e(B, S, 2 * S), e(B, S, S), e(B, H, S)
    hip.attn_fwd_lse(*t, out, R, hp, hg, Mk, lse, B, S, S, H, hd)
    return out, R, hp, hg, Mk, lse


def _backward_lse(hip, q, k, v, dout, Mk, lse, B, S, H, hd):
    """Every output and the scratch start as NaN: whatever the call does not write shows."""
    D = H * hd
    e = lambda *s: torch.full(s, float("nan"), device="cuda")   # noqa: E731
    need = hip.attn_bwd_lse_scratch_bytes(B, S, S, H, hd)
    assert need > 0 and need % 4 == 0
    scratch = e(need // 4)
    dq, dk, dv, dM = e(B, S, D), e(B, S, D), e(B, S, D), e(B, S, S)
    hip.attn_bwd_lse(q, k, v, dout, Mk, lse, scratch, dq, dk, dv, dM, B, S, S, H, hd)
    return dq, dk, dv, dM


@pytest.mark.parametrize("B,S,H,hd", SHAPES)
def test_forward_is_bit_identical_to_the_stored_one_and_the_lse_matches_float64(B, S, H, hd):
    hip = calm.backend.get_backend()
    ins = _inputs(B, S, H, hd)
    t = [x.cuda() for x in ins]
    D = H * hd
    e = lambda *s: torch.empty(*s, device="cuda")   # noqa: E731
    stored = (e(B, S, D), e(B, S, S), e(B, S, 2 * S), e(B, S, 2 * S), e(B, S, S))
    hip.attn_fwd(*t, *stored, e(B, H, S, S), B, S, S, H, hd)
    lean = _forward_lse(hip, t, B, S, H, hd, fill=float("nan"))
    for name, a, b in zip(("out", "R", "hp", "hg", "Mk"), lean, stored):
        assert torch.equal(a, b), name
    ref, _ = _reference64(ins, torch.zeros(B, S, D), B, S, H, hd)
    lse = lean[5].double().cpu()
    assert torch.isfinite(lse).all()
    err = float((lse - ref[5]).abs().max() / ref[5].abs().max())
    print(f"\n[{B},{S},{H},{hd}] lse err {err:.2e}  out err {rel_err(lean[0], ref[0]):.2e}")
    assert err < TOL


@pytest.mark.parametrize("B,S,H,hd", SHAPES)
def test_backward_from_the_lean_forward_matches_float64(B, S, H, hd):
    """dq, dk, dv, dM of calm_attention_bwd_lse on P-consistent inputs (Mk and lse from the lean forward of the same
    q, k) against float64, 1e-4.  Margin: the same arithmetic (P recomputed from the LSE) in fp32 on a CPU, at eight of
    these shapes with the `_inputs` recipe, is at most 3.4e-6 from float64 (dq at (2,128,6,64); out <= 3.2e-6,
    lse <= 5.0e-7), so 1e-4 leaves about 30x; the GPU's fast exponential adds about 1e-6 relative."""
    hip = calm.backend.get_backend()
    ins = _inputs(B, S, H, hd)
    dout = rnd(B, S, H * hd, seed=8)
    t = [x.cuda() for x in ins]
    out, R, hp, hg, Mk, lse = _forward_lse(hip, t, B, S, H, hd)
    got = _backward_lse(hip, t[0], t[1], t[2], dout.cuda(), Mk, lse, B, S, H, hd)
    _, want = _reference64(ins, dout, B, S, H, hd)
    errs = {n: rel_err(a, b) for n, a, b in zip(("dq", "dk", "dv", "dM"), got, want)}
    print(f"\n[{B},{S},{H},{hd}] " + "  ".join(f"{n} {v:.2e}" for n, v in errs.items()))
    for n, a in zip(("dq", "dk", "dv", "dM"), got):
        assert torch.isfinite(a).all(), n
        assert errs[n] < TOL, (n, errs[n])


@pytest.mark.parametrize("B,S,H,hd", SHAPES)
def test_backward_repeats_bit_for_bit(B, S, H, hd):
    hip = calm.backend.get_backend()
    t = [x.cuda() for x in _inputs(B, S, H, hd)]
    dout = rnd(B, S, H * hd, seed=8).cuda()
    out, R, hp, hg, Mk, lse = _forward_lse(hip, t, B, S, H, hd)
    first = _backward_lse(hip, t[0], t[1], t[2], dout, Mk, lse, B, S, H, hd)
    second = _backward_lse(hip, t[0], t[1], t[2], dout, Mk, lse, B, S, H, hd)
    for n, a, b in zip(("dq", "dk", "dv", "dM"), first, second):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("B,S,H,hd", SHAPES)
def test_a_nan_in_q_reaches_dq(B, S, H, hd):
    """GradScaler's inf check relies on non-finite values travelling through the backward."""
    hip = calm.backend.get_backend()
    t = [x.cuda() for x in _inputs(B, S, H, hd)]
    dout = rnd(B, S, H * hd, seed=8).cuda()
    b, i, c = B - 1, S // 2 + 1, (H * hd) // 3
    t[0][b, i, c] = float("nan")
    out, R, hp, hg, Mk, lse = _forward_lse(hip, t, B, S, H, hd)
    dq, dk, dv, dM = _backward_lse(hip, t[0], t[1], t[2], dout, Mk, lse, B, S, H, hd)
    assert not torch.isfinite(dq[b, i]).all()
    assert not torch.isfinite(dq).all()


def test_unsupported_shapes_and_a_short_scratch_are_refused_not_run():
    hip = calm.backend.get_backend()
    e = lambda *s: torch.empty(*s, device="cuda")   # noqa: E731
    for B, S, H, hd in ((1, 36, 3, 36), (1, 64, 4, 24)):
        D = H * hd
        assert hip.attn_bwd_lse_scratch_bytes(B, S, S, H, hd) == 0
        t = [x.cuda() for x in _inputs(B, S, H, hd)]
        with pytest.raises(RuntimeError, match="calm_attention_fwd_lse"):
            hip.attn_fwd_lse(*t, e(B, S, D), e(B, S, S), e(B, S, 2 * S), e(B, S, 2 * S), e(B, S, S), e(B, H, S),
                             B, S, S, H, hd)
        with pytest.raises(RuntimeError, match="calm_attention_bwd_lse"):
            hip.attn_bwd_lse(t[0], t[1], t[2], e(B, S, D), e(B, S, S), e(B, H, S), e(2 * B * H * S * S), e(B, S, D),
                             e(B, S, D), e(B, S, D), e(B, S, S), B, S, S, H, hd)
    assert hip.attn_bwd_lse_scratch_bytes(2, 224, 176, 6, 112) == 0
    # a supported shape with less scratch than the query asks for: CALM_E_INVAL (-1), nothing launched, nothing written
    B, S, H, hd = 2, 80, 6, 40
    D = H * hd
    t = [x.cuda() for x in _inputs(B, S, H, hd)]
    out, R, hp, hg, Mk, lse = _forward_lse(hip, t, B, S, H, hd)
    need = hip.attn_bwd_lse_scratch_bytes(B, S, S, H, hd)
    short = torch.empty(need - 4, dtype=torch.uint8, device="cuda")
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")   # noqa: E731
    dq, dk, dv, dM = nan(B, S, D), nan(B, S, D), nan(B, S, D), nan(B, S, S)
    with pytest.raises(RuntimeError, match=r"calm_attention_bwd_lse failed: code -1 "):
        hip.attn_bwd_lse(t[0], t[1], t[2], e(B, S, D), Mk, lse, short, dq, dk, dv, dM, B, S, S, H, hd)
    torch.cuda.synchronize()
    assert all(torch.isnan(x).all() for x in (dq, dk, dv, dM))


def _fn_args(B, S, H, hd):
    q, k, v, w1, b1, s1, w2, b2, s2 = (x.cuda() for x in _inputs(B, S, H, hd))
    leaves = [x.requires_grad_(True) for x in (q, k, v, w1, b1, w2, b2)]
    g = torch.Generator().manual_seed(11)
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, generator=g), dim=0).cuda()   # noqa: E731
    u1, v1, u2, v2 = unit(2 * S), unit(S), unit(S), unit(2 * S)
    return leaves, (q, k, v, w1, b1, w2, b2, u1, v1, s1, u2, v2, s2, H)


@pytest.mark.parametrize("B,S,H,hd", [(2, 224, 6, 112), (2, 128, 6, 64), (2, 80, 12, 20)])
def test_lean_function_gives_the_gradients_of_the_stored_one(B, S, H, hd):
    dout = rnd(B, S, H * hd, seed=8).cuda()
    res = []
    for fn in (calm.ops.LatentMaskAttentionFn, calm.ops.LatentMaskAttentionLseFn):
        leaves, args = _fn_args(B, S, H, hd)
        out = fn.apply(*args)
        out.backward(dout)
        res.append((out.detach(), [x.grad for x in leaves]))
    assert torch.equal(res[0][0], res[1][0])                     # the forward does not move with the mode
    for n, a, b in zip(("dq", "dk", "dv", "dW1", "db1", "dW2", "db2"), res[1][1], res[0][1]):
        assert rel_err(a, b) < TOL, n


def test_memory_held_between_forward_and_backward():
    """Growth of the caching allocator's live bytes over each function's forward, output alive: stored minus lean is
    bytes(P) - bytes(Mk) - bytes(lse) up to the allocator's 512-byte rounding of every saved tensor.

    The figure compared is the allocator's `requested_bytes` counter, not torch.cuda.memory_allocated(): the latter
    counts whole blocks, and the allocator hands a request of 1 MiB or more a free block up to 1 MiB larger without
    splitting it.  Measured on MI355X at this shape that block overhead was 819 200 bytes on the stored side and
    720 896 on the lean side (memory_allocated: 23 298 048 / 15 214 592, difference 8 083 456 against the 7 985 152
    expected — 98 304 bytes of unsplit remainders, none of them the functions' doing).  Both figures are printed."""
    B, S, H, hd = 8, 224, 6, 112
    live = lambda: torch.cuda.memory_stats()["requested_bytes.all.current"]   # noqa: E731
    held, blocks, n_saved = {}, {}, {}
    for fn in (calm.ops.LatentMaskAttentionFn, calm.ops.LatentMaskAttentionLseFn):
        leaves, args = _fn_args(B, S, H, hd)
        count = []
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before, before_blocks = live(), torch.cuda.memory_allocated()
        with torch.autograd.graph.saved_tensors_hooks(lambda t: (count.append(1), t)[1], lambda t: t):
            out = fn.apply(*args)
        torch.cuda.synchronize()
        held[fn], blocks[fn] = live() - before, torch.cuda.memory_allocated() - before_blocks
        n_saved[fn] = len(count)
        del out, leaves, args
    stored, lean = held[calm.ops.LatentMaskAttentionFn], held[calm.ops.LatentMaskAttentionLseFn]
    want = 4 * (B * H * S * S - B * S * S - B * H * S)
    slack = 512 * (n_saved[calm.ops.LatentMaskAttentionFn] + n_saved[calm.ops.LatentMaskAttentionLseFn])
    print(f"\nrequested: stored {stored} lean {lean} difference {stored - lean} expected {want} slack {slack}; "
          f"memory_allocated: stored {blocks[calm.ops.LatentMaskAttentionFn]} lean {blocks[calm.ops.LatentMaskAttentionLseFn]}")
    assert abs((stored - lean) - want) <= slack
    assert blocks[calm.ops.LatentMaskAttentionLseFn] < blocks[calm.ops.LatentMaskAttentionFn]


def _check_against_fixture(name, fixture, bs):
    """The checks of tests/test_realsize_gpu.py::test_full_model_fp32_matches_reference_fixture, in 'lse' mode."""
    g = load_golden(fixture)
    cfg = CONFIGS[name]
    S = cfg.seq_length
    calm.backend.set_attention_storage("lse")
    lean_calls = []
    be = calm.backend.get_backend()
    real = be.attn_fwd_lse
    m = build_model(name, g, "cuda").eval()
    x = torch.from_numpy(W.make_input((bs, 3, S, S), 2)).cuda()
    with torch.no_grad():
        y, kl = m(x)
    assert rel_err(y, g["eval/y"]) < MODEL_TOL
    assert rel_err_elem(y, g["eval/y"]) < MODEL_TOL
    assert abs(float(kl) - float(g["eval/kl"])) < MODEL_TOL * max(1.0, abs(float(g["eval/kl"])))
    m.train()
    x = x.clone().requires_grad_(True)
    calm.ops.set_noise_override(W.NoiseStream(7))
    try:
        be.attn_fwd_lse = lambda *a: (lean_calls.append(a[-4]), real(*a))[1]      # an instance attribute: Sq of each call
        y, kl = m(x)
        gy = torch.from_numpy(W.make_input(tuple(y.shape), 3, "gy")).to(y.device)
        ((y * gy).sum() + 0.5 * kl).backward()
    finally:
        del be.attn_fwd_lse
        calm.ops.set_noise_override(None)
    y, kl = y.detach(), kl.detach()
    assert rel_err(y, g["train/y"]) < MODEL_TOL
    assert rel_err_elem(y, g["train/y"]) < MODEL_TOL
    assert abs(float(kl) - float(g["train/kl"])) < MODEL_TOL * max(1.0, abs(float(g["train/kl"])))
    assert rel_err(x.grad, g["train/dx"]) < MODEL_TOL
    assert rel_err_elem(x.grad, g["train/dx"]) < MODEL_TOL
    params = dict(m.named_parameters())
    for n, ref in zip([str(s) for s in g["train/grad_names"]], g["train/grad_norms"]):
        got = float(params[n].grad.norm())
        assert abs(got - ref) <= MODEL_TOL * max(abs(ref), 1e-6) + 1e-8, (n, got, ref)
    sd = m.state_dict()
    for key in g.files:
        if key.startswith("grad/"):
            assert rel_err(params[key[5:]].grad, g[key]) < MODEL_TOL, key
        if key.startswith("post/"):
            assert rel_err(sd[key[5:]], g[key]) < MODEL_TOL, key
    return sorted(set(lean_calls))


@pytest.mark.parametrize("name", ["small224_cls", "base224_cls"])
def test_full_model_in_lse_mode_matches_reference_fixture(name):
    assert _check_against_fixture(name, name + "_b1", 1) == [80, 128, 176, 224]     # every stage runs lean


def test_nano48_in_lse_mode_matches_reference_fixture_with_mixed_dispatch():
    assert _check_against_fixture("nano48_cls", "nano48_cls", 2) == [48]           # stage 36 keeps the composed path


class _FixedNoise:
    """Latent noise that a captured step can replay: one device tensor per draw of a step, made on first use."""

    def __init__(self):
        self.bank, self.i = [], 0
        self.gen = torch.Generator(device="cuda").manual_seed(3)

    def start_step(self):
        self.i = 0

    def __call__(self, like):
        if self.i == len(self.bank):
            self.bank.append(torch.randn(like.shape, generator=self.gen, device=like.device, dtype=like.dtype))
        self.i += 1
        return self.bank[self.i - 1]


def test_graphed_step_in_lse_mode_equals_eager_step():
    """The pattern (and the bounds) of tests/test_trainer_gpu.py::test_graphed_step_equals_eager_step at Nano-48, whose
    first stage runs the lean attention: the scratch comes from the caching allocator, nothing synchronises."""
    name = "nano48_cls"
    g = load_golden(name)
    cfg = CONFIGS[name]
    rng = np.random.default_rng(5)
    bs = 8
    x = torch.from_numpy(rng.standard_normal((bs, 3, cfg.seq_length, cfg.seq_length)).astype(np.float32)).cuda()
    yy = np.zeros((bs, cfg.out_features), dtype=np.float32)
    yy[np.arange(bs), rng.integers(0, cfg.out_features, bs)] += 0.7
    yy[np.arange(bs), rng.integers(0, cfg.out_features, bs)] += 0.3
    y = torch.from_numpy(yy).cuda()
    calm.backend.set_attention_storage("lse")
    results = []
    for graphed in (False, True):
        noise = _FixedNoise()
        calm.ops.set_noise_override(noise)
        m = build_model(name, g, "cuda").train()
        opt = trainer.make_optimizer(m, capturable=True)
        eager = trainer.TrainStep(m, opt, None)
        eager(x, y)                                   # step 1 eagerly in both runs (lazy plans, the noise bank)
        noise.start_step()
        step = trainer.GraphedTrainStep(m, opt, x, y, warmup=0) if graphed else eager
        losses = []
        for _ in range(2):                            # steps 2 and 3: replayed vs eager
            noise.start_step()
            losses.append(float(step(x, y)[0]))
        torch.cuda.synchronize()
        results.append(({k: v.detach().clone() for k, v in m.state_dict().items()}, losses))
    (sd_e, l_e), (sd_g, l_g) = results
    assert all(np.isfinite(l_e)) and all(np.isfinite(l_g))
    assert abs(l_e[-1] - l_g[-1]) < 1e-4 * max(1.0, abs(l_e[-1])), (l_e, l_g)
    worst = max(float((sd_e[k] - sd_g[k]).abs().max()) for k in sd_e)
    assert worst < 5e-4, worst
