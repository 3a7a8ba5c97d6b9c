"""The loss end of the step (soft-target cross-entropy, token-layout Huber, device step metrics) on a host without a GPU:
the five C-ABI additions are declared, exported and bound, the scratch query answers from host code, the switch behaves,
and the host logic — ops.SoftTargetCrossEntropyFn / HuberTokensFn, trainer.StepMetrics, where TrainStep / RegTrainStep /
evaluate take the kernels and where they stay with torch — is checked over the torch emulation of the entry points
(tests/emulated_loss.py) against float64 autograd."""
import os
import re
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import calm_vit_dte_amd as calm
import weights as W
from emulated_loss import EmulatedLossBackend
from helpers import CONFIGS, load_golden, rel_err
from test_host_logic_cpu import build_model

trainer = import_module("calm_vit_dte_amd.trainer")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "calm_vit.h")
NAMES = ("calm_soft_ce_fwd", "calm_soft_ce_bwd", "calm_huber_tokens_fwd", "calm_huber_tokens_bwd", "calm_top1_count")
# (B, C, logit scale) of the cross-entropy checks and (B, S) of the Huber checks — shared with tests/test_loss_gpu.py
CE_CASES = [(256, 1000, 1.0), (484, 1000, 4.0), (1, 1000, 1.0), (3, 10, 1.0), (257, 1001, 8.0), (256, 1000, 30.0),
            (37, 21843, 2.0)]
HUBER_CASES = [(2, 48), (3, 32), (2, 224), (5, 80)]
# formulas, not hardware: the fp32 formula of the kernels stays at or below 3.8e-6 of float64 on every input above
TOL = 1e-5


@pytest.fixture(autouse=True)
def _restore_switch():
    prev = calm.backend.get_loss_kernels()
    yield
    calm.backend.set_loss_kernels(prev)
    calm.ops.set_noise_override(None)


def ce_inputs(B, C, scale, kind="cutmix", seed=0, offset=0.0):
    """Logits scale * randn + offset and targets: 'cutmix' = two classes per row with weights lam, 1 - lam (the
    CutMix / MixUp labels of cls:58-61), 'unnormalised' = uniform(0, 1) in every class (row sums ~ C / 2)."""
    g = torch.Generator().manual_seed(seed + 7919 * B + C)
    z = torch.randn(B, C, generator=g) * scale + offset
    if kind == "unnormalised":
        return z, torch.rand(B, C, generator=g)
    y = torch.zeros(B, C)
    lam = torch.rand(B, generator=g) * 0.8 + 0.1
    rows = torch.arange(B)
    y[rows, torch.randint(0, C, (B,), generator=g)] += lam
    y[rows, torch.randint(0, C, (B,), generator=g)] += 1.0 - lam
    return z, y


def ce_reference(z, y, upstream=1.0):
    """float64 autograd of F.cross_entropy with probability targets: (loss, dlogits) for d(upstream * loss)."""
    z64 = z.double().requires_grad_(True)
    loss = F.cross_entropy(z64, y.double())
    (loss * upstream).backward()
    return loss.detach(), z64.grad


def huber_inputs(B, S, spread=1.0, shift=0.0, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * B + S)
    x = torch.randn(B, 3, S, S, generator=g)
    d = torch.randn(B, S, 3 * S, generator=g) * spread
    if shift:
        d = d + shift * torch.sign(d)                              # every |difference| > shift
    if spread < 1:
        d = d.clamp(-0.9, 0.9)                                     # every |difference| < 1
    tokens = x.permute(0, 2, 3, 1).reshape(B, S, 3 * S) + d
    return tokens.contiguous(), x


def huber_reference(tokens, x, upstream=1.0, delta=1.0):
    B, S = tokens.shape[0], tokens.shape[1]
    t64 = tokens.double().requires_grad_(True)
    loss = F.huber_loss(t64.reshape(-1, S, S, 3).permute(0, 3, 1, 2), x.double(), delta=delta)
    (loss * upstream).backward()
    return loss.detach(), t64.grad


def test_entry_points_are_declared_exported_bound_and_the_scratch_query_answers():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(calm_\w+)\s*\(", text, flags=re.M))
    binding = calm._lib
    lib = binding.load()                                       # resolves every bound symbol, checks the ABI version
    for n in NAMES:
        assert n in declared, n
        assert n in binding.SIGNATURES, n
        assert hasattr(lib, n), n
    assert int(re.search(r"#define\s+CALM_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 7   # additions only
    assert binding.ABI_VERSION == 7
    assert (binding.RED_SOFT_CE, binding.RED_HUBER) == (5, 6)
    for B, C, _ in CE_CASES:
        need = int(lib.calm_reduce_scratch_floats(binding.RED_SOFT_CE, B, C))
        assert 0 < need <= (1 << 22), (B, C, need)
    for B, S in HUBER_CASES + [(256, 224)]:
        need = int(lib.calm_reduce_scratch_floats(binding.RED_HUBER, B * S, 3 * S))
        assert 0 < need <= (1 << 22), (B, S, need)
    assert int(lib.calm_reduce_scratch_floats(99, 10, 10)) == 0


def test_switch_default_round_trip_environment_and_off_is_stock_torch():
    be = calm.backend
    if not os.environ.get("CALM_LOSS_KERNELS"):
        assert be.get_loss_kernels() is False
    be.set_loss_kernels(True)
    assert be.get_loss_kernels() is True
    be.set_loss_kernels(False)
    assert be.get_loss_kernels() is False
    code = "import calm_vit_dte_amd as c; print('loss_kernels=' + str(c.backend.get_loss_kernels()))"
    for value, expect in (("1", True), ("0", False), (None, False)):
        env = {k: v for k, v in os.environ.items() if k != "CALM_LOSS_KERNELS"}
        if value is not None:
            env["CALM_LOSS_KERNELS"] = value
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert f"loss_kernels={expect}" in r.stdout
    z, y = ce_inputs(6, 10, 1.0)
    z.requires_grad_(True)
    z2 = z.detach().clone().requires_grad_(True)
    a, b = trainer.soft_target_cross_entropy(z, y), F.cross_entropy(z2, y)
    a.backward()
    b.backward()
    assert torch.equal(a, b) and torch.equal(z.grad, z2.grad)
    # switched on, what the kernels do not serve still is F.cross_entropy: CPU tensors on the product backend, 1-D logits
    be.set_loss_kernels(True)
    assert torch.equal(trainer.soft_target_cross_entropy(z.detach(), y), b.detach())
    with be.use_backend(EmulatedLossBackend()):
        assert torch.equal(trainer.soft_target_cross_entropy(z.detach()[0], y[0]), F.cross_entropy(z.detach()[0], y[0]))


@pytest.mark.parametrize("kind,upstream", [("cutmix", 1.0), ("unnormalised", 1.0), ("cutmix", 1024.0)])
@pytest.mark.parametrize("B,C,scale", CE_CASES)
def test_cross_entropy_function_against_float64_autograd(B, C, scale, kind, upstream):
    z, y = ce_inputs(B, C, scale, kind)
    loss_ref, dz_ref = ce_reference(z, y, upstream)
    zl = z.clone().requires_grad_(True)
    with calm.backend.use_backend(EmulatedLossBackend()):
        loss = calm.ops.SoftTargetCrossEntropyFn.apply(zl, y)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        (loss * upstream).backward()
    print(f"\nCE {B}x{C} scale {scale} {kind} x{upstream}: loss {rel_err(loss.detach(), loss_ref):.2e} "
          f"dlogits {rel_err(zl.grad, dz_ref):.2e}")
    assert rel_err(loss.detach(), loss_ref) <= TOL
    assert rel_err(zl.grad, dz_ref) <= TOL


def test_cross_entropy_function_saves_logits_targets_and_row_stats_only():
    z, y = ce_inputs(5, 10, 1.0)
    sizes = []
    with calm.backend.use_backend(EmulatedLossBackend()), \
            torch.autograd.graph.saved_tensors_hooks(lambda t: (sizes.append(tuple(t.shape)), t)[1], lambda t: t):
        calm.ops.SoftTargetCrossEntropyFn.apply(z.requires_grad_(True), y)
    assert sorted(sizes) == [(5, 2), (5, 10), (5, 10)]


@pytest.mark.parametrize("upstream", [1.0, 512.0])
@pytest.mark.parametrize("B,S,spread,shift", [(b, s, 1.0, 0.0) for b, s in HUBER_CASES] + [(2, 48, 0.2, 0.0), (2, 48, 1.0, 1.0)])
def test_huber_function_against_float64_autograd(B, S, spread, shift, upstream):
    tokens, x = huber_inputs(B, S, spread, shift)
    loss_ref, dt_ref = huber_reference(tokens, x, upstream)
    tl = tokens.clone().requires_grad_(True)
    with calm.backend.use_backend(EmulatedLossBackend()):
        loss = calm.ops.HuberTokensFn.apply(tl, x)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        (loss * upstream).backward()
    assert rel_err(loss.detach(), loss_ref) <= TOL
    assert rel_err(tl.grad, dt_ref) <= TOL


def test_step_metrics_accumulate_break_ties_low_ignore_nan_rows_and_reset():
    be = EmulatedLossBackend()
    m = trainer.StepMetrics(torch.device("cpu"))
    assert m.read() == (0.0, 0, 0, 0)
    want_loss = want_agree = 0.0
    with calm.backend.use_backend(be):
        for seed in range(3):
            z, y = ce_inputs(7, 10, 1.0, seed=seed)
            loss = calm.ops.SoftTargetCrossEntropyFn.apply(z, y, m.buf)
            want_loss += float(loss) * 7
            want_agree += int((z.argmax(1) == y.argmax(1)).sum())
        loss_sum, agree, rows, steps = m.read()
        assert (agree, rows, steps) == (want_agree, 21, 3)
        assert isinstance(agree, int) and isinstance(rows, int) and isinstance(steps, int)
        assert abs(loss_sum - want_loss) <= 1e-5 * want_loss
        m.reset()
        assert m.read() == (0.0, 0, 0, 0)
        # ties go to the lowest index, on both sides
        z = torch.tensor([[0.0, 2.0, 2.0, 1.0], [3.0, 1.0, 3.0, 3.0], [1.0, 5.0, 0.0, 5.0]])
        y = torch.tensor([[0.0, 0.5, 0.5, 0.0], [0.0, 0.0, 0.5, 0.5], [0.0, 0.5, 0.0, 0.5]])
        assert list(np.argmax(z.numpy(), axis=1)) == [1, 0, 1] and list(np.argmax(y.numpy(), axis=1)) == [1, 2, 1]
        calm.ops.SoftTargetCrossEntropyFn.apply(z, y, m.buf)
        assert m.read()[1:] == (2, 3, 1)
        m.reset()
        # a row that holds a NaN counts as no agreement, whatever its argmax would say
        z = torch.tensor([[0.0, 2.0, float("nan"), 1.0], [0.0, 3.0, 1.0, 2.0]])
        y = torch.tensor([[0.0, 1.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]])
        loss = calm.ops.SoftTargetCrossEntropyFn.apply(z, y, m.buf)
        assert not torch.isfinite(loss)
        assert m.read()[1:] == (1, 2, 1)
        m.reset()
        be.top1_count(torch.tensor([[1.0, 4.0, 4.0], [2.0, 1.0, 0.0]]), torch.tensor([1, 2]), m.buf, 2, 3)
        assert m.read() == (0.0, 1, 2, 0)


class _KeepGrads(torch.optim.SGD):
    """lr = 0 and a zero_grad that first keeps what the step left in `.grad`: lets a test read the gradients of a whole
    TrainStep (which ends in zero_grad, cls:96)."""

    def zero_grad(self, set_to_none=True):
        self.kept = [None if p.grad is None else p.grad.detach().clone() for g in self.param_groups for p in g["params"]]
        super().zero_grad(set_to_none)


def first_step(name, on, device="cpu", scaler=None, autocast_dtype=None, bs=2):
    """(loss, gradients after clipping) of the first trainer step of a fixture model with the loss kernels on / off."""
    g = load_golden(name)
    cfg = CONFIGS[name]
    calm.backend.set_loss_kernels(on)
    m = build_model(name, g, device).train()
    x = torch.from_numpy(W.make_input((bs, 3, cfg.seq_length, cfg.seq_length), 2)).to(device)
    opt = _KeepGrads([p for p in m.parameters() if p.requires_grad], lr=0.0)
    calm.ops.set_noise_override(W.NoiseStream(7))
    try:
        if cfg.generate:
            loss, _ = trainer.RegTrainStep(m, opt, None, scaler=scaler, autocast_dtype=autocast_dtype)(x)
        else:
            _, y = ce_inputs(bs, cfg.out_features, 1.0)
            loss, _ = trainer.TrainStep(m, opt, None, scaler=scaler, autocast_dtype=autocast_dtype)(x, y.to(device))
    finally:
        calm.ops.set_noise_override(None)
    return loss, dict(zip([n for n, p in m.named_parameters() if p.requires_grad], opt.kept))


@pytest.mark.parametrize("name", ["nano48_cls", "nano48_gen"])
def test_first_trainer_step_with_the_kernels_on_equals_the_torch_loss_step(name):
    calls = []
    be = EmulatedLossBackend()
    for fn in ("soft_ce_fwd", "soft_ce_bwd", "huber_tokens_fwd", "huber_tokens_bwd"):
        setattr(be, fn, (lambda real, fn=fn: lambda *a: (calls.append(fn), real(*a))[1])(getattr(be, fn)))
    with calm.backend.use_backend(be):
        loss_off, grads_off = first_step(name, False)
        assert not calls
        loss_on, grads_on = first_step(name, True)
    assert calls == (["huber_tokens_fwd", "huber_tokens_bwd"] if name.endswith("gen") else ["soft_ce_fwd", "soft_ce_bwd"])
    assert rel_err(loss_on, loss_off) <= TOL
    for n in grads_off:
        assert grads_on[n] is not None and grads_off[n] is not None, n
        assert rel_err(grads_on[n], grads_off[n]) <= TOL, n


def test_evaluate_counts_on_the_device_once_and_returns_the_same_accuracy():
    m = build_model("nano48_cls", load_golden("nano48_cls")).train()
    xs = torch.from_numpy(W.make_input((4, 3, 48, 48), 5))
    be = EmulatedLossBackend()
    with calm.backend.use_backend(be):
        with torch.no_grad():
            labels = m.eval()(xs)[0].reshape(4, -1).argmax(dim=1)
        m.train()
        labels[3] = (labels[3] + 1) % 10
        batches = [(xs[:2], labels[:2]), (xs[2:], labels[2:])]
        off = trainer.evaluate(m, batches)
        calm.backend.set_loss_kernels(True)
        reads = []
        real = trainer.StepMetrics.read
        trainer.StepMetrics.read = lambda self: (reads.append(1), real(self))[1]
        try:
            on = trainer.evaluate(m, batches)
        finally:
            trainer.StepMetrics.read = real
    assert off == on == 0.75 and len(reads) == 1 and m.training


def test_device_metrics_argument_errors_come_before_any_process_group():
    data = torch.utils.data.TensorDataset(torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,)))
    sgd = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    for on, use_gpu in ((True, False), (False, True), (False, False)):
        calm.backend.set_loss_kernels(on)
        with pytest.raises(ValueError, match="device_metrics"):
            trainer.train(torch.nn.Linear(4, 4), sgd, use_gpu=use_gpu, dataset=data, epochs=1, batch_size=2,
                          num_classes=10, device_metrics=True)
    assert not torch.distributed.is_initialized()
