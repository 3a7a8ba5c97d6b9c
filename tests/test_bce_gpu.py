"""The binary cross-entropy kernels of csrc/loss.hip on the MI355X, through the C-ABI (HipBackend): calm_bce_fwd / _bwd
against the float64 checker (tests/bce_f64.py) on every case and variant and on strided rows, the device step metrics
(ties, NaN rows, accumulation), bit-reproducibility, non-finite propagation, and the trainer with loss="bce" and the switch
on against the stock-torch loss end (eager, autocast + GradScaler, captured into a hipGraph, the launcher's device_metrics
mode).

Measured on MI355X (figures printed by each test; helpers.rel_err against float64): see DESIGN.md section 7, "Binary
cross-entropy"."""
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import bce_f64 as K
import weights as W
from helpers import CONFIGS, load_golden, rel_err
from test_host_logic_cpu import build_model
from test_loss_cpu import _KeepGrads

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
TOL = 1e-4                                    # the project's fp32 kernel tolerance (TOL of tests/test_loss_gpu.py)


@pytest.fixture(autouse=True)
def _restore_switch():
    prev = calm.backend.get_loss_kernels()
    yield
    calm.backend.set_loss_kernels(prev)
    calm.ops.set_noise_override(None)


def _bce(z, y, flags=0, threshold=0.0, dloss=1.0, metrics=None):
    """calm_bce_fwd + _bwd on device tensors (any row stride): (loss, dlogits)."""
    be = calm.backend.get_backend()
    B, C = z.shape
    loss = torch.full((), -1.0, device="cuda")
    dlogits = torch.full((B, C), 7.0, device="cuda")
    be.bce_fwd(z, y, flags, threshold, loss, metrics, B, C)
    be.bce_bwd(z, y, flags, threshold, torch.tensor([dloss], device="cuda"), dlogits, B, C)
    return loss, dlogits


def _strided(t, pad=3):
    """The same values in rows of stride C + pad (unit column stride)."""
    buf = torch.zeros(t.shape[0], t.shape[1] + pad, device="cuda")
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _ids(p):
    (B, C, scale, kind, flags, threshold, dloss, seed), strided = p
    return f"{B}x{C}-s{scale:g}-{kind}-f{flags}-t{threshold:g}-d{dloss:g}" + ("-strided" if strided else "")


STRIDED = [(B, C, 1.0, "cutmix", f, 0.0, 3.0, 0) for B, C in ((4, 1000), (3, 10), (257, 1000)) for f in (0, K.SUM_CLASSES)]


@pytest.mark.parametrize("p", [(v, False) for v in K.VARIANTS] + [(v, True) for v in STRIDED], ids=_ids)
def test_forward_and_backward_against_the_float64_checker(p):
    (B, C, scale, kind, flags, threshold, dloss, seed), strided = p
    z, y = K.inputs(B, C, scale, kind, seed)
    ref = K.reference(z, y, flags, threshold, dloss)
    zd, yd = z.cuda(), y.cuda()
    if strided:
        zd, yd = _strided(zd), _strided(yd)
        assert zd.stride(0) == C + 3
    m = trainer.StepMetrics(torch.device("cuda"))
    loss, dlogits = _bce(zd, yd, flags, threshold, dloss, m.buf)
    got = {"loss": loss, "dlogits": dlogits, "metrics": m.buf}
    f = K.figures(got, ref)
    print(f"\nBCE {_ids(p)}: loss {f['loss'] / float(ref['loss']):.2e} dlogits {f['dlogits']:.2e} "
          f"metrics[0] {f['metrics0'] / float(ref['metrics0']):.2e} agreement {int(f['metrics'][1])} of {B}")
    assert K.check(got, ref) == []


def test_constructed_ties_go_to_the_lowest_index_nan_rows_count_as_no_agreement_and_metrics_accumulate():
    C = 1000
    z = torch.randn(5, C, generator=torch.Generator().manual_seed(1))
    y = torch.zeros(5, C)
    z[0, 17] = z[0, 901] = 9.0                             # tie inside the logits: index 17
    y[0, 17] = 1.0
    z[1, 5] = 9.0
    y[1, 5] = y[1, 640] = 0.5                              # tie inside the targets: index 5
    z[2, 3] = z[2, 2] = 9.0                                # tie -> 2, target 3: no agreement
    y[2, 3] = 1.0
    z[3, 100] = 9.0
    z[3, 999] = float("nan")                               # NaN in the logits
    y[3, 100] = 1.0
    z[4, 7] = 9.0
    y[4, 7] = 1.0
    y[4, 500] = float("nan")                               # NaN in the targets
    assert list(np.argmax(z[:3].numpy(), axis=1)) == [17, 5, 2] and list(np.argmax(y[:3].numpy(), axis=1)) == [17, 5, 3]
    m = trainer.StepMetrics(torch.device("cuda"))
    loss, _ = _bce(z.cuda(), y.cuda(), metrics=m.buf)
    assert not bool(torch.isfinite(loss))
    assert m.read()[1:] == (2, 5, 1)
    # with a threshold the count is still taken against the targets as they came: 0.6 / 0.4 -> both 1 behind the threshold,
    # whose lowest index is the WEAKER class
    m.reset()
    z2 = torch.randn(3, C, generator=torch.Generator().manual_seed(2))
    y2 = torch.zeros(3, C)
    for b, (weak, strong) in enumerate(((10, 700), (20, 800), (900, 30))):
        y2[b, weak], y2[b, strong] = 0.4, 0.6
        z2[b, strong] = 9.0
    l1, _ = _bce(z2.cuda(), y2.cuda(), K.THRESHOLD, 0.2, metrics=m.buf)
    l2, _ = _bce(z2.cuda(), y2.cuda(), K.THRESHOLD | K.SUM_CLASSES, 0.2, metrics=m.buf)
    loss_sum, agree, rows, steps = m.read()
    assert (agree, rows, steps) == (6, 6, 2)
    want = 3 * (float(l1) + float(l2))                     # [0] += B * loss under either reduction
    assert abs(loss_sum - want) <= 1e-5 * want
    assert abs(float(l2) - C * float(l1)) <= 1e-5 * float(l2)


def test_two_launches_give_the_same_bits():
    for B, C, scale, flags in ((257, 1000, 4.0, 0), (2, 21843, 2.0, K.SUM_CLASSES), (5, 1001, 1.0, K.THRESHOLD)):
        z, y = K.inputs(B, C, scale)
        a, b = _bce(z.cuda(), y.cuda(), flags, 0.2, 2.0), _bce(z.cuda(), y.cuda(), flags, 0.2, 2.0)
        for u, v in zip(a, b):
            assert torch.equal(u, v), (B, C)


def test_non_finite_logit_propagates_and_the_scaled_optimizer_step_is_skipped():
    z, y = K.inputs(8, 1000, 1.0)
    z[2, 40] = float("inf")
    z[5, 7] = float("nan")
    loss, dlogits = _bce(z.cuda(), y.cuda())
    assert not bool(torch.isfinite(loss))
    bad = ~torch.isfinite(dlogits).cpu()
    assert bool(bad[2, 40]) and bool(bad[5, 7]) and int(bad.sum()) == 2       # every class is its own problem
    # the same through a model: backward hands non-finite gradients to every parameter, the scaled step is skipped and the
    # GradScaler's scale backs off
    name = "tiny32_cls"
    cfg = CONFIGS[name]
    calm.backend.set_loss_kernels(True)
    m = build_model(name, load_golden(name), "cuda").train()
    opt = trainer.FusedClipAdamW(m)
    try:
        x = torch.from_numpy(W.make_input((4, 3, cfg.seq_length, cfg.seq_length), 2)).cuda()
        y = K.inputs(4, cfg.out_features, 1.0)[1].cuda()
        scale = torch.tensor(1024.0, device="cuda")
        bump = torch.zeros(4, cfg.out_features, device="cuda")
        for expect_inf in (0.0, 1.0):
            before = {k: v.clone() for k, v in m.state_dict().items() if k.endswith("weight_orig")}
            y_hat, _ = m(x)
            loss = trainer.soft_target_bce(y_hat.reshape(4, -1) + bump, y)
            assert loss.grad_fn is not None and "BinaryCrossEntropyFn" in type(loss.grad_fn).__name__
            (loss * scale).backward()
            stats = opt.step(grad_scale=scale)
            assert float(stats[1]) == expect_inf
            assert bool(torch.isfinite(loss)) == (expect_inf == 0.0)
            changed = sum(not torch.equal(v, before[k]) for k, v in m.state_dict().items() if k in before)
            assert (changed == 0) == (expect_inf == 1.0)
            bump[1, 3] = float("inf")
        assert opt.step_count == 1
    finally:
        opt.close()
    # and through TrainStep with a GradScaler: the scale backs off
    m = build_model(name, load_golden(name), "cuda").train()
    opt = trainer.FusedClipAdamW(m)
    try:
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
        step = trainer.TrainStep(m, opt, None, scaler=scaler, loss="bce")
        xb = x.clone()
        xb[1, 0, 0, 0] = float("inf")
        step(x, y)
        assert float(scaler.get_scale()) == 1024.0 and opt.step_count == 1
        loss, _ = step(xb, y)
        assert not bool(torch.isfinite(loss))
        assert float(scaler.get_scale()) == 512.0 and opt.step_count == 1
    finally:
        opt.close()


def first_step(name, on, scaler=None, autocast_dtype=None, bs=4, loss="bce"):
    """(loss, gradients after clipping) of the first TrainStep(loss=) of a fixture model with the loss kernels on / off (as
    first_step of tests/test_loss_cpu.py)."""
    g = load_golden(name)
    cfg = CONFIGS[name]
    calm.backend.set_loss_kernels(on)
    m = build_model(name, g, "cuda").train()
    x = torch.from_numpy(W.make_input((bs, 3, cfg.seq_length, cfg.seq_length), 2)).cuda()
    opt = _KeepGrads([p for p in m.parameters() if p.requires_grad], lr=0.0)
    calm.ops.set_noise_override(W.NoiseStream(7))
    calls = []
    fn = calm.ops.BinaryCrossEntropyFn
    real = fn.apply
    fn.apply = lambda *a: (calls.append(1), real(*a))[1]
    try:
        y = K.inputs(bs, cfg.out_features, 1.0)[1].cuda()
        out, _ = trainer.TrainStep(m, opt, None, scaler=scaler, autocast_dtype=autocast_dtype, loss=loss)(x, y)
    finally:
        del fn.apply
        calm.ops.set_noise_override(None)
    assert len(calls) == int(on)                           # the kernels ran exactly when they were switched on
    return out, dict(zip([n for n, p in m.named_parameters() if p.requires_grad], opt.kept))


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "autocast+GradScaler"])
@pytest.mark.parametrize("loss", ["bce", {"name": "bce", "target_threshold": 0.2, "sum_classes": True}], ids=["mean", "threshold-sum"])
@pytest.mark.parametrize("name", ["nano48_cls", "tiny32_cls"])
def test_first_trainer_step_with_the_kernels_on_equals_the_torch_loss_step(name, loss, amp):
    res = []
    for on in (False, True):
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0) if amp else None
        res.append(first_step(name, on, scaler=scaler, autocast_dtype=torch.bfloat16 if amp else None, loss=loss))
    (loss_off, grads_off), (loss_on, grads_on) = res
    worst = max(rel_err(grads_on[n], grads_off[n]) for n in grads_off)
    print(f"\n{name} amp={amp} {loss}: loss {rel_err(loss_on, loss_off):.2e} worst parameter gradient {worst:.2e}")
    assert rel_err(loss_on, loss_off) <= TOL
    for n in grads_off:
        assert rel_err(grads_on[n], grads_off[n]) <= TOL, n


def test_graphed_step_with_a_metrics_buffer_replays_the_eager_trajectory_exactly():
    name = "nano48_cls"
    g = load_golden(name)
    cfg = CONFIGS[name]
    bs = 8
    x = torch.from_numpy(W.make_input((bs, 3, cfg.seq_length, cfg.seq_length), 2)).cuda()
    y = K.inputs(bs, cfg.out_features, 1.0)[1].cuda()
    calm.backend.set_loss_kernels(True)
    be = calm.backend.get_backend()
    prev = be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, 1)
    try:
        outs = []
        for graphed in (False, True):
            torch.manual_seed(11)                          # nano48_cls draws latent noise: both runs from one generator state
            torch.cuda.manual_seed(11)
            m = build_model(name, g, "cuda").train()
            opt = trainer.FusedClipAdamW(m)
            metrics = trainer.StepMetrics(torch.device("cuda"))
            try:
                if graphed:
                    step = trainer.GraphedTrainStep(m, opt, x, y, restore_after_warmup=True, metrics=metrics, loss="bce")
                    assert step.inner.loss_settings["name"] == "bce"
                else:
                    step = trainer.TrainStep(m, opt, None, metrics=metrics, loss="bce")
                losses = [step(x, y)[0].clone() for _ in range(4)]
                torch.cuda.synchronize()
                outs.append(({k: v.detach().clone() for k, v in m.state_dict().items()}, torch.stack(losses), metrics.read()))
            finally:
                opt.close()
    finally:
        be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, prev)
    (sd_e, l_e, m_e), (sd_g, l_g, m_g) = outs
    assert torch.equal(l_e, l_g)
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k
    assert m_g[2:] == (4 * bs, 4) and m_e == m_g
    assert abs(m_g[0] - float(l_g.sum()) * bs) <= 1e-5 * m_g[0]


class _Reads:
    """Counts the device-to-host reads a loop makes through Tensor.item and StepMetrics.read."""

    def __enter__(self):
        self.items, self.reads = 0, 0
        self._item, self._read = torch.Tensor.item, trainer.StepMetrics.read
        outer = self

        def item(t):
            outer.items += 1
            return outer._item(t)

        def read(m):
            outer.reads += 1
            return outer._read(m)
        torch.Tensor.item, trainer.StepMetrics.read = item, read
        return self

    def __exit__(self, *exc):
        torch.Tensor.item, trainer.StepMetrics.read = self._item, self._read


def test_launcher_with_device_metrics_makes_no_per_step_read_and_prints_the_epoch_mean(capsys):
    name = "nano48_cls"
    g = load_golden(name)
    cfg = CONFIGS[name]
    S = cfg.seq_length
    gen = torch.Generator().manual_seed(3)
    data = torch.utils.data.TensorDataset(torch.randn(48, 3, S, S, generator=gen),
                                          torch.randint(0, cfg.out_features, (48,), generator=gen))
    calm.backend.set_loss_kernels(True)
    losses, settings = [], []
    real_call = trainer.TrainStep.__call__

    def spy(self, x, y):
        out = real_call(self, x, y)
        losses.append(out[0].clone())                      # kept on the device: read after the run
        settings.append(self.loss_settings)
        return out
    trainer.TrainStep.__call__ = spy
    try:
        with _Reads() as r:
            trainer.train(build_model(name, g, "cpu"), "fused", scheduler=False, use_gpu=True, dataset=data, epochs=1,
                          batch_size=8, num_classes=cfg.out_features, log_every=100, max_steps=6, device_metrics=True,
                          selfcheck=None, loss={"name": "bce", "sum_classes": True})
    finally:
        trainer.TrainStep.__call__ = real_call
    out = capsys.readouterr().out
    assert len(losses) == 6 and all(s == {"name": "bce", "target_threshold": None, "sum_classes": True} for s in settings)
    assert "loss: binary cross-entropy with logits, target_threshold None, sum_classes True" in out
    # log_every=100: the one `Batch: 1` line reads its accuracy and its loss; nothing reads per step (six steps ran)
    print(f"\nreads {r.reads} items {r.items}")
    assert r.reads == 1 and r.items <= 2, (r.reads, r.items)
    line = [ln for ln in out.splitlines() if "Mean loss" in ln]
    assert len(line) == 1, out
    mean = float(re.search(r"Mean loss: ([-+0-9.eE]+|nan|inf)", line[0]).group(1))
    want = float(torch.stack(losses).double().mean())
    assert abs(mean - want) <= 1e-5 * abs(want), (mean, want)
    assert re.search(r"Dominant-class accuracy: \d+\.\d+%", line[0])
