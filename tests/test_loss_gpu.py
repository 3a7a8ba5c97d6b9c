"""The loss kernels of csrc/loss.hip on the MI355X, through the C-ABI (HipBackend): soft-target cross-entropy and the
token-layout Huber loss against float64, the device step metrics against torch's argmax counts, bit-reproducibility,
non-finite propagation, and the trainer with the switch on against the stock-torch loss end (eager, autocast +
GradScaler, captured into a hipGraph, the eval loop, the launcher's device_metrics mode).

Measured on MI355X (figures printed by each test; normalised inf-norm against float64, helpers.rel_err): see DESIGN.md
section 7, "Loss kernels"."""
import re
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import calm_vit_dte_amd as calm
import weights as W
from helpers import CONFIGS, load_golden, rel_err
from test_host_logic_cpu import build_model
from test_loss_cpu import (CE_CASES, HUBER_CASES, ce_inputs, ce_reference, first_step, huber_inputs, huber_reference)

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
TOL = 1e-4                                    # the project's fp32 kernel tolerance (normalised inf-norm, helpers.rel_err)


@pytest.fixture(autouse=True)
def _restore_switch():
    prev = calm.backend.get_loss_kernels()
    yield
    calm.backend.set_loss_kernels(prev)
    calm.ops.set_noise_override(None)


def _ce(z, y, dloss=1.0, metrics=None):
    """calm_soft_ce_fwd + _bwd on device tensors (any row stride): (loss, dlogits, row_stats)."""
    be = calm.backend.get_backend()
    B, C = z.shape
    row_stats = torch.empty(B, 2, device="cuda")
    loss = torch.full((), -1.0, device="cuda")
    dlogits = torch.empty(B, C, device="cuda")
    be.soft_ce_fwd(z, y, row_stats, loss, metrics, B, C)
    be.soft_ce_bwd(z, y, row_stats, torch.tensor([dloss], device="cuda"), dlogits, B, C)
    return loss, dlogits, row_stats


def _huber(tokens, x, dloss=1.0, delta=1.0):
    be = calm.backend.get_backend()
    B, S = tokens.shape[0], tokens.shape[1]
    loss = torch.full((), -1.0, device="cuda")
    dtokens = torch.empty_like(tokens)
    be.huber_tokens_fwd(tokens, x, delta, loss, B, S)
    be.huber_tokens_bwd(tokens, x, delta, torch.tensor([dloss], device="cuda"), dtokens, B, S)
    return loss, dtokens


def _strided(t, pad=3):
    """The same values in rows of stride C + pad (unit column stride)."""
    buf = torch.zeros(t.shape[0], t.shape[1] + pad, device="cuda")
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


@pytest.mark.parametrize("B,C,scale,strided", [c + (False,) for c in CE_CASES] +
                         [(256, 1000, 1.0, True), (3, 10, 1.0, True), (257, 1001, 8.0, True)])
def test_cross_entropy_forward_and_backward_against_float64(B, C, scale, strided):
    z, y = ce_inputs(B, C, scale)
    loss_ref, dz_ref = ce_reference(z, y, 3.0)
    zd, yd = z.cuda(), y.cuda()
    if strided:
        zd, yd = _strided(zd), _strided(yd)
    loss, dlogits, row_stats = _ce(zd, yd, 3.0)
    m64 = z.double().max(dim=1).values
    ls64 = torch.log(torch.exp(z.double() - m64[:, None]).sum(dim=1))
    e = (rel_err(loss, loss_ref), rel_err(dlogits, dz_ref), rel_err(row_stats[:, 0], m64), rel_err(row_stats[:, 1], ls64))
    print(f"\nCE {B}x{C} scale {scale} strided={strided}: loss {e[0]:.2e} dlogits {e[1]:.2e} max {e[2]:.2e} logsum {e[3]:.2e}")
    assert e[0] <= TOL and e[1] <= TOL
    assert e[2] <= 1e-5 and e[3] <= 1e-5
    if not strided:                                        # un-normalised targets: the sum_c y factor of the backward
        z, y = ce_inputs(B, C, scale, "unnormalised")
        loss_ref, dz_ref = ce_reference(z, y)
        loss, dlogits, _ = _ce(z.cuda(), y.cuda())
        assert rel_err(loss, loss_ref) <= TOL and rel_err(dlogits, dz_ref) <= TOL


@pytest.mark.parametrize("B,C,scale", CE_CASES)
def test_dominant_class_and_top1_counts_equal_torch_argmax_counts(B, C, scale):
    z, y = ce_inputs(B, C, scale)
    y = y + 1e-3 * torch.rand(B, C, generator=torch.Generator().manual_seed(B + C))
    for ref in (z, y):                                     # tie-free inputs: the counts below have one right answer
        top2 = ref.double().topk(min(2, C), dim=1).values
        assert C == 1 or bool((top2[:, 0] - top2[:, 1] > 0).all())
    labels = torch.where(torch.arange(B) % 2 == 0, z.argmax(1), torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(3)))
    m = trainer.StepMetrics(torch.device("cuda"))
    be = calm.backend.get_backend()
    _ce(z.cuda(), y.cuda(), metrics=m.buf)
    be.top1_count(z.cuda(), labels.cuda(), m.buf, B, C)
    _, agree, rows, steps = m.read()
    want = int((z.argmax(1) == y.argmax(1)).sum()) + int((z.argmax(1) == labels).sum())
    assert (agree, rows, steps) == (want, 2 * B, 1)


def test_constructed_ties_go_to_the_lowest_index_and_nan_rows_count_as_no_agreement():
    C = 1000
    z = torch.randn(4, C, generator=torch.Generator().manual_seed(1))
    y = torch.zeros(4, C)
    z[0, 17] = z[0, 901] = 9.0                             # tie inside the logits: index 17
    y[0, 17] = 1.0
    z[1, 5] = 9.0
    y[1, 5] = y[1, 640] = 0.5                              # tie inside the targets: index 5
    z[2, 3] = z[2, 2] = 9.0                                # tie -> 2, target 3: no agreement
    y[2, 3] = 1.0
    z[3, 100] = 9.0
    z[3, 999] = float("nan")                               # NaN row
    y[3, 100] = 1.0
    assert list(np.argmax(z[:3].numpy(), axis=1)) == [17, 5, 2] and list(np.argmax(y[:3].numpy(), axis=1)) == [17, 5, 3]
    m = trainer.StepMetrics(torch.device("cuda"))
    _ce(z.cuda(), y.cuda(), metrics=m.buf)
    calm.backend.get_backend().top1_count(z.cuda(), torch.tensor([17, 901, 2, 100]).cuda(), m.buf, 4, C)
    _, agree, rows, steps = m.read()
    assert (agree, rows, steps) == (2 + 2, 8, 1)


def test_offset_logits_keep_the_accuracy_of_torchs_own_fp32_gradient():
    """z = 1e4 + randn: exp(z - lse) in fp32 loses the gradient to the rounding of z - lse (ulp(1e4) ~ 1e-3); subtracting
    the row maximum first does not.  Bound: the kernel's error against float64 is at most 4x the error of torch's fp32
    F.cross_entropy gradient on the same device and input (the factor covers the fast exponential), plus a floor of 1e-6."""
    z, y = ce_inputs(64, 1000, 1.0, offset=1e4)
    _, dz_ref = ce_reference(z, y)
    zt = z.cuda().requires_grad_(True)
    F.cross_entropy(zt, y.cuda()).backward()
    err_torch = rel_err(zt.grad, dz_ref)
    _, dlogits, _ = _ce(z.cuda(), y.cuda())
    err = rel_err(dlogits, dz_ref)
    lse = torch.logsumexp(z.cuda(), dim=1, keepdim=True)
    fused = (torch.exp(z.cuda() - lse) * y.cuda().sum(1, keepdim=True) - y.cuda()) / 64          # the cancelling formula
    print(f"\noffset 1e4: kernel {err:.2e} torch fp32 {err_torch:.2e} exp(z - lse) {rel_err(fused, dz_ref):.2e}")
    assert err <= 4 * err_torch + 1e-6
    assert rel_err(fused, dz_ref) > 4 * err_torch + 1e-6                # what the bound is there to catch


@pytest.mark.parametrize("B,S,spread,shift", [(b, s, 1.0, 0.0) for b, s in HUBER_CASES] + [(2, 48, 0.2, 0.0), (2, 48, 1.0, 1.0)])
def test_huber_forward_and_backward_against_float64(B, S, spread, shift):
    tokens, x = huber_inputs(B, S, spread, shift)
    d = tokens.reshape(B, S, S, 3).permute(0, 3, 1, 2) - x
    linear = float((d.abs() > 1).float().mean())
    if shift:
        assert linear == 1.0
    elif spread < 1:
        assert linear == 0.0
    loss_ref, dt_ref = huber_reference(tokens, x, 5.0)
    loss, dtokens = _huber(tokens.cuda(), x.cuda(), 5.0)
    e = (rel_err(loss, loss_ref), rel_err(dtokens, dt_ref))
    print(f"\nHuber B={B} S={S} linear share {linear:.2f}: loss {e[0]:.2e} dtokens {e[1]:.2e}")
    assert e[0] <= TOL and e[1] <= TOL


def test_huber_at_a_side_the_vector_path_does_not_serve_keeps_the_right_numbers():
    """S = 36 is a multiple of 4 and runs the kernel; S = 6 is not, and RegTrainStep's loss then is torch's."""
    tokens, x = huber_inputs(2, 36)
    loss_ref, dt_ref = huber_reference(tokens, x)
    loss, dtokens = _huber(tokens.cuda(), x.cuda())
    assert rel_err(loss, loss_ref) <= TOL and rel_err(dtokens, dt_ref) <= TOL
    calm.backend.set_loss_kernels(True)
    tokens, x = huber_inputs(2, 6)
    loss_ref, dt_ref = huber_reference(tokens, x)
    t = tokens.cuda().requires_grad_(True)
    loss = trainer.RegTrainStep._huber(t, t.reshape(-1, 6, 6, 3).permute(0, 3, 1, 2), x.cuda())
    loss.backward()
    assert rel_err(loss.detach(), loss_ref) <= TOL and rel_err(t.grad, dt_ref) <= TOL


def test_two_launches_give_the_same_bits():
    z, y = ce_inputs(484, 1000, 4.0)
    a, b = _ce(z.cuda(), y.cuda(), 2.0), _ce(z.cuda(), y.cuda(), 2.0)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    z, y = ce_inputs(37, 21843, 2.0)
    a, b = _ce(z.cuda(), y.cuda()), _ce(z.cuda(), y.cuda())
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    tokens, x = huber_inputs(2, 224)
    a, b = _huber(tokens.cuda(), x.cuda(), 2.0), _huber(tokens.cuda(), x.cuda(), 2.0)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_non_finite_logit_propagates_and_the_scaled_optimizer_step_is_skipped():
    z, y = ce_inputs(8, 1000, 1.0)
    z[2, 40] = float("inf")
    loss, dlogits, _ = _ce(z.cuda(), y.cuda())
    assert not bool(torch.isfinite(loss))
    assert not bool(torch.isfinite(dlogits[2]).any())
    assert bool(torch.isfinite(dlogits[[0, 1, 3, 4, 5, 6, 7]]).all())
    # the same through a model: backward hands non-finite gradients to every parameter, the scaled step is skipped
    name = "tiny32_cls"
    cfg = CONFIGS[name]
    calm.backend.set_loss_kernels(True)
    m = build_model(name, load_golden(name), "cuda").train()
    opt = trainer.FusedClipAdamW(m)
    try:
        x = torch.from_numpy(W.make_input((4, 3, cfg.seq_length, cfg.seq_length), 2)).cuda()
        y = ce_inputs(4, cfg.out_features, 1.0)[1].cuda()
        scale = torch.tensor(1024.0, device="cuda")
        bump = torch.zeros(4, cfg.out_features, device="cuda")
        for expect_inf in (0.0, 1.0):
            before = {k: v.clone() for k, v in m.state_dict().items() if k.endswith("weight_orig")}
            y_hat, _ = m(x)
            loss = trainer.soft_target_cross_entropy(y_hat.reshape(4, -1) + bump, y)
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


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "autocast+GradScaler"])
@pytest.mark.parametrize("name", ["nano48_cls", "tiny32_cls", "nano48_gen"])
def test_first_trainer_step_with_the_kernels_on_equals_the_torch_loss_step(name, amp):
    res = []
    for on in (False, True):
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0) if amp else None
        res.append(first_step(name, on, "cuda", scaler=scaler, autocast_dtype=torch.bfloat16 if amp else None, bs=4))
    (loss_off, grads_off), (loss_on, grads_on) = res
    worst = max(rel_err(grads_on[n], grads_off[n]) for n in grads_off)
    print(f"\n{name} amp={amp}: loss {rel_err(loss_on, loss_off):.2e} worst parameter gradient {worst:.2e}")
    assert rel_err(loss_on, loss_off) <= TOL
    for n in grads_off:
        assert rel_err(grads_on[n], grads_off[n]) <= TOL, n


def test_graphed_step_with_a_metrics_buffer_replays_the_eager_trajectory_exactly():
    name = "tiny32_cls"
    g = load_golden(name)
    cfg = CONFIGS[name]
    bs = 8
    x = torch.from_numpy(W.make_input((bs, 3, cfg.seq_length, cfg.seq_length), 2)).cuda()
    y = ce_inputs(bs, cfg.out_features, 1.0)[1].cuda()
    calm.backend.set_loss_kernels(True)
    be = calm.backend.get_backend()
    prev = be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, 1)
    try:
        outs = []
        for graphed in (False, True):
            m = build_model(name, g, "cuda").train()
            opt = trainer.FusedClipAdamW(m)
            metrics = trainer.StepMetrics(torch.device("cuda"))
            try:
                if graphed:
                    step = trainer.GraphedTrainStep(m, opt, x, y, restore_after_warmup=True, metrics=metrics)
                else:
                    step = trainer.TrainStep(m, opt, None, metrics=metrics)
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


def test_evaluate_reads_once_for_the_whole_loop_and_returns_the_same_accuracy():
    m = build_model("nano48_cls", load_golden("nano48_cls"), "cuda")
    xs = torch.from_numpy(W.make_input((6, 3, 48, 48), 5)).cuda()
    with torch.no_grad():
        labels = m.eval()(xs)[0].reshape(6, -1).argmax(dim=1)
    labels[4] = (labels[4] + 1) % 10
    batches = [(xs[:2], labels[:2]), (xs[2:4], labels[2:4]), (xs[4:], labels[4:])]
    off = trainer.evaluate(m, batches)
    calm.backend.set_loss_kernels(True)
    with _Reads() as r:
        on = trainer.evaluate(m, batches)
    assert on == off == 5 / 6
    assert (r.reads, r.items) == (1, 0)


def test_launcher_with_device_metrics_makes_no_per_step_read_and_prints_the_epoch_mean(capsys):
    name = "tiny32_cls"
    g = load_golden(name)
    cfg = CONFIGS[name]
    S = cfg.seq_length
    gen = torch.Generator().manual_seed(3)
    data = torch.utils.data.TensorDataset(torch.randn(48, 3, S, S, generator=gen),
                                          torch.randint(0, cfg.out_features, (48,), generator=gen))
    calm.backend.set_loss_kernels(True)
    losses = []
    real_call = trainer.TrainStep.__call__

    def spy(self, x, y):
        out = real_call(self, x, y)
        losses.append(out[0].clone())                      # kept on the device: read after the run
        return out
    trainer.TrainStep.__call__ = spy
    try:
        with _Reads() as r:
            trainer.train(build_model(name, g, "cpu"), "fused", scheduler=False, use_gpu=True, dataset=data, epochs=1,
                          batch_size=8, num_classes=cfg.out_features, log_every=100, max_steps=6, device_metrics=True,
                          selfcheck=None)
    finally:
        trainer.TrainStep.__call__ = real_call
    out = capsys.readouterr().out
    assert len(losses) == 6
    # log_every=100: the one `Batch: 1` line reads its accuracy and its loss; nothing reads per step (six steps ran)
    print(f"\nreads {r.reads} items {r.items}")
    assert r.reads == 1 and r.items <= 2, (r.reads, r.items)
    line = [ln for ln in out.splitlines() if "Mean loss" in ln]
    assert len(line) == 1, out
    mean = float(re.search(r"Mean loss: ([-+0-9.eE]+|nan|inf)", line[0]).group(1))
    want = float(torch.stack(losses).double().mean())
    assert abs(mean - want) <= 1e-5 * abs(want), (mean, want)
    assert re.search(r"Dominant-class accuracy: \d+\.\d+%", line[0])
