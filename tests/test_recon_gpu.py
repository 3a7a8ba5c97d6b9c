"""The generative job on the MI355X: calm_recon_metrics and the rows Huber pair through the C-ABI (HipBackend), and
trainer.ReconMetrics / RegTrainStep on row tokens / evaluate(recon=True) / train(task="reg") on top of them.

calm_recon_metrics is checked against the float64 checker (tests/recon_f64.py: explicit 11 x 11 windows, centred moments)
on every shape x {rows, NCHW} target x {fp32, bf16} tokens x {16-byte aligned bases, bases offset by 4 bytes — the entry
point takes any element-aligned base}.  The integer-valued slots (images, non-finite images, elements) are exact.  The bound
of the others is measured, not fixed: the yardstick is the error of trainer.recon_metrics_torch — the plain fp32 conv2d /
elementwise composition — against the checker on the same inputs, and the kernel may err by 4 x that plus 1e-6 of the slot's
magnitude (bf16 tokens widen exactly: the same rule on the widened values).  No case and no slot is left out.
Measured on MI355X: see DESIGN.md, "Generative job"."""
import json
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import recon_f64 as F
import weights as W
from helpers import CONFIGS, load_golden
from test_host_logic_cpu import build_model

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
DTYPES = [torch.float32, torch.bfloat16]
_CASES = {}


@pytest.fixture(autouse=True)
def _restore_switch():
    prev = calm.backend.get_loss_kernels()
    yield
    calm.backend.set_loss_kernels(prev)


def _case(B, S, layout, dtype):
    """(tokens, target, reference, bound, yardstick), computed once per case and left unchanged."""
    key = (B, S, layout, dtype)
    if key not in _CASES:
        tokens, target = F.make_case(B, S, layout, dtype, nonfinite=B >= 3)
        ref = F.reference(tokens, target)
        _CASES[key] = (tokens, target, ref) + F.allowance(tokens, target, ref, trainer.recon_metrics_torch)
    return _CASES[key]


def _offset(t, aligned):
    """The values of t on the device at a 16-byte aligned base, or 4 bytes behind one."""
    shift = 0 if aligned else 4 // t.element_size()
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device="cuda")
    view = buf[shift:shift + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (0 if aligned else 4) and view.is_contiguous()
    return view


def _kernel(tokens, target, ssim=True, sums=None):
    be = calm.backend.get_backend()
    B, S = tokens.shape[0], tokens.shape[1]
    sums = torch.zeros(8, dtype=torch.float64, device="cuda") if sums is None else sums
    be.recon_metrics(tokens, target, binding.RECON_NCHW if target.dim() == 4 else binding.RECON_ROWS, F.MEAN, F.STD, 1.0,
                     ssim, sums, B, S)
    return sums


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["rows", "nchw"])
@pytest.mark.parametrize("B,S", F.SHAPES + F.EXTRA_SHAPES)
def test_kernel_against_the_float64_checker(B, S, layout, dtype, aligned):
    tokens, target, ref, bound, yard = _case(B, S, layout, dtype)
    got = _kernel(_offset(tokens, aligned), _offset(target, aligned))
    err = F.errors(got, ref)
    print(f"\ncalm_recon_metrics {B}x{S} {layout} {str(dtype)[6:]} aligned={aligned}: slots 2,3,4,6,7 yardstick "
          f"{np.array2string(yard[[2, 3, 4, 6, 7]], precision=3)} kernel {np.array2string(err[[2, 3, 4, 6, 7]], precision=3)} "
          f"values {np.array2string(ref[[2, 3, 4, 6, 7]], precision=6)}")
    assert F.mismatches(got, ref, bound) == []
    assert (int(got[0]), int(got[1]), int(got[5])) == (B, 2 if B >= 3 else 0, (B - (2 if B >= 3 else 0)) * 3 * S * S)
    no_ssim = _kernel(_offset(tokens, aligned), _offset(target, aligned), ssim=False)
    assert float(no_ssim[7]) == 0.0 and torch.equal(no_ssim[:7], got[:7])       # the other slots do not depend on the flag


@pytest.mark.parametrize("layout", ["rows", "nchw"])
def test_bf16_tokens_two_bytes_behind_an_aligned_base(layout):
    """bf16 tokens are read as aligned 32-bit words where the base allows it and element by element otherwise: the base
    here allows only the latter (the (1, 11) case above reaches it through its odd element count)."""
    tokens, target, ref, bound, _ = _case(2, 44, layout, torch.bfloat16)
    buf = torch.zeros(tokens.numel() + 8, dtype=torch.bfloat16, device="cuda")
    view = buf[1:1 + tokens.numel()].view(tokens.shape)
    view.copy_(tokens)
    assert view.data_ptr() % 4 == 2
    got = _kernel(view, target.cuda())
    assert F.mismatches(got, ref, bound) == []
    assert torch.equal(got, _kernel(tokens.cuda(), target.cuda()))            # the same values, the same bits


def test_small_images_are_served_without_ssim_and_refused_with_it():
    tokens, target = F.make_case(3, 6, "nchw")
    ref = F.reference(tokens, target, ssim=False)
    bound, _ = F.allowance(tokens, target, ref, trainer.recon_metrics_torch, ssim=False)
    sums = torch.full((8,), 2.0, dtype=torch.float64, device="cuda")
    _kernel(tokens.cuda(), target.cuda(), ssim=False, sums=sums)
    assert float(sums[7]) == 2.0                                              # slot 7 is left alone
    assert F.mismatches(sums.cpu() - 2.0, ref, bound + 1e-12, ssim=False) == []
    with pytest.raises(RuntimeError, match="-3"):
        _kernel(tokens.cuda(), target.cuda(), ssim=True)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("n", F.HUBER_SIZES)
def test_rows_huber_forward_and_backward_against_float64(n, aligned):
    """The bound follows the loss kernels' rule (4 x torch + 1e-6): torch's fp32 huber_loss on the same values
    is the yardstick of the loss; a gradient element is one subtraction, one clamp and one product — 1e-6 of the largest."""
    a, b = F.huber_case(n)
    want, dwant = F.huber_reference(a, b)
    yard = abs(float(torch.nn.functional.huber_loss(a, b)) - want)
    be = calm.backend.get_backend()
    ta, tb = _offset(a, aligned), _offset(b, aligned)
    loss = torch.zeros((), device="cuda")
    dtok = _offset(torch.zeros(n), aligned)
    be.huber_rows_fwd(ta, tb, 1.0, loss, n)
    be.huber_rows_bwd(ta, tb, 1.0, torch.ones((), device="cuda"), dtok, n)
    err = abs(float(loss) - want)
    gerr = float((dtok.cpu().double() - dwant).abs().max())
    print(f"\ncalm_recon_huber_rows n={n} aligned={aligned}: loss err {err:.3e} (torch {yard:.3e}), grad err {gerr:.3e}")
    assert err <= 4 * yard + 1e-6 * abs(want)
    assert gerr <= 1e-6 * float(dwant.abs().max())
    loss2 = torch.zeros((), device="cuda")
    be.huber_rows_fwd(ta, tb, 1.0, loss2, n)
    assert torch.equal(loss, loss2)
    # through autograd, with a scaled upstream gradient (GradScaler's scale arrives as a device scalar)
    x = ta.clone().requires_grad_(True)
    (calm.ops.HuberRowsFn.apply(x, tb, 1.0) * 8.0).backward()
    assert float((x.grad.cpu().double() - 8.0 * dwant).abs().max()) <= 8e-6 * float(dwant.abs().max())


def test_split_updates_repeat_runs_and_a_captured_update():
    calm.backend.set_loss_kernels(True)
    B, S = 5, 44
    tokens, target = F.make_case(B, S, "rows", torch.bfloat16, seed=3)
    tokens[3, 7, 11] = float("nan")
    ref = F.reference(tokens, target)
    bound, _ = F.allowance(tokens, target, ref, trainer.recon_metrics_torch)
    tokens, target = tokens.cuda(), target.cuda()

    def run(parts):
        m = trainer.ReconMetrics(F.MEAN, F.STD, device="cuda")
        for p in parts:
            m.update(tokens[p], target[p])
        return m
    one, again, split = run([slice(0, B)]), run([slice(0, B)]), run([slice(0, 2), slice(2, B)])
    assert F.mismatches(one.sums, ref, bound) == [] and F.mismatches(split.sums, ref, bound) == []
    assert torch.equal(one.sums, again.sums)                                 # bit for bit
    assert torch.equal(split.sums[[0, 1, 5]], one.sums[[0, 1, 5]])
    # the per-image values do not depend on the batch they arrive in; only the double additions are grouped differently
    assert float((split.sums - one.sums).abs().max()) <= 1e-12 * float(one.sums.abs().max())
    # captured: warmed up on a side stream (the records are allocated there), zeroed, captured, replayed twice
    m = trainer.ReconMetrics(F.MEAN, F.STD, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.update(tokens, target)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    m.reset()
    records = m._records.data_ptr()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.update(tokens, target)
    assert m._records.data_ptr() == records
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(m.sums, 2 * one.sums)                                  # (x + x is exact)
    rep, rep1 = m.read(), one.read()
    assert rep["n"] == 2 * B and rep["nonfinite"] == 2 and rep["psnr"] == rep1["psnr"] and rep["ssim"] == rep1["ssim"]


def test_evaluate_recon_lean_graph_on_the_nano48_model_equals_recon_metrics_on_its_outputs():
    name = "nano48_gen"
    cfg = CONFIGS[name]
    S = cfg.seq_length
    m = build_model(name, load_golden(name), "cuda").train()
    xs = torch.from_numpy(W.make_input((10, 3, S, S), 5)).cuda()
    with torch.no_grad():                                                     # (batch by batch, as the loop below sees them)
        tokens = torch.cat([trainer.Predictor(m)(xs[lo:hi])[0].reshape(hi - lo, S, 3 * S).float()
                            for lo, hi in ((0, 4), (4, 8), (8, 10))])
    batches = [xs[0:4], (xs[4:8], None), xs[8:10]]                            # two replays, one ragged batch
    ref = F.reference(tokens, xs, trainer.DeviceCollate.MEAN, trainer.DeviceCollate.STD)
    bound, _ = F.allowance(tokens, xs, ref, trainer.recon_metrics_torch, mean=trainer.DeviceCollate.MEAN,
                           std=trainer.DeviceCollate.STD)
    reports = {}
    for on in (True, False):
        calm.backend.set_loss_kernels(on)
        direct = trainer.ReconMetrics(trainer.DeviceCollate.MEAN, trainer.DeviceCollate.STD, device="cuda")
        for lo, hi in ((0, 4), (4, 8), (8, 10)):
            direct.update(tokens[lo:hi], xs[lo:hi])
        assert F.mismatches(direct.sums, ref, bound) == []
        rep = trainer.evaluate(m, batches, lean=True, graph=True, recon=True)
        assert m.training
        assert rep == direct.read()                                           # the same batches, the same calls
        assert rep["n"] == 10 and rep["nonfinite"] == 0 and 0.0 < rep["huber"] and rep["psnr"] > 0.0
        reports[on] = rep
    for k in ("huber", "mae", "mse", "psnr"):
        assert abs(reports[True][k] - reports[False][k]) <= 1e-5 * abs(reports[False][k]), k
    assert abs(reports[True]["ssim"] - reports[False]["ssim"]) <= 2e-5
    rows = [x.permute(0, 2, 3, 1).reshape(x.shape[0], S, 3 * S).contiguous() for x in (xs[0:4], xs[4:8], xs[8:10])]
    calm.backend.set_loss_kernels(True)
    assert trainer.evaluate(m, rows, lean=True, recon=True) == reports[True]   # row tokens in: the same image, the same tallies


def test_reg_train_step_on_row_tokens_with_the_loss_kernels_on_and_off():
    """The same step twice from the same weights and noise: losses and gradients agree within the Huber tolerance — the
    loss within 4 x torch's own fp32 error + 1e-6 (both sides are fp32 sums of the same 13824 terms; 1e-5 relative stands
    for that here, as tests/test_loss_gpu.py does for the image pair) and the gradients, which differ only through the
    loss gradient's last bits, within 1e-4 of the largest element of each tensor."""
    name = "nano48_gen"
    g = load_golden(name)
    S = CONFIGS[name].seq_length
    x = torch.from_numpy(W.make_input((2, 3, S, S), 2)).cuda()
    rows = x.permute(0, 2, 3, 1).reshape(2, S, 3 * S).contiguous()
    runs = {}
    for on in (False, True):
        calm.backend.set_loss_kernels(on)
        m = build_model(name, g, "cuda").train()
        calm.ops.set_noise_override(W.NoiseStream(7))
        try:
            y_hat, kl = m(rows)
            loss = trainer.RegTrainStep._huber(y_hat, None, rows) + kl * 0.1
            loss.backward()
        finally:
            calm.ops.set_noise_override(None)
        runs[on] = (float(loss), {k: p.grad.detach().clone() for k, p in m.named_parameters()})
        if on:                                                               # the image step from the same state: the same loss
            m2 = build_model(name, g, "cuda").train()
            calm.ops.set_noise_override(W.NoiseStream(7))
            try:
                y2, kl2 = m2(x)
                img = y2.reshape(-1, S, S, 3).permute(0, 3, 1, 2)
                loss_img = float(trainer.RegTrainStep._huber(y2, img, x) + kl2 * 0.1)
            finally:
                calm.ops.set_noise_override(None)
    (l0, g0), (l1, g1) = runs[False], runs[True]
    print(f"\nRegTrainStep rows: loss torch {l0!r} kernels {l1!r} image-layout kernels {loss_img!r}")
    assert abs(l1 - l0) <= 1e-5 * abs(l0) and abs(loss_img - l0) <= 1e-5 * abs(l0)
    for k in g0:
        assert float((g1[k] - g0[k]).abs().max()) <= 1e-4 * float(g0[k].abs().max()) + 1e-9, k


def test_mixup_with_lam_one_is_the_identity_on_a_uint8_batch():
    """What train(task="reg", device_collate=True) hands the collate: (mix-up, lam = 1, no box).  The output is the
    normalised, cropped, flipped sample whatever its partner holds."""
    gen = torch.Generator().manual_seed(2)
    u8 = torch.randint(0, 256, (4, 3, 20, 20), dtype=torch.uint8, generator=gen)
    other = torch.cat([u8[:1], u8[1:].flip(0)])
    outs = []
    for batch in (u8, other):
        dc = trainer.DeviceCollate(num_classes=10, seed=5)
        d = dc.draw(4, 16, 16)
        x, y = dc(batch.cuda(), torch.zeros(4, dtype=torch.int64, device="cuda"), decisions=(1, 1.0, None, d[3]),
                  crop=(16, 16), tokens=True)
        outs.append((x, dc.last_corners.cpu(), d[3]))
        assert torch.equal(y, torch.nn.functional.one_hot(torch.zeros(4, dtype=torch.int64), 10).float().cuda())
    (x, corners, flips), (x2, _, _) = outs
    assert torch.equal(x[0], x2[0])                                          # sample 0 does not see its partner
    mean = torch.tensor(trainer.DeviceCollate.MEAN).view(3, 1, 1)
    std = torch.tensor(trainer.DeviceCollate.STD).view(3, 1, 1)
    for b in range(4):
        y0, x0 = int(corners[b, 0]), int(corners[b, 1])
        img = (u8[b, :, y0:y0 + 16, x0:x0 + 16].float() / 255.0 - mean) / std
        img = img.flip(-1) if int(flips[b]) else img
        assert torch.allclose(x[b].cpu(), img.permute(1, 2, 0).reshape(16, 48), rtol=0, atol=2e-6), b


def test_train_reg_with_device_collate_runs_three_steps_and_writes_samples_and_the_validation_log(tmp_path, capsys):
    name = "nano48_gen"
    S = CONFIGS[name].seq_length
    gen = torch.Generator().manual_seed(0)
    data = torch.utils.data.TensorDataset(torch.randint(0, 256, (12, 3, S + 4, S + 4), generator=gen, dtype=torch.uint8),
                                          torch.zeros(12, dtype=torch.int64))
    val = torch.utils.data.TensorDataset(torch.randn(5, 3, S, S, generator=gen) * 0.5, torch.zeros(5, dtype=torch.int64))
    calm.backend.set_loss_kernels(True)
    m = build_model(name, load_golden(name), "cpu")
    before = {k: v.clone() for k, v in m.state_dict().items()}
    path = str(tmp_path / "model_reg.pth")
    out = trainer.train(m, "fused", scheduler=False, use_gpu=True, dataset=data, epochs=1, batch_size=4, task="reg",
                        device_collate=True, crop=(S, S), log_every=1, checkpoint_path=path, selfcheck=None,
                        samples_dir=str(tmp_path / "samples"), val_dataset=val, val_batch_size=4, ema=0.9)
    text = capsys.readouterr().out
    losses = [float(line.split("Loss: ")[1]) for line in text.splitlines() if line.startswith("Epoch: 1, Batch:")]
    assert len(losses) == 3 and all(np.isfinite(losses)) and "Accuracy" not in text
    assert any(not torch.equal(out.state_dict()[k], before[k]) for k in before)
    assert sorted(os.listdir(tmp_path / "samples")) == [f"sample_{i}.png" for i in range(4)]
    lines = [json.loads(x) for x in open(tmp_path / "model_reg_val.jsonl")]
    assert len(lines) == 1 and lines[0]["epoch"] == 1 and lines[0]["step"] == 3 and lines[0]["n"] == 5
    assert lines[0]["nonfinite"] == 0 and np.isfinite([lines[0][k] for k in ("huber", "mae", "mse", "psnr", "ssim")]).all()
    assert "ema" in lines[0] and os.path.exists(tmp_path / "model_reg_best.pth") and os.path.exists(tmp_path / "model_reg_ema_best.pth")
