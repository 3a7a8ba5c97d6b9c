"""The distillation kernels of csrc/loss.hip on the MI355X, through the C-ABI (HipBackend), against the float64 checker of
tests/distill_f64.py: every shape at which a code path can go wrong (one class, below a vector, the register-resident path
with and without a tail, more rows than the final workgroup has threads, rows read again per pass, the limit), temperatures,
weights, both modes, a bf16 teacher, row strides and bases the vector path does not serve; identical rows, offset logits,
ties, -inf and NaN; the two metric buffers; bit-reproducibility; the trainer step with the kernels on against the
stock-torch loss; the captured teacher; train(teacher=...) on the device collate.

Measured on MI355X: the figures each test prints; see DESIGN.md section 7, "Distillation loss"."""
import math
import re
from importlib import import_module

import pytest
import torch
import torch.nn.functional as F

import calm_vit_dte_amd as calm
import distill_f64 as D
import weights as W
from helpers import CONFIGS, load_golden, rel_err
from test_host_logic_cpu import build_model
from test_loss_cpu import _KeepGrads, ce_inputs

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
TOL = 1e-4                                    # the project's fp32 kernel tolerance (normalised inf-norm, helpers.rel_err)
RS = binding.DISTILL_ROW_STATS


@pytest.fixture(autouse=True)
def _restore_switch():
    prev = calm.backend.get_loss_kernels()
    yield
    calm.backend.set_loss_kernels(prev)
    calm.ops.set_noise_override(None)


def _distill(z, t, y, T, alpha, mode, dloss=3.0, metrics=None, dmetrics=None, dlogits=None):
    """calm_distill_fwd + _bwd on device tensors (any row stride): (loss, dlogits, row_stats)."""
    be = calm.backend.get_backend()
    B, C = z.shape
    row_stats = torch.full((B, RS), -7.0, device="cuda")
    loss = torch.full((), -1.0, device="cuda")
    if dlogits is None:
        dlogits = torch.full((B, C), -7.0, device="cuda")
    be.distill_fwd(z, t, y, T, alpha, mode, row_stats, loss, metrics, dmetrics, B, C)
    be.distill_bwd(z, t, y, T, alpha, mode, row_stats, torch.tensor([dloss], device="cuda"), dlogits, B, C)
    return loss, dlogits, row_stats


_CACHE = {}


def _case(v):
    """(z, t, y, float64 reference at dloss = 3) of one variant of distill_f64.VARIANTS: computed once, shared, not changed."""
    if v not in _CACHE:
        B, C, T, alpha, mode, scale, tdt = v
        z, t, y = D.inputs(B, C, scale, teacher=tdt)
        _CACHE[v] = (z, t, y, D.reference(z, t, y, T, alpha, mode, 3.0))
    return _CACHE[v]


def _strided(t, pad=3):
    """The same values in rows of stride C + pad (unit column stride)."""
    buf = torch.zeros(t.shape[0], t.shape[1] + pad, device="cuda", dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _off_by_one(t):
    """The same values, contiguous, with the base one element behind a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 1, device="cuda", dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:].view(t.shape)
    out.copy_(t)
    return out


@pytest.mark.parametrize("v", D.VARIANTS, ids=lambda v: "-".join(str(x) for x in v))
def test_forward_and_backward_against_float64(v):
    z, t, y, ref = _case(v)
    loss, dlogits, row_stats = _distill(z.cuda(), t.cuda(), y.cuda(), v[2], v[3], v[4])
    figures, failures = D.check(loss, dlogits, row_stats, ref, strict=False)
    print(f"\n{v}: " + " ".join(f"{k} {e:.2e}" for k, e in figures.items()))
    assert not failures, failures
    assert bool((row_stats[:, 7] == 0).all())


LAYOUT_CASES = [v for v in D.VARIANTS if (v[0], v[1]) in ((4, 1000), (5, 1001), (2, 21843)) and v[3] == 0.5 and v[5] == 1.0
                and v[2] in (2.0, 1.0)]


@pytest.mark.parametrize("layout", ["stride", "base"])
@pytest.mark.parametrize("v", LAYOUT_CASES, ids=lambda v: "-".join(str(x) for x in v))
def test_rows_the_vector_path_does_not_serve_keep_the_right_numbers(v, layout):
    z, t, y, ref = _case(v)
    move = _strided if layout == "stride" else _off_by_one
    zd, td, yd = move(z.cuda()), move(t.cuda()), move(y.cuda())
    assert layout == "stride" or zd.data_ptr() % 16 == 4
    dl = _off_by_one(torch.zeros(z.shape, device="cuda")) if layout == "base" else None
    loss, dlogits, row_stats = _distill(zd, td, yd, v[2], v[3], v[4], dlogits=dl)
    D.check(loss, dlogits, row_stats, ref, label=f"{v} {layout}")
    # one input at a time off the vector path: the others stay on it
    for which in range(3):
        args = [z.cuda(), t.cuda(), y.cuda()]
        args[which] = move(args[which])
        loss, dlogits, row_stats = _distill(*args, v[2], v[3], v[4])
        D.check(loss, dlogits, row_stats, ref, label=f"{v} {layout} input {which}")


@pytest.mark.parametrize("T", [0.5, 1.0, 4.0])
@pytest.mark.parametrize("B,C", [(4, 1000), (5, 1001), (2, 21843)])
def test_identical_student_and_teacher_rows_give_no_distillation_gradient(B, C, T):
    """alpha = 1, soft: the loss is T^2 KL(p || p) = 0 and the gradient T (pT - q) / B = 0.  pT and q come out of one
    expression on equal inputs, so both are zero to the last bit; the bounds are the issue's."""
    z, _, y = D.inputs(B, C, 3.0)
    dloss = 3.0
    loss, dlogits, _ = _distill(z.cuda(), z.clone().cuda(), y.cuda(), T, 1.0, "soft", dloss)
    worst, bound = float(dlogits.abs().max()), 4 * 2.0 ** -23 * dloss * T / B
    print(f"\nidentical rows {B}x{C} T={T}: |loss| {abs(float(loss)):.2e} (bound {1e-6 * T * T:.1e}) "
          f"max |dlogits| {worst:.2e} (bound {bound:.2e})")
    assert worst <= bound
    assert abs(float(loss)) <= 1e-6 * T * T


def _torch_chain(z, t, y, T, alpha):
    zt = z.clone().requires_grad_(True)
    loss = trainer.distill_loss_torch(zt, t, y, alpha, T, "soft")
    loss.backward()
    return loss.detach(), zt.grad


def test_offset_logits_keep_the_accuracy_of_torchs_own_fp32_chain():
    """z, t = 1e4 + randn: every maximum is subtracted before every exponential, so the kernels lose nothing to the offset.
    Bound (the rule of test_offset_logits_keep_the_accuracy_of_torchs_own_fp32_gradient): the error against float64 is at
    most 4x that of torch's fp32 chain on the same device and input, plus 1e-6."""
    B, C, T, alpha = 64, 1000, 2.0, 0.5
    z, t, y = D.inputs(B, C, 1.0)
    z, t = z + 1e4, t + 1e4
    ref = D.reference(z, t, y, T, alpha, "soft", 1.0)
    loss_t, dz_t = _torch_chain(z.cuda(), t.cuda(), y.cuda(), T, alpha)
    loss, dlogits, _ = _distill(z.cuda(), t.cuda(), y.cuda(), T, alpha, "soft", 1.0)
    e_k, e_t = rel_err(dlogits, ref["dlogits"]), rel_err(dz_t, ref["dlogits"])
    l_k, l_t = rel_err(loss, ref["loss"]), rel_err(loss_t, ref["loss"])
    print(f"\noffset 1e4: dlogits kernel {e_k:.2e} torch fp32 {e_t:.2e}; loss kernel {l_k:.2e} torch fp32 {l_t:.2e}")
    assert e_k <= 4 * e_t + 1e-6
    assert l_k <= 4 * l_t + 1e-6


def test_constructed_tie_minus_infinity_and_nan():
    C = 1000
    z, t, y = D.inputs(4, C, 1.0, seed=3)
    t[0, 17] = t[0, 901] = 9.0                              # a teacher tie: hard mode picks index 17
    t[1, 640] = 9.0
    z[1, 640] = 9.0                                         # (row 1 agrees with the teacher)
    t[2, 5] = -math.inf                                     # q = 0 there: the class adds nothing
    t[3, 999] = math.nan                                    # a NaN row
    z[3, int(t[3, :999].argmax())] = 9.0                    # its argmax would agree: it must not count
    zd, td, yd = z.cuda(), t.cuda(), y.cuda()
    for mode in ("hard", "soft"):
        dm = trainer.DistillMetrics(torch.device("cuda"))
        loss, dlogits, row_stats = _distill(zd, td, yd, 2.0, 0.5, mode, 1.0, dmetrics=dm.buf)
        assert math.isnan(float(loss)), mode
        assert not bool(torch.isfinite(dlogits[3]).any()) and bool(torch.isfinite(dlogits[:3]).all()), mode
        assert row_stats[:3, 5].tolist() == [17.0, 640.0, float(t[2].argmax())]
        want_agree = int((z[:3].argmax(1) == t[:3].argmax(1)).sum())
        assert want_agree >= 1 and dm.read()[2:] == (want_agree, 4), mode
        # without the NaN row: everything is finite and equals float64, ties and -inf included
        ref = D.reference(z[:3], t[:3], y[:3], 2.0, 0.5, mode, 1.0)
        assert math.isfinite(float(ref["loss"]))
        loss, dlogits, row_stats = _distill(zd[:3], td[:3], yd[:3], 2.0, 0.5, mode, 1.0)
        D.check(loss, dlogits, row_stats, ref, label=mode)
        if mode == "hard":
            assert float(dlogits[0, 17]) < 0 < float(dlogits[0, 901])       # the one-hot sits at the lowest index
        else:
            assert float(dlogits[2, 5]) > 0                                  # pT - 0
    # a NaN in the student or in the labels reaches the loss as well
    for which in (0, 2):
        args = [z[:3].clone(), t[:3].clone(), y[:3].clone()]
        args[which][1, 7] = math.nan
        assert math.isnan(float(_distill(*(a.cuda() for a in args), 2.0, 0.5, "soft")[0]))


def test_both_metric_buffers_after_two_calls_equal_the_float64_sums():
    m, dm = trainer.StepMetrics(torch.device("cuda")), trainer.DistillMetrics(torch.device("cuda"))
    want = dict(row_sum=0.0, ce_sum=0.0, d_sum=0.0, agree_y=0, agree_t=0)
    rows = 0
    for seed, (B, C) in enumerate(((257, 1000), (37, 1001))):
        z, t, y = D.inputs(B, C, 1.0, seed=seed)
        y = y + 1e-3 * torch.rand(B, C, generator=torch.Generator().manual_seed(seed))      # (tie-free labels)
        y[0] = 0.0
        y[0, int(z[0].argmax())] = 1.0
        t[1] = z[1]
        ref = D.reference(z, t, y, 2.0, 0.3, "soft")
        _distill(z.cuda(), t.cuda(), y.cuda(), 2.0, 0.3, "soft", metrics=m.buf, dmetrics=dm.buf)
        rows += B
        for k in want:
            want[k] += float(ref[k])
    loss_sum, agree, n, steps = m.read()
    ce_sum, d_sum, agree_t, n_t = dm.read()
    print(f"\nmetrics: loss {loss_sum} ({want['row_sum']}) CE {ce_sum} ({want['ce_sum']}) D {d_sum} ({want['d_sum']}) "
          f"agree {agree} / {agree_t}")
    assert (agree, n, steps, agree_t, n_t) == (want["agree_y"], rows, 2, want["agree_t"], rows)
    assert agree >= 2 and agree_t >= 2
    for got, k in ((loss_sum, "row_sum"), (ce_sum, "ce_sum"), (d_sum, "d_sum")):
        assert abs(got - want[k]) <= 1e-5 * abs(want[k]), k


def test_two_launches_give_the_same_bits():
    for B, C, mode, tdt in ((257, 1000, "soft", "f32"), (2, 21843, "soft", "bf16"), (5, 1001, "hard", "f32")):
        z, t, y = D.inputs(B, C, 2.0, teacher=tdt)
        a = _distill(z.cuda(), t.cuda(), y.cuda(), 2.0, 0.5, mode)
        b = _distill(z.cuda(), t.cuda(), y.cuda(), 2.0, 0.5, mode)
        for u, v in zip(a, b):
            assert torch.equal(u, v), (B, C, mode)


def test_backend_checks_its_arguments():
    be = calm.backend.get_backend()
    z, t, y = (v.cuda() for v in D.inputs(3, 10))
    rs, loss, dz = torch.empty(3, RS, device="cuda"), torch.empty((), device="cuda"), torch.empty(3, 10, device="cuda")
    one = torch.ones(1, device="cuda")
    assert be.distill_scratch_floats(3, 10) == 15
    with pytest.raises(ValueError, match="dlogits"):
        be.distill_bwd(z, t, y, 1.0, 0.5, "soft", rs, one, torch.empty(3, 13, device="cuda")[:, :10], 3, 10)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        be.distill_fwd(z.cpu(), t, y, 1.0, 0.5, "soft", rs, loss, None, None, 3, 10)
    with pytest.raises(TypeError, match="fp32"):
        be.distill_fwd(z, t.half(), y, 1.0, 0.5, "soft", rs, loss, None, None, 3, 10)
    with pytest.raises(TypeError, match="fp32"):
        be.distill_fwd(z.bfloat16(), t, y, 1.0, 0.5, "soft", rs, loss, None, None, 3, 10)
    with pytest.raises(ValueError, match="mode"):
        be.distill_fwd(z, t, y, 1.0, 0.5, "both", rs, loss, None, None, 3, 10)
    with pytest.raises(ValueError, match="unit column stride"):
        be.distill_fwd(z, t.t().contiguous().t(), y, 1.0, 0.5, "soft", rs, loss, None, None, 3, 10)
    with pytest.raises(RuntimeError, match="calm_distill_fwd"):
        be.distill_fwd(z, t, y, 0.0, 0.5, "soft", rs, loss, None, None, 3, 10)
    be.distill_fwd(z, t, y, 1.0, 0.5, "soft", rs, loss, None, None, 3, 10)
    be.distill_bwd(z, t, y, 1.0, 0.5, "soft", rs, one, dz, 3, 10)
    assert bool(torch.isfinite(dz).all())


# ---- the trainer ---------------------------------------------------------------------------------------------------------
NAME = "nano48_cls"


def _teacher(name=NAME, device="cuda"):
    """The fixture model with other weights than the student's."""
    m = build_model(name, load_golden(name), device)
    g = torch.Generator().manual_seed(1234)
    with torch.no_grad():
        for p in m.parameters():
            p.add_((0.05 * torch.randn(p.shape, generator=g)).to(p.device))
    return m


def _first_step(on, amp, distill, teacher_graph=False, bs=4):
    """(loss, gradients after clipping, teacher agreement count) of the first DistillTrainStep of the fixture models."""
    cfg = CONFIGS[NAME]
    calm.backend.set_loss_kernels(on)
    m = build_model(NAME, load_golden(NAME), "cuda").train()
    teacher = _teacher()
    x = torch.from_numpy(W.make_input((bs, 3, cfg.seq_length, cfg.seq_length), 2)).cuda()
    y = ce_inputs(bs, cfg.out_features, 1.0)[1].cuda()
    opt = _KeepGrads([p for p in m.parameters() if p.requires_grad], lr=0.0)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0) if amp else None
    dm = trainer.DistillMetrics(torch.device("cuda"))
    calm.ops.set_noise_override(W.NoiseStream(7))
    try:
        step = trainer.DistillTrainStep(m, opt, teacher, scaler=scaler, autocast_dtype=torch.bfloat16 if amp else None,
                                        teacher_graph=teacher_graph, distill_metrics=dm, **distill)
        loss, _ = step(x, y)
        if teacher_graph:
            assert step.teacher.graph is not None
            step.teacher.close()
    finally:
        calm.ops.set_noise_override(None)
    assert not any(p.requires_grad for p in teacher.parameters()) and teacher.training      # (the flag is put back)
    return loss, dict(zip([n for n, p in m.named_parameters() if p.requires_grad], opt.kept)), dm.read()


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "autocast+GradScaler"])
@pytest.mark.parametrize("distill", [dict(alpha=0.5, temperature=2.0, mode="soft"), dict(alpha=0.5, mode="hard")],
                         ids=["soft", "hard"])
def test_first_trainer_step_with_the_kernels_on_equals_the_torch_loss_step(distill, amp):
    (loss_off, grads_off, dm_off), (loss_on, grads_on, dm_on) = (_first_step(on, amp, distill) for on in (False, True))
    worst = max(rel_err(grads_on[n], grads_off[n]) for n in grads_off)
    print(f"\n{distill['mode']} amp={amp}: loss {rel_err(loss_on, loss_off):.2e} worst parameter gradient {worst:.2e}")
    assert rel_err(loss_on, loss_off) <= TOL
    for n in grads_off:
        assert rel_err(grads_on[n], grads_off[n]) <= TOL, n
    assert dm_off == (0.0, 0.0, 0, 0) and dm_on[3] == 4            # only the kernels feed the buffer


def test_captured_teacher_gives_the_eager_teachers_bits():
    distill = dict(alpha=0.5, temperature=2.0, mode="soft")
    be = calm.backend.get_backend()
    prev = be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, 1)      # (the student's k-split GEMMs: no fp32 atomics, so that
    try:                                                         # two runs of ONE configuration give the same bits)
        (loss_e, grads_e, dm_e), (loss_g, grads_g, dm_g) = (_first_step(True, True, distill, teacher_graph=g)
                                                            for g in (False, True))
    finally:
        be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, prev)
    assert torch.equal(loss_e, loss_g) and dm_e == dm_g
    for n in grads_e:
        assert torch.equal(grads_e[n], grads_g[n]), n


def test_launcher_with_a_teacher_on_the_device_collate_prints_the_recounted_agreement(capsys):
    cfg = CONFIGS[NAME]
    S = cfg.seq_length
    gen = torch.Generator().manual_seed(3)
    data = torch.utils.data.TensorDataset(torch.randint(0, 256, (32, 3, S, S), generator=gen, dtype=torch.uint8),
                                          torch.randint(0, cfg.out_features, (32,), generator=gen))
    calm.backend.set_loss_kernels(True)
    seen = []
    real = trainer.distillation_loss

    def spy(logits, teacher_logits, *a, **kw):
        seen.append((logits.detach().clone(), teacher_logits.detach().clone()))
        return real(logits, teacher_logits, *a, **kw)
    trainer.distillation_loss = spy
    teacher = _teacher(device="cpu").train()
    try:
        out = trainer.train(build_model(NAME, load_golden(NAME), "cpu"), "fused", scheduler=False, use_gpu=True, dataset=data,
                            epochs=1, batch_size=8, num_classes=cfg.out_features, log_every=100, max_steps=4,
                            device_collate=True, device_metrics=True, selfcheck=None, teacher=teacher,
                            distill={"alpha": 0.5, "temperature": 2.0, "graph": True})
    finally:
        trainer.distillation_loss = real
    text = capsys.readouterr().out
    assert len(seen) == 4 and all(z.shape == (8, cfg.out_features) == t.shape for z, t in seen)
    assert teacher.training and next(teacher.parameters()).device.type == "cpu" and out.training
    line = [ln for ln in text.splitlines() if "Teacher agreement" in ln]
    assert len(line) == 1 and len([ln for ln in text.splitlines() if "Mean loss" in ln]) == 1, text
    agree = sum(int((z.argmax(1) == t.argmax(1)).sum()) for z, t in seen)
    got = float(re.search(r"Teacher agreement: ([0-9.]+)%", line[0]).group(1))
    assert abs(got - 100.0 * agree / 32) < 1e-3, (got, agree)
    ce = float(re.search(r"Mean CE: ([-+0-9.eE]+)", line[0]).group(1))
    want_ce = sum(float(F.cross_entropy(z, torch.zeros_like(z).scatter_(1, z.argmax(1, keepdim=True), 1.0), reduction="sum"))
                  for z, _ in seen)
    assert math.isfinite(ce) and ce >= want_ce / 32 * (1 - 1e-5)   # (the CE against any labels is at least -log max p)
