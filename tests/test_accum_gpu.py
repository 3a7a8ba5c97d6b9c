"""Gradient accumulation on the GPU: calm_grad_accum (csrc/accum.hip) against the float64 checker of tests/accum_f64.py on
the optimizer-step case table, and AccumTrainStep(accumulate=2) with FusedClipAdamWindow against the unfused path (in-backward
spectral-norm correction, autograd accumulation, torch AdamW) on the golden models.  tests/test_accum_cpu.py proves the
checker on an emulation and on planted faults.  Accumulators and gradients sit between NaN-pattern guards."""
from importlib import import_module

import pytest
import torch

import calm_vit_dte_amd as calm
import accum_f64 as af
import tail_f64 as tf
import weights as W
from helpers import load_golden, rel_err
from oracle import calm_oracle as O
from test_host_logic_cpu import build_model
from test_rowwise_f64_gpu import DEV, GUARD, place
from test_trainer_gpu import _batch

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
TABLE = af.optim_table()


@pytest.fixture(scope="module")
def hip():
    return calm.backend.get_backend()


class Arena:
    """Tensors laid out in ONE device buffer, each starting `off` floats past a 16-byte boundary behind at least GUARD
    guard elements (a NaN pattern no kernel produces): one upload, one download, every gap must come back bit for bit."""

    def __init__(self, tensors, offsets):
        self.spans, at = [], 0
        for t, off in zip(tensors, offsets):
            at = -(-(at + GUARD) // 4) * 4 + off
            self.spans.append((at, at + t.numel()))
            at += t.numel()
        host = torch.full((at + GUARD,), tf.FILL[torch.float32], dtype=torch.int32)
        self.gap = torch.ones(at + GUARD, dtype=torch.bool)
        for t, (lo, hi) in zip(tensors, self.spans):
            host[lo:hi] = t.reshape(-1).view(torch.int32)
            self.gap[lo:hi] = False
        self.before = host
        self.buf = host.view(torch.float32).to(DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[lo:hi] for lo, hi in self.spans]

    def read(self):
        """the tensors now (CPU, one flat tensor each); the gaps must be untouched"""
        now = self.buf.cpu()
        assert torch.equal(now.view(torch.int32)[self.gap], self.before[self.gap]), "write outside a tensor"
        return [now[lo:hi].clone() for lo, hi in self.spans]

    def unchanged(self):
        return torch.equal(self.buf.cpu().view(torch.int32), self.before)


class Device:
    """The table's state on the device, the optimizer's plan over it, and NaN-filled accumulators `acc_off` floats off
    16-byte alignment."""

    def __init__(self, hip, recs, acc_off):
        self.hip = hip
        zeros = [0] * len(recs)
        self.p, self.m, self.v = (Arena([r[k] for r in recs], zeros) for k in ("param", "exp_avg", "exp_avg_sq"))
        self.sn = [None if r["sn"] is None else (place(r["sn"][0]), place(r["sn"][1]), place(r["sn"][2]), r["sn"][3], r["sn"][4])
                   for r in recs]
        self.plan = hip.optim_plan([dict(param=p, exp_avg=m, exp_avg_sq=v, sn=s)
                                    for p, m, v, s in zip(self.p.views, self.m.views, self.v.views, self.sn)])
        self.acc = Arena([torch.full((e["numel"],), float("nan")) for e in TABLE], [acc_off] * len(TABLE))
        assert all((a.data_ptr() % 16 != 0) == bool(acc_off) for a in self.acc.views)
        self.acc_ptrs = torch.tensor([a.data_ptr() for a in self.acc.views], dtype=torch.int64, device=DEV)

    def forward_state(self, recs):
        """u, v, sigma of another forward, in place (the table keeps its addresses)."""
        for s, r in zip(self.sn, recs):
            if s is not None:
                for dst, src in zip(s[:3], r["sn"][:3]):
                    dst.copy_(src)

    def accum(self, grads, first):
        G = Arena(grads, [e["goff"] for e in TABLE])
        self.hip.grad_accum(self.plan, G.views, self.acc_ptrs, first)
        out = self.acc.read()
        assert G.unchanged() and all(a.unchanged() for a in (self.p, self.m, self.v)), "an input was written"
        return out


@pytest.fixture(scope="module")
def case():
    """Two micro-batches on one table: the same parameters, other u, v, sigma and gradients; the float64 reference of the
    first call, computed once."""
    recs1, recs2 = af.optim_state(TABLE), af.optim_state(TABLE, seed=1)
    for a, b in zip(recs1, recs2):
        b["param"] = a["param"]
    g1, g2 = af.optim_grads(TABLE, recs1, seed=1), af.optim_grads(TABLE, recs2, seed=2)
    nan = [torch.full((e["numel"],), float("nan")) for e in TABLE]
    ref1, bound1 = af.accum_reference(recs1, g1, nan, True)
    return dict(recs1=recs1, recs2=recs2, g1=g1, g2=g2, ref1=ref1, bound1=bound1)


def _two_calls(hip, case, acc_off):
    dev = Device(hip, case["recs1"], acc_off)
    acc1 = dev.accum(case["g1"], True)                    # over NaN-filled accumulators
    assert all(bool(torch.isfinite(a).all()) for a in acc1)
    worst, failures = af.check_accum(acc1, case["ref1"], case["bound1"], strict=False)
    print(f"\n[accum_f64] off={acc_off} first=1: {worst}")
    assert not failures, failures
    dev.forward_state(case["recs2"])
    acc2 = dev.accum(case["g2"], False)
    ref2, bound2 = af.accum_reference(case["recs2"], case["g2"], acc1, False)     # starts from the device's first result
    worst, failures = af.check_accum(acc2, ref2, bound2, strict=False)
    print(f"[accum_f64] off={acc_off} first=0: {worst}")
    assert not failures, failures
    for e, a1, a2, x1, x2 in zip(TABLE, acc1, acc2, case["g1"], case["g2"]):
        if e["sn"] is None:
            assert torch.equal(a1, x1) and torch.equal(a2, x1 + x2), e
    return acc1, acc2


@pytest.fixture(scope="module")
def aligned(hip, case):
    assert hip.lib.calm_optim_chunk_elems() == af.OPT_CHUNK
    return _two_calls(hip, case, 0)


def test_kernel_against_the_checker_and_two_runs_are_equal(hip, case, aligned):
    again = _two_calls(hip, case, 0)
    for a, b in zip(aligned[0] + aligned[1], again[0] + again[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_misaligned_accumulators_take_the_scalar_path_to_the_same_bits(hip, case, aligned):
    """Views offset by one float: same bounds — and, since the result per element does not depend on the path, same bits."""
    got = _two_calls(hip, case, 1)
    for a, b in zip(aligned[0] + aligned[1], got[0] + got[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- the step classes ------------------------------------------------------------------------------------------------
@pytest.fixture()
def deterministic(hip):
    prev = hip.gemm_set_option(hip.GEMM_OPT_DETERMINISTIC, 1)
    yield
    hip.gemm_set_option(hip.GEMM_OPT_DETERMINISTIC, prev)
    calm.ops.set_noise_override(None)


def _micro_batches(name):
    _, x, y = _batch(name, bs=8)                          # the batch of the single-batch optimizer test, in two halves
    return [(x[:4].cuda(), y[:4].cuda()), (x[4:].cuda(), y[4:].cuda())]


@pytest.mark.parametrize("name", ["tiny32_cls", "nano48_cls"])
def test_fused_window_matches_the_unfused_window(name, deterministic):
    """Accumulators against the unfused path's summed .grad (rel_err < 1e-3 per tensor, the fp32 parity bar), then the
    parameter updates behind the boundary with the criterion of test_fused_optimizer_side_step_matches_clip_plus_adamw:
    per element 1e-3 * lr + 1e-7, at most 0.1 % outliers.  The gradient tail stays armed in every micro-backward."""
    g = load_golden(name)
    mbs = _micro_batches(name)
    start = {k: v.clone() for k, v in build_model(name, g, "cuda").state_dict().items()}
    # the summed gradients of the unfused path: in-backward correction, autograd accumulation, no step
    m_sum = build_model(name, g, "cuda").train()
    for i, (x, y) in enumerate(mbs):
        calm.ops.set_noise_override(W.NoiseStream(30 + i))
        trainer.soft_target_cross_entropy(m_sum(x)[0].squeeze(), y).backward()
    want = [p.grad.clone() for p in m_sum.parameters() if p.requires_grad]
    # the unfused window
    m_ref = build_model(name, g, "cuda").train()
    step_ref = trainer.AccumTrainStep(m_ref, trainer.make_optimizer(m_ref), accumulate=2)
    for i, (x, y) in enumerate(mbs):
        calm.ops.set_noise_override(W.NoiseStream(30 + i))
        step_ref(x, y)
    # the fused window
    m = build_model(name, g, "cuda").train()
    opt = trainer.FusedClipAdamWindow(m, lr=3.1e-3, weight_decay=0.02, betas=(0.9, 0.98), max_norm=1.0)
    step = trainer.AccumTrainStep(m, opt, accumulate=2)
    try:
        for i, (x, y) in enumerate(mbs):
            calm.ops.set_noise_override(W.NoiseStream(30 + i))
            flushes = calm.ops._tail.flushes
            step(x, y)
            assert calm.ops._tail.flushes > flushes, f"gradient tail not armed in micro-backward {i}"
            assert step.boundary == (i == 1) and all(p.grad is None for p in opt.params)
        assert float(opt.stats[1]) == 0.0 and opt.step_count == 1 and opt.window == 0
        for k, (a, w) in enumerate(zip(opt._acc, want)):       # the step reads the accumulators and leaves them
            assert rel_err(a, w) < 1e-3, (k, tuple(a.shape), rel_err(a, w))
    finally:
        opt.close()
    sd_r, sd_f = m_ref.state_dict(), m.state_dict()
    bad = tot = 0
    for k in sd_r:
        if O.is_buffer(k):
            assert rel_err(sd_f[k], sd_r[k]) < 1e-4, k
            continue
        d_r, d_f = sd_r[k] - start[k], sd_f[k] - start[k]
        bad += int(((d_f - d_r).abs() > 1e-3 * 3.1e-3 + 1e-7).sum())
        tot += d_r.numel()
    print(f"\n[accum] {name}: {bad} of {tot} updates outside 1e-3 * lr + 1e-7")
    assert bad <= 1e-3 * tot, (bad, tot)


def test_inf_in_one_micro_batch_skips_the_window_and_the_next_one_recovers(deterministic):
    name = "tiny32_cls"
    g = load_golden(name)
    mbs = _micro_batches(name)
    m = build_model(name, g, "cuda").train()
    opt = trainer.FusedClipAdamWindow(m)
    ema = trainer.ModelEMA(m, 0.9)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    step = trainer.AccumTrainStep(m, opt, scaler=scaler, ema=ema, accumulate=2)
    first = next(iter(m.parameters()))

    def poison(grad):
        grad = grad.clone()
        grad.view(-1)[0] = float("inf")
        return grad

    try:
        before = {k: v.clone() for k, v in m.state_dict().items() if not O.is_buffer(k)}
        shadows = [s.clone() for s in ema.shadows]
        handle = first.register_hook(poison)               # micro-batch 1 of 2
        step(*mbs[0])
        handle.remove()
        step(*mbs[1])
        assert step.boundary and float(opt.stats[1]) == 1.0
        assert opt.step_count == 0 and ema.num_updates == 0 and scaler.get_scale() == 512.0
        assert not bool(torch.isfinite(opt._acc[0]).all())      # the inf stayed in the accumulator
        for k, v in m.state_dict().items():
            if k in before:
                assert torch.equal(v, before[k]), k
        assert all(torch.equal(a, b) for a, b in zip(ema.shadows, shadows))
        for x, y in mbs:                                    # the following window: first = 1 overwrites the sums
            step(x, y)
        assert float(opt.stats[1]) == 0.0 and opt.step_count == 1 and ema.num_updates == 1 and scaler.get_scale() == 512.0
        assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
        assert any(not torch.equal(v, before[k]) for k, v in m.state_dict().items() if k in before)
    finally:
        opt.close()


def test_rccl_world_of_one_with_a_window_is_bit_identical_to_no_reducer(deterministic):
    """The window's exchange on one GPU: the accumulators are the bucket views, reduce_held() all-reduces every flat bucket
    once per window (ReduceOp.AVG inside RCCL) on the side stream; two windows leave exactly the parameters of the
    reducer-less run."""
    import os
    import socket
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{port}", world_size=1, rank=0,
                            device_id=torch.device("cuda", 0))
    try:
        name = "nano48_cls"
        g = load_golden(name)
        mbs = _micro_batches(name)
        results = []
        for use_reducer in (False, True):
            m = build_model(name, g, "cuda").train()
            calm.ops.set_noise_override(W.NoiseStream(11))
            opt = trainer.FusedClipAdamWindow(m)
            red = trainer.HeldGradReducer(m, bucket_mb=1, tail_mb=1, force=True) if use_reducer else None
            step = trainer.AccumTrainStep(m, opt, red, accumulate=2)
            if red is not None:
                assert red.enabled and red.hold and red.avg_in_collective and len(red.buckets) >= 2
                assert [a.data_ptr() for a in opt._acc] == [v.data_ptr() for v in red.views_of(opt.params)]
            try:
                losses = [float(step(x, y)[0]) for _ in range(2) for x, y in mbs]
                assert opt.step_count == 2
            finally:
                opt.close()
                calm.ops.set_noise_override(None)
            torch.cuda.synchronize()
            results.append((losses, {k: v.clone() for k, v in m.state_dict().items()}))
        (l0, sd0), (l1, sd1) = results
        assert l0 == l1, (l0, l1)
        differing = [k for k in sd0 if not torch.equal(sd0[k], sd1[k])]
        assert not differing, differing[:8]
    finally:
        dist.destroy_process_group()
