"""calm_sam_perturb / calm_sam_restore of libcalmvit_hip.so against the float64 checker (tests/sam_f64.py) on
tail_f64.optim_table() — the smallest table at which the chunk walk, the deferred correction with its cancelling tensor,
the row-split chunks and the two access paths can each go wrong — once where tail_f64's arenas put the tensors and once with
every tensor 16-byte aligned; then SamTrainStep on tiny32_cls against a hand-written loop over backend.sam_perturb /
backend.sam_restore, and train(sam=).  tests/test_sam_cpu.py proves the checker on an fp32 emulation and on planted faults.
Outputs, backups and scratch sit between NaN-pattern guards; every input arena must come back bit for bit.  The inf / NaN
of the non-finite cases are values planted in input data."""
import functools
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import sam_f64 as sf
import tail_f64 as tf
import weights as W
from helpers import CONFIGS, load_golden
from test_grad_stats_gpu import StatsDevice
from test_host_logic_cpu import build_model
from test_rowwise_f64_gpu import Out, place
from test_tail_f64_gpu import Arena, show
from test_trainer_gpu import _batch

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
TABLE = tf.optim_table()
N = len(TABLE)
NAME = "tiny32_cls"
RHO, EPS, ETA = 0.05, 1e-12, 0.01
SCENARIOS = {"plain": (None, 0), "scaled": (1024.0, 0), "adaptive": (None, 1), "adaptive_scaled": (1024.0, 1)}
CASES = {c[0]: c for c in tf.optim_nonfinite_cases(TABLE)}
RUNS = [(s, None) for s in SCENARIOS] + [(s, c) for s in ("plain", "adaptive_scaled") for c in CASES]


@pytest.fixture(scope="module")
def hip():
    return calm.backend.get_backend()


@functools.lru_cache(maxsize=None)
def _inputs(scenario, case):
    """(recs, grads, hp, scale, ref, bound) of a run, computed once and shared by both placements"""
    scale, adaptive = SCENARIOS[scenario]
    recs = tf.optim_state(TABLE)
    grads = tf.optim_grads(TABLE, recs, seed=1, scale=scale or 1.0)
    if case is not None:
        _, tensor, element, value = CASES[case]
        grads[tensor][element] = value
    hp = (RHO, EPS, ETA, adaptive)
    return (recs, grads, hp, scale) + sf.reference(recs, grads, hp, scale)


class SamDevice(StatsDevice):
    """tail_f64's device state (aligned: every tensor on a multiple of 16 bytes) with the buffers of the two entry points:
    the backups in a guarded arena laid out like the parameters', scratch and stats_out between guards."""

    def __init__(self, hip, recs, aligned=False):
        super().__init__(hip, TABLE, recs, aligned=aligned)
        self.b = Arena([torch.full_like(r["param"], -7.0) for r in recs], self.goff if aligned else None)
        self.ptrs = torch.tensor([v.data_ptr() for v in self.b.views], dtype=torch.int64, device="cuda")
        self.sam_scratch = Out((hip.sam_scratch_floats(self.plan),))
        assert self.sam_scratch.t.numel() == 3 * self.plan.n_chunks + N + 4
        self.sam_stats = Out((3,))

    def pair(self, grads, hp, scale):
        """one perturb / restore pair -> what sam_f64.check takes; every guard and every input is compared on the way"""
        G = Arena(grads, self.goff)
        self.paths = [all(t.data_ptr() % 16 == 0 for t in q) for q in zip(G.views, self.p.views, self.b.views)]
        inputs = self.state_bits()[1:]                       # moments, u / v / sigma
        gs = place(torch.tensor([scale])) if scale else None
        self.hip.sam_perturb(self.plan, G.views, hp, gs, self.ptrs, self.sam_scratch.t, self.sam_stats.t)
        st = self.sam_stats.check()
        self.sam_scratch.check(written=False)
        got = dict(norm=float(st[0]), found_inf=float(st[1]), scale=float(st[2]), p_after=self.p.read(), backup=self.b.read())
        self.hip.sam_restore(self.plan, self.ptrs)
        got["p_restored"] = self.p.read()
        assert torch.equal(G.read().view(torch.int32), G.before[~G.gap]), "the calls changed a gradient"
        assert torch.equal(self.b.read().view(torch.int32), got["backup"].view(torch.int32)), "the restore changed a backup"
        assert all(torch.equal(a, b) for a, b in zip(inputs, self.state_bits()[1:])), "the calls changed a moment or u / v / sigma"
        assert torch.equal(self.p.buf.cpu().view(torch.int32), self.p.before), "the parameter arena after the restore"
        return got


@pytest.mark.parametrize("aligned", [False, True], ids=["tail-layout", "aligned16"])
@pytest.mark.parametrize("scenario,case", RUNS, ids=[s + ("-" + c if c else "") for s, c in RUNS])
def test_perturb_and_restore_inside_every_bound(hip, scenario, case, aligned):
    recs, grads, hp, scale, ref, bound = _inputs(scenario, case)
    dev = SamDevice(hip, recs, aligned=aligned)
    got = dev.pair(grads, hp, scale)
    if aligned:
        assert all(dev.paths)
    else:                                                    # some tensors on each path where tail_f64 puts them
        assert any(dev.paths) and not all(dev.paths)
    worst, failures = sf.check(got, ref, bound, strict=False)
    show(f"sam {scenario} {case or ''} {'aligned' if aligned else 'tail layout'}", worst)
    assert not failures, failures
    assert ref["found_inf"] == (0.0 if case is None else 1.0)


@pytest.mark.parametrize("aligned", [False, True], ids=["tail-layout", "aligned16"])
def test_two_calls_and_another_stream_give_identical_bits(hip, aligned):
    recs, grads, hp, scale, ref, bound = _inputs("adaptive_scaled", None)
    dev = SamDevice(hip, recs, aligned=aligned)
    a = dev.pair(grads, hp, scale)
    b = dev.pair(grads, hp, scale)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        c = dev.pair(grads, hp, scale)
    side.synchronize()
    for other in (b, c):
        assert (a["norm"], a["scale"], a["found_inf"]) == (other["norm"], other["scale"], other["found_inf"])
        for k in ("p_after", "backup", "p_restored"):
            assert torch.equal(a[k].view(torch.int32), other[k].view(torch.int32)), k
    assert a["scale"] > 0 and not torch.equal(a["p_after"], a["backup"])


# ---- model level ---------------------------------------------------------------------------------------------------------
def _scale_update(scaler, scale, bad, clean):
    """TrainStep's GradScaler bookkeeping behind a fused step -> the new count of clean steps"""
    clean = 0 if bad else clean + 1
    grow = clean >= scaler.get_growth_interval()
    scaler.update(scale * (scaler.get_backoff_factor() if bad else scaler.get_growth_factor() if grow else 1.0))
    return 0 if grow else clean


def _three_steps(hip, hand, autocast):
    """Three SAM steps of tiny32_cls with a GradScaler and an EMA: SamTrainStep, or the same from public pieces —
    forward, backward, backend.sam_perturb, release, forward, backward, accumulate, backend.sam_restore, step."""
    _, x, y = _batch(NAME, bs=8)
    xs, y = [x.cuda(), x.cuda().flip(0)], y.cuda()
    m = build_model(NAME, load_golden(NAME), "cuda").train()
    opt = trainer.FusedClipAdamWindow(m)
    ema = trainer.ModelEMA(m, 0.9)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    dtype = torch.bfloat16 if autocast else None
    trace, clean = [], 0
    try:
        if hand:
            backups = [torch.empty_like(p) for p in opt.params]
            ptrs = torch.tensor([b.data_ptr() for b in backups], dtype=torch.int64, device="cuda")
            scratch = torch.empty(hip.sam_scratch_floats(opt._plan), device="cuda")
            stats, one = torch.zeros(3, device="cuda"), torch.ones((), device="cuda")

            def backward(x):
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    loss = trainer.soft_target_cross_entropy(m(x)[0].squeeze(), y)
                with calm.ops.grad_tail(opt.params, enabled=True):
                    scaler.scale(loss).backward()
                return loss.detach()
        else:
            sam = trainer.SharpnessAware(m, opt, rho=RHO)
            assert sam.native
            step = trainer.SamTrainStep(m, opt, sam=sam, scaler=scaler, autocast_dtype=dtype, ema=ema)
        for k in range(3):
            calm.ops.set_noise_override(W.NoiseStream(70 + k))
            if hand:
                loss = backward(xs[k % 2])
                scale = scaler.scale(one)
                hip.sam_perturb(opt._plan, opt._contiguous_grads(keep=False), (RHO, EPS, ETA, 0), scale, ptrs, scratch, stats)
                for p in opt.params:
                    p.grad = None
                backward(xs[k % 2])
                opt.accumulate()
                hip.sam_restore(opt._plan, ptrs)
                st = opt.step(grad_scale=scale)
                ema.update(skip=st[1:2])
                clean = _scale_update(scaler, scale, bool(st[1] > 0), clean)
            else:
                loss, _ = step(xs[k % 2], y)
            torch.cuda.synchronize()
            bits = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).view(torch.int32).cpu()      # noqa: E731
            trace.append((loss.cpu(), bits(opt.params), bits(opt.exp_avg), bits(ema.shadows), float(scaler.get_scale()),
                          float(opt.stats[1])))
        assert opt.step_count == 3 - sum(t[5] for t in trace)
    finally:
        calm.ops.set_noise_override(None)
        opt.close()
    return trace


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast-bf16"])
def test_sam_train_step_equals_the_hand_written_loop_bit_for_bit(hip, autocast):
    prev = hip.gemm_set_option(hip.GEMM_OPT_DETERMINISTIC, 1)
    try:
        a = _three_steps(hip, False, autocast)
        b = _three_steps(hip, True, autocast)
    finally:
        hip.gemm_set_option(hip.GEMM_OPT_DETERMINISTIC, prev)
    for k, (s, h) in enumerate(zip(a, b)):
        assert torch.equal(s[0], h[0]), f"step {k}: the loss is not the first pass's"
        assert all(torch.equal(s[i], h[i]) for i in (1, 2, 3)), f"step {k}: parameters, moments or the EMA differ"
        assert s[4:] == h[4:], f"step {k}: scale / found_inf"
    assert any(t[5] == 0.0 for t in a) and not torch.equal(a[0][1], a[2][1])      # at least one step was applied


def test_train_with_sam_a_monitor_and_the_device_collate(tmp_path):
    cfg = CONFIGS[NAME]
    S = cfg.seq_length
    gen = torch.Generator().manual_seed(0)
    data = torch.utils.data.TensorDataset(torch.randint(0, 256, (16, 3, S + 4, S + 4), generator=gen, dtype=torch.uint8),
                                          torch.randint(0, cfg.out_features, (16,), generator=gen))
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    m = build_model(NAME, load_golden(NAME), "cpu")
    out = trainer.train(m, "fused", scheduler=None, use_gpu=True, dataset=data, epochs=1, batch_size=4,
                        num_classes=cfg.out_features, device_collate=True, crop=(S, S), log_every=1000, max_steps=3,
                        sam=0.05, monitor=True)
    assert all(bool(torch.isfinite(p).all()) for p in out.parameters())
    sam, mon = out._calm_sam, out._calm_monitor
    assert isinstance(sam, trainer.SharpnessAware) and sam.native and isinstance(sam.optimizer, trainer.FusedClipAdamWindow)
    rep, first = mon.read(), sam.read()
    assert rep["calls"] == 3                                 # one observed gradient per step: the second pass's
    stats = sam.optimizer.stats.cpu()
    if float(stats[1]) == 0.0 and first["found_inf"] == 0.0:
        # the monitor's norm and the step's own are fp32 sums of depth < 200 over the same (second-pass) gradient: each
        # within 200 U = 1.2e-5 of it; the first pass's norm, at other weights, is a different number
        assert abs(rep["norm"] - float(stats[0])) <= 1e-4 * float(stats[0])
        assert first["norm"] > 0 and first["norm"] != rep["norm"] and np.isclose(first["scale"] * first["norm"], 0.05, rtol=1e-5)
    else:
        assert rep["skipped"] > 0 or first["found_inf"] == 1.0
