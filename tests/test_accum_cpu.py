"""Gradient accumulation without a GPU: the float64 checker of calm_grad_accum (tests/accum_f64.py) on an fp32 emulation in
the kernel's order and on planted faults, the window logic of FusedClipAdamWindow on the emulated backend, AccumTrainStep(accumulate=k)
against the hand-written torch loop, train(accumulate=k) with snapshot and exact resume, one all-reduce per bucket per window
on two gloo ranks, what is refused, and the C-ABI addition."""
import os
import re
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import calm_vit_dte_amd as calm  # noqa: E402
import accum_f64 as af  # noqa: E402
from emulated_backend import EmulatedBackend  # noqa: E402
from test_host_logic_cpu import build_model  # noqa: E402
from test_snapshot_cpu import _TinySet, _assert_same_run  # noqa: E402
from importlib import import_module  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
HEADER = os.path.join(ROOT, "include", "calm_vit.h")
TABLE = af.optim_table()


def names(failures):
    return {n for n, _ in failures}


# ---- the checker -----------------------------------------------------------------------------------------------------
def micro_batches():
    """Two micro-batches on one table: the same parameters, but u, v, sigma of the second forward differ from the first's
    (the power iteration advanced), and so do the gradients."""
    recs1 = af.optim_state(TABLE)
    recs2 = af.optim_state(TABLE, seed=1)
    for a, b in zip(recs1, recs2):
        b["param"] = a["param"]
    return recs1, recs2, af.optim_grads(TABLE, recs1, seed=1), af.optim_grads(TABLE, recs2, seed=2)


@pytest.fixture(scope="module")
def case():
    recs1, recs2, g1, g2 = micro_batches()
    nan = [torch.full((e["numel"],), float("nan")) for e in TABLE]
    ref1, bound1 = af.accum_reference(recs1, g1, nan, True)
    acc1 = af.emu_accum(recs1, g1, nan, True)
    ref2, bound2 = af.accum_reference(recs2, g2, acc1, False)
    return dict(recs1=recs1, recs2=recs2, g1=g1, g2=g2, nan=nan, ref1=ref1, bound1=bound1, acc1=acc1, ref2=ref2, bound2=bound2)


def test_emulation_inside_every_bound_over_a_nan_filled_accumulator_and_on_the_second_call(case):
    worst, _ = af.check_accum(case["acc1"], case["ref1"], case["bound1"])
    print(f"accum first=1: {worst}")
    assert all(bool(torch.isfinite(a).all()) for a in case["acc1"])
    acc2 = af.emu_accum(case["recs2"], case["g2"], case["acc1"], False)
    worst, _ = af.check_accum(acc2, case["ref2"], case["bound2"])
    print(f"accum first=0: {worst}")
    for e, a1, a2, g1, g2 in zip(TABLE, case["acc1"], acc2, case["g1"], case["g2"]):
        if e["sn"] is None:
            assert torch.equal(a1, g1) and torch.equal(a2, g1 + g2)


def test_the_table_reaches_what_the_issue_names():
    C = af.OPT_CHUNK
    sizes = {e["numel"] for e in TABLE if e["sn"] is None}
    assert {1, C - 1, C, C + 1, 3 * C + 5} <= sizes
    assert any(e["goff"] for e in TABLE)
    split = [e["sn"] for e in TABLE if e["sn"] and e["numel"] > C and C % e["sn"][1]]
    assert (144, 288) in split and (300, 260) in split
    assert any(e["kind"] == "cancel" for e in TABLE)


@pytest.mark.parametrize("fault", ["first_ignored", "no_inv_sigma", "other_uv", "one_chunk"])
def test_planted_fault_is_caught(case, fault):
    if fault == "first_ignored":
        zeros_then = [torch.ones(e["numel"]) for e in TABLE]          # an old accumulator that is finite: still caught
        got = af.emu_accum(case["recs1"], case["g1"], zeros_then, True, fault)
        ref, bound = case["ref1"], case["bound1"]
    else:
        got = af.emu_accum(case["recs2"], case["g2"], case["acc1"], False, fault, other=case["recs1"])
        ref, bound = case["ref2"], case["bound2"]
    _, failures = af.check_accum(got, ref, bound, strict=False)
    assert "acc" in names(failures), fault


def test_torch_fallback_is_inside_the_bound(case):
    acc = [t.clone() for t in case["nan"]]
    trainer.grad_accum_torch(case["recs1"], case["g1"], acc, True)
    af.check_accum(acc, case["ref1"], case["bound1"])
    first = [t.clone() for t in acc]                                # the second reference starts from the first result
    trainer.grad_accum_torch(case["recs2"], case["g2"], acc, False)
    ref2, bound2 = af.accum_reference(case["recs2"], case["g2"], first, False)
    af.check_accum(acc, ref2, bound2)


# ---- FusedClipAdamWindow -------------------------------------------------------------------------------------------
def _batch(seed=0, B=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 32, 32, generator=g), torch.softmax(torch.randn(B, 10, generator=g), 1)


class _Spy(EmulatedBackend):
    """The emulated backend, recording (plan, divisor) of every optimizer-side step."""

    def __init__(self):
        super().__init__()
        self.steps = []

    def optim_step(self, plan, grads, hp, grad_scale, stats_out, lr_dev=None):
        self.steps.append((plan, None if grad_scale is None else float(grad_scale), [g.data_ptr() for g in grads]))
        return super().optim_step(plan, grads, hp, grad_scale, stats_out, lr_dev=lr_dev)


def _backward(m, seed):
    x, y = _batch(seed)
    trainer.soft_target_cross_entropy(m(x)[0].squeeze(), y).backward()


def test_fused_optimizer_window_counts_divisor_discard_and_shared_step_counter():
    be = _Spy()
    with calm.backend.use_backend(be):
        torch.manual_seed(3)
        m = build_model("tiny32_cls", None).train()
        opt = trainer.FusedClipAdamWindow(m)
        try:
            assert opt.window == 0
            _backward(m, 0)
            opt.step()                                              # window == 0: the single-batch step, as before
            assert be.steps[-1][0] is opt._plan and be.steps[-1][1] is None and opt.step_count == 1
            for k in range(3):
                _backward(m, k)
                assert all(p.grad is not None for p in opt.params)
                opt.accumulate()
                assert opt.window == k + 1 and all(p.grad is None for p in opt.params)
            assert opt._acc_plan.step_dev is opt._plan.step_dev      # one counter
            assert all(a.dtype == torch.float32 and a.shape == p.shape for a, p in zip(opt._acc, opt.params))
            opt.step()
            plan, div, ptrs = be.steps[-1]
            assert plan is opt._acc_plan and div == 3.0 and ptrs == [a.data_ptr() for a in opt._acc]
            assert all(r["sn"] is None for r in plan.records)
            assert opt.window == 0 and opt.step_count == 2
            _backward(m, 5)
            opt.accumulate()
            opt.zero_grad()                                         # discards the window
            assert opt.window == 0 and all(p.grad is None for p in opt.params)
            _backward(m, 6)
            opt.accumulate()
            _backward(m, 7)
            with pytest.raises(RuntimeError, match="window"):       # a gradient outside the open window
                opt.step()
            opt.accumulate()
            opt.step(grad_scale=torch.tensor(8.0))
            assert be.steps[-1][1] == 16.0 and opt.step_count == 3  # grad_scale * window
            _backward(m, 8)
            opt.accumulate()
            opt._acc[0] = opt._acc[0].clone()                        # _check_plan covers the accumulators
            with pytest.raises(RuntimeError, match="moved or replaced"):
                opt.step()
        finally:
            opt.close()


def test_fused_window_equals_the_unfused_window_and_flush_divides_by_the_micro_batches_taken():
    be = _Spy()
    with calm.backend.use_backend(be):
        torch.manual_seed(4)
        m_ref = build_model("tiny32_cls", None).train()
        m = build_model("tiny32_cls", None).train()
        m.load_state_dict(m_ref.state_dict())
        step_ref = trainer.AccumTrainStep(m_ref, trainer.make_optimizer(m_ref), accumulate=3)
        opt = trainer.FusedClipAdamWindow(m)
        step = trainer.AccumTrainStep(m, opt, accumulate=3)
        try:
            assert step.flush() is False                            # an empty window
            for k in range(5):                                      # one whole window, then two of three
                step_ref(*_batch(k))
                step(*_batch(k))
                assert step.boundary == step_ref.boundary == (k == 2)
                assert step.window == opt.window == (k + 1) % 3
            assert be.steps[-1][1] == 3.0 and opt.step_count == 1
            assert step_ref.flush() is True and step.flush() is True
            assert be.steps[-1][1] == 2.0 and opt.step_count == 2 and step.window == opt.window == 0 and step.boundary
            assert step.flush() is False
            sd, sd_ref = m.state_dict(), m_ref.state_dict()
            worst = max(float((sd[k] - sd_ref[k]).abs().max()) for k in sd)
            assert worst < 2e-5, worst                              # (the bar of the single-batch comparison)
        finally:
            opt.close()


def test_unfused_window_equals_the_hand_written_torch_loop_bit_for_bit():
    with calm.backend.use_backend(EmulatedBackend()):
        torch.manual_seed(5)
        m_ref = build_model("tiny32_cls", None).train()
        m = build_model("tiny32_cls", None).train()
        m.load_state_dict(m_ref.state_dict())
        opt_ref = trainer.make_optimizer(m_ref)
        params = [p for p in m_ref.parameters() if p.requires_grad]
        ema = trainer.ModelEMA(m, 0.9)
        step = trainer.AccumTrainStep(m, trainer.make_optimizer(m), accumulate=2, ema=ema)
        for w in range(2):
            for k in range(2):
                x, y = _batch(2 * w + k)
                torch.nn.functional.cross_entropy(m_ref(x)[0].squeeze(), y).backward()      # autograd sums into .grad
                step(x, y)
                assert step.boundary == (k == 1)
            torch._foreach_mul_([p.grad for p in params], 0.5)
            torch.nn.utils.clip_grad_norm_(params, max_norm=1.0)
            opt_ref.step()
            opt_ref.zero_grad()
        sd, sd_ref = m.state_dict(), m_ref.state_dict()
        assert all(torch.equal(sd[k], sd_ref[k]) for k in sd)
        assert ema.num_updates == 2                                 # one update per optimizer step


@pytest.mark.parametrize("config", ["plain", "ema", "ema_scaler"])
def test_a_window_of_one_is_the_single_batch_step_bit_for_bit(config):
    """AccumTrainStep(accumulate=1) against TrainStep, torch AdamW: parameters, optimizer state and EMA shadows after every
    step.  The window class runs TrainStep's own optimizer-side sequence (m = 1: no 1/m pass), not a copy of it."""
    assert "_optimizer_step" not in vars(trainer.AccumTrainStep)
    with calm.backend.use_backend(EmulatedBackend()):
        runs = []
        for cls, kw in ((trainer.TrainStep, {}), (trainer.AccumTrainStep, {"accumulate": 1})):
            torch.manual_seed(9)
            m = build_model("tiny32_cls", None).train()
            opt = trainer.make_optimizer(m)
            ema = trainer.ModelEMA(m, 0.9) if config != "plain" else None
            scaler = torch.amp.GradScaler("cpu", init_scale=4.0, growth_interval=2) if config == "ema_scaler" else None
            runs.append((m, opt, ema, cls(m, opt, ema=ema, scaler=scaler, **kw)))
        (m_a, opt_a, ema_a, step_a), (m_b, opt_b, ema_b, step_b) = runs
        assert (step_b._ema_one is not None) == (config == "ema_scaler") and step_b._clean_steps is None
        for k in range(3):
            loss_a, _ = step_a(*_batch(k))
            loss_b, _ = step_b(*_batch(k))
            assert step_b.boundary and step_b.window == 0 and torch.equal(loss_a, loss_b)
            sd_a, sd_b = m_a.state_dict(), m_b.state_dict()
            assert all(torch.equal(sd_a[n], sd_b[n]) for n in sd_a), k
            st_a, st_b = opt_a.state_dict()["state"], opt_b.state_dict()["state"]
            assert len(st_a) == len(st_b) > 0
            for i in st_a:
                assert all(torch.equal(torch.as_tensor(st_a[i][n]), torch.as_tensor(st_b[i][n])) for n in st_a[i]), (k, i)
            if ema_a is not None:
                assert ema_a.num_updates == ema_b.num_updates == k + 1
                assert all(torch.equal(a, b) for a, b in zip(ema_a.shadows, ema_b.shadows)), k


def test_generative_step_steps_only_at_the_boundary():
    """AccumRegTrainStep: RegTrainStep's forward and loss, AccumTrainStep's window."""
    with calm.backend.use_backend(EmulatedBackend()):
        torch.manual_seed(8)
        m = build_model("nano48_gen", None).train()
        step = trainer.AccumRegTrainStep(m, trainer.make_optimizer(m), accumulate=2, kl_weight=0.2)
        assert step.kl_weight == 0.2
        x = torch.randn(2, 3, 48, 48)
        before = [p.detach().clone() for p in step.params]
        step(x)
        assert not step.boundary and step.window == 1
        assert all(torch.equal(p, b) for p, b in zip(step.params, before))
        step(x)
        assert step.boundary and step.window == 0
        assert any(not torch.equal(p, b) for p, b in zip(step.params, before))


def test_save_async_inside_a_window_refuses(tmp_path):
    with calm.backend.use_backend(EmulatedBackend()):
        torch.manual_seed(6)
        m = build_model("tiny32_cls", None).train()
        for kind in ("adamw", "fused"):
            opt = trainer.FusedClipAdamWindow(m) if kind == "fused" else trainer.make_optimizer(m)
            try:
                step = trainer.AccumTrainStep(m, opt, accumulate=2)
                st = trainer.TrainState(m, opt, step=step)
                path = str(tmp_path / f"{kind}.snap")
                step(*_batch(0))
                with pytest.raises(RuntimeError, match="window"):
                    st.save_async(path, {"epoch": 0, "batch": 1, "step": 0})
                step(*_batch(1))
                st.save_async(path, {"epoch": 0, "batch": 2, "step": 1})
                st.wait()
                assert trainer.TrainState.read_header(path)[0]["host"]["progress"]["step"] == 1
                st.close()
            finally:
                if kind == "fused":
                    opt.close()


# ---- train(accumulate=2) ---------------------------------------------------------------------------------------------------
def _run(optimizer_kind, seed=50, epochs=2, **kw):
    """train() with 5 batches of 4 per epoch and windows of 2: optimizer steps behind batches 2, 4 and (flushed) 5."""
    torch.manual_seed(seed)
    m = build_model("tiny32_cls", None).train()
    with calm.backend.use_backend(EmulatedBackend()):
        opt = "fused" if optimizer_kind == "fused" else trainer.make_optimizer(m)
        out = trainer.train(m, opt, None, use_gpu=False, dataset=_TinySet(20), epochs=epochs, batch_size=4, num_classes=10,
                            collate_fn="mix", num_workers=0, log_every=1000, ema=0.99, accumulate=2, **kw)
    return out, opt


def _progress(path):
    return trainer.TrainState.read_header(path)[0]["host"]["progress"]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("optimizer_kind", ["adamw", "fused"])
def test_train_counts_optimizer_steps_and_resumes_exactly_at_a_boundary(tmp_path, optimizer_kind):
    fa, fb, fc, fd = (str(tmp_path / f"{n}.snap") for n in "abcd")
    a, opt_a = _run(optimizer_kind, snapshot_path=fa)
    assert _progress(fa) == {"epoch": 2, "batch": 0, "step": 6}          # 3 optimizer steps per epoch of 5 batches
    assert a._calm_ema.num_updates == 6                                  # the last of each epoch from one micro-batch
    if optimizer_kind == "adamw":
        assert all(int(s["step"]) == 6 for s in opt_a.state_dict()["state"].values())
    _run(optimizer_kind, snapshot_path=fb, max_steps=2)                  # max_steps counts optimizer steps
    assert _progress(fb) == {"epoch": 0, "batch": 4, "step": 2}
    c, _ = _run(optimizer_kind, seed=51, snapshot_path=fc, resume=fb)
    _assert_same_run(a, c, fa, fc)
    for sa, sc in zip(a._calm_ema.shadows, c._calm_ema.shadows):
        assert torch.equal(sa, sc)
    _run(optimizer_kind, snapshot_path=fd, snapshot_every=1, max_steps=3)    # the third step is the flushed one
    assert _progress(fd) == {"epoch": 1, "batch": 0, "step": 3}


# ---- two gloo ranks ----------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _two_rank_worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    real = dist.all_reduce

    def counted(tensor, *a, **kw):
        calls.append(tensor.numel())
        return real(tensor, *a, **kw)

    dist.all_reduce = counted
    out = {}
    try:
        with calm.backend.use_backend(EmulatedBackend()):
            for kind in ("adamw", "fused"):
                torch.manual_seed(60)
                m = build_model("tiny32_cls", None).train()
                opt = trainer.FusedClipAdamWindow(m) if kind == "fused" else trainer.make_optimizer(m)
                red = trainer.HeldGradReducer(m, bucket_mb=0, tail_mb=0)      # one bucket per parameter but the last two
                step = trainer.AccumTrainStep(m, opt, red, accumulate=2)
                assert red.hold and len(red.buckets) > 4
                if kind == "fused":
                    assert [a.data_ptr() for a in opt._acc] == [v.data_ptr() for v in red.views_of(opt.params)]
                per_window = []
                for k in range(5):
                    before = len(calls)
                    step(*_batch(10 * rank + k))
                    per_window.append(len(calls) - before)
                before = len(calls)
                assert step.flush()
                per_window.append(len(calls) - before)
                n = len(red.buckets)
                assert per_window == [0, n, 0, n, 0, n], (kind, per_window, n)
                out[kind] = {k: v.clone() for k, v in m.state_dict().items()}
                if kind == "fused":
                    opt.close()
    finally:
        dist.all_reduce = real
    torch.save(out, os.path.join(outdir, f"rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_one_all_reduce_per_bucket_per_window_on_two_gloo_ranks(tmp_path):
    mp.spawn(_two_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(2))
    for kind in ("adamw", "fused"):
        for k in r0[kind]:
            assert torch.equal(r0[kind][k], r1[kind][k]), f"{kind}: ranks diverged at {k}"
    worst = max(float((r0["fused"][k] - r0["adamw"][k]).abs().max()) for k in r0["fused"])
    assert worst < 2e-5, worst                                      # the two paths mean the same thing


# ---- refusals and the ABI ----------------------------------------------------------------------------------------------------
def test_argument_refusals_come_before_any_process_group():
    data = torch.utils.data.TensorDataset(torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,)))
    lin = torch.nn.Linear(4, 4)
    sgd = torch.optim.SGD(lin.parameters(), lr=0.1)
    for kw in (dict(accumulate=0), dict(accumulate=-2), dict(accumulate=1.5),
               dict(accumulate=2, graph=True, use_gpu=True, optimizer="fused")):
        kw = dict(dict(use_gpu=False, optimizer=sgd), **kw)
        with pytest.raises(ValueError, match="accumulate"):
            trainer.train(lin, kw.pop("optimizer"), dataset=data, epochs=1, batch_size=2, num_classes=10, **kw)
    assert not torch.distributed.is_initialized()
    for k in (0, -1, 2.5):
        with pytest.raises(ValueError, match="accumulate"):
            trainer.AccumTrainStep(lin, sgd, accumulate=k)
        with pytest.raises(ValueError, match="accumulate"):
            trainer.AccumRegTrainStep(lin, sgd, accumulate=k)
    with calm.backend.use_backend(EmulatedBackend()):
        m = build_model("tiny32_cls", None).train()
        plain = trainer.FusedClipAdamW(m)                           # corrects once per step: it has no window
        try:
            with pytest.raises(TypeError, match="FusedClipAdamWindow"):
                trainer.AccumTrainStep(m, plain, accumulate=2)
            with pytest.raises(ValueError, match="accumulate"):
                trainer.train(m, plain, use_gpu=False, dataset=data, epochs=1, batch_size=2, num_classes=10, accumulate=2)
        finally:
            plain.close()
    assert not torch.distributed.is_initialized()


def test_calm_grad_accum_is_exported_bound_and_refuses_bad_arguments_before_any_launch():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"^\s*int\s+calm_grad_accum\s*\(", text, flags=re.M)
    assert int(re.search(r"#define\s+CALM_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == binding.ABI_VERSION == 7
    lib = binding.load()
    assert hasattr(lib, "calm_grad_accum") and "calm_grad_accum" in binding.SIGNATURES
    assert lib.calm_abi_version() == 7
    P = 0x7f0000010000
    valid = [P, 3, P, 5, P, P, 1, None]                             # never passed as it is: nothing is launched
    for i in (0, 2, 4, 5):
        args = list(valid)
        args[i] = None
        assert lib.calm_grad_accum(*args) == binding.E_INVAL, i
    for i, v in ((1, 0), (1, -1), (3, 0), (3, -4), (6, 2), (6, -1)):
        args = list(valid)
        args[i] = v
        assert lib.calm_grad_accum(*args) == binding.E_INVAL, (i, v)
