"""Knowledge distillation without a GPU: the two C-ABI additions are declared, exported and bound and refuse bad arguments
before any launch; the float64 checker (tests/distill_f64.py) passes the torch emulation of the entry points
(tests/emulated_distill.py) and rejects each of its planted faults; ops.DistillLossFn against autograd through
trainer.distill_loss_torch; train(teacher=...) against a hand-written loop on one and on two gloo ranks, with accumulation,
snapshot and exact resume; what is refused."""
import math
import os
import re
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import calm_vit_dte_amd as calm  # noqa: E402
import distill_f64 as D  # noqa: E402
from emulated_infer import EmulatedInferBackend as EmulatedBackend  # noqa: E402  (the teacher runs the lean forward)
from emulated_distill import DEFECTS, ROW_STATS, EmulatedDistillBackend  # noqa: E402
from emulated_loss import EmulatedLossBackend  # noqa: E402
from helpers import rel_err  # noqa: E402
from test_host_logic_cpu import build_model  # noqa: E402
from test_snapshot_cpu import _TinySet, _assert_same_run  # noqa: E402
from importlib import import_module  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
HEADER = os.path.join(ROOT, "include", "calm_vit.h")
TOL = 1e-5                                     # formulas, not hardware (TOL of tests/test_loss_cpu.py)


@pytest.fixture(autouse=True)
def _restore_switch():
    prev = calm.backend.get_loss_kernels()
    yield
    calm.backend.set_loss_kernels(prev)


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_bound_and_sized():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(calm_\w+)\s*\(", text, flags=re.M))
    lib = binding.load()
    for n in ("calm_distill_fwd", "calm_distill_bwd"):
        assert n in declared and n in binding.SIGNATURES and hasattr(lib, n), n
    assert int(re.search(r"#define\s+CALM_ABI_VERSION\s+(\d+)", raw).group(1)) == binding.ABI_VERSION == lib.calm_abi_version() == 7
    assert re.search(r"CALM_RED_DISTILL\s*=\s*9\b", text) and binding.RED_DISTILL == 9
    assert int(re.search(r"#define\s+CALM_DISTILL_ROW_STATS\s+(\d+)", raw).group(1)) == binding.DISTILL_ROW_STATS == ROW_STATS
    assert re.search(r"CALM_DISTILL_SOFT\s*=\s*0\b", text) and re.search(r"CALM_DISTILL_HARD\s*=\s*1\b", text)
    assert (binding.DISTILL_SOFT, binding.DISTILL_HARD) == (0, 1)
    for B, C in D.CASES:
        assert int(lib.calm_reduce_scratch_floats(binding.RED_DISTILL, B, C)) == 5 * B
    assert int(lib.calm_reduce_scratch_floats(99, 10, 10)) == 0


P = 0x7f0000010000                             # never dereferenced: every call below is refused before any launch


def _fwd_args(**kw):
    a = dict(logits=P, ld=10, teacher=P, tld=10, teacher_type=binding.ST_F32, targets=P, td=10, temperature=1.0, alpha=0.5,
             mode=0, row_stats=P, loss=P, metrics=None, dmetrics=None, B=3, C=10, partials=P, stream=None)
    a.update(kw)
    return list(a.values())


def _bwd_args(**kw):
    a = dict(logits=P, ld=10, teacher=P, tld=10, teacher_type=binding.ST_F32, targets=P, td=10, temperature=1.0, alpha=0.5,
             mode=0, row_stats=P, dloss=P, dlogits=P, B=3, C=10, stream=None)
    a.update(kw)
    return list(a.values())


SHARED_REFUSALS = [dict(logits=None), dict(teacher=None), dict(targets=None), dict(row_stats=None), dict(B=0), dict(B=-1),
                   dict(C=0), dict(C=-3), dict(ld=9), dict(tld=9), dict(td=9), dict(temperature=0.0), dict(temperature=-1.0),
                   dict(temperature=math.inf), dict(temperature=math.nan), dict(alpha=-0.01), dict(alpha=1.01),
                   dict(alpha=math.nan), dict(mode=2), dict(mode=-1), dict(teacher_type=binding.ST_FP8_E4M3),
                   dict(teacher_type=7)]


def test_every_refusal_is_returned_without_a_gpu():
    lib = binding.load()
    for kw in SHARED_REFUSALS + [dict(loss=None), dict(partials=None)]:
        assert lib.calm_distill_fwd(*_fwd_args(**kw)) == binding.E_INVAL, kw
    for kw in SHARED_REFUSALS + [dict(dloss=None), dict(dlogits=None)]:
        assert lib.calm_distill_bwd(*_bwd_args(**kw)) == binding.E_INVAL, kw
    big = dict(C=65537, ld=65537, tld=65537, td=65537)
    assert lib.calm_distill_fwd(*_fwd_args(**big)) == binding.E_UNSUPP
    assert lib.calm_distill_bwd(*_bwd_args(**big)) == binding.E_UNSUPP
    assert lib.calm_distill_fwd(*_fwd_args(partials=P + 4)) == binding.E_LAYOUT
    # the emulation refuses the same way
    be = EmulatedDistillBackend()
    z, t, y = D.inputs(3, 10)
    rs, loss = torch.empty(3, ROW_STATS), torch.empty(())
    for kw in (dict(temperature=0.0), dict(temperature=math.inf), dict(alpha=1.5), dict(alpha=math.nan), dict(mode="both")):
        a = dict(dict(temperature=1.0, alpha=0.5, mode="soft"), **kw)
        with pytest.raises(RuntimeError, match="code -1"):
            be.distill_fwd(z, t, y, a["temperature"], a["alpha"], a["mode"], rs, loss, None, None, 3, 10)
    with pytest.raises(RuntimeError, match="code -1"):
        be.distill_fwd(z, t.to(torch.float16), y, 1.0, 0.5, "soft", rs, loss, None, None, 3, 10)


# ---- the checker on the emulation and on its planted faults -------------------------------------------------------------------
def _emulate(be, z, t, y, T, alpha, mode, dloss=3.0, metrics=None, dmetrics=None):
    B, C = z.shape
    rs, loss, dz = torch.empty(B, ROW_STATS), torch.empty(()), torch.empty(B, C)
    be.distill_fwd(z, t, y, T, alpha, mode, rs, loss, metrics, dmetrics, B, C)
    be.distill_bwd(z, t, y, T, alpha, mode, rs, torch.tensor([dloss]), dz, B, C)
    return loss, dz, rs


def _tie_case():
    """Teacher rows whose maximum appears twice: hard mode has to pick the lowest index."""
    z, t, y = D.inputs(3, 10, seed=5)
    t[0, 2] = t[0, 7] = 9.0
    t[1, 0] = t[1, 9] = 9.0
    return z, t, y


TIE = (3, 10, 1.0, 0.5, "hard", 1.0, "tie")
_REF_CACHE = {}


def _variant_inputs(v):
    """(z, t, y, float64 reference at dloss = 3) of one variant, computed once and shared."""
    if v not in _REF_CACHE:
        B, C, T, alpha, mode, scale, tdt = v
        z, t, y = _tie_case() if tdt == "tie" else D.inputs(B, C, scale, teacher=tdt)
        _REF_CACHE[v] = (z, t, y, D.reference(z, t, y, T, alpha, mode, 3.0))
    return _REF_CACHE[v]


@pytest.mark.parametrize("v", D.VARIANTS + [TIE], ids=lambda v: "-".join(str(x) for x in v))
def test_checker_passes_the_clean_emulation(v):
    z, t, y, ref = _variant_inputs(v)
    loss, dz, rs = _emulate(EmulatedDistillBackend(), z, t, y, v[2], v[3], v[4])
    figures, _ = D.check(loss, dz, rs, ref, label=str(v))
    print(f"\n{v}: {figures}")


@pytest.mark.parametrize("defect", DEFECTS)
def test_checker_rejects_every_planted_defect_on_at_least_one_case(defect):
    caught = []
    for v in D.VARIANTS + [TIE]:
        if v[1] > 1001 and defect != "tail_skipped":           # (the long rows add nothing to what the short ones catch)
            continue
        z, t, y, ref = _variant_inputs(v)
        loss, dz, rs = _emulate(EmulatedDistillBackend(defect), z, t, y, v[2], v[3], v[4])
        _, failures = D.check(loss, dz, rs, ref, strict=False)
        if failures:
            caught.append((v, [f[0] for f in failures]))
    print(f"\n{defect}: caught on {len(caught)} cases, e.g. {caught[:2]}")
    assert caught, defect
    names = {n for _, fs in caught for n in fs}
    if defect in ("no_t2", "kl_swapped", "alpha_on_ce", "tail_skipped", "rows_from_256_dropped"):
        assert "loss" in names and "dlogits" in names, (defect, names)     # both directions carry the fault
    if defect == "t2_in_grad":
        assert names == {"dlogits"}
    if defect == "tie_highest":
        assert "argmax t" in names and all(v is TIE for v, _ in caught)


def test_counts_and_sums_of_the_emulation_equal_the_reference():
    be = EmulatedDistillBackend()
    m, dm = trainer.StepMetrics(torch.device("cpu")), trainer.DistillMetrics(torch.device("cpu"))
    assert dm.read() == (0.0, 0.0, 0, 0)
    want = dict(row_sum=0.0, ce_sum=0.0, d_sum=0.0, agree_y=0, agree_t=0)
    for seed in range(2):
        z, t, y = D.inputs(37, 10, seed=seed)
        y[0] = 0.0
        y[0, int(z[0].argmax())] = 1.0                              # (at least one row agrees with the labels)
        t[1] = z[1]                                                 # (and one with the teacher)
        ref = D.reference(z, t, y, 2.0, 0.3, "soft")
        _emulate(be, z, t, y, 2.0, 0.3, "soft", metrics=m.buf, dmetrics=dm.buf)
        for k in want:
            want[k] += float(ref[k])
    loss_sum, agree, rows, steps = m.read()
    ce_sum, d_sum, agree_t, rows_t = dm.read()
    assert (agree, rows, steps, agree_t, rows_t) == (want["agree_y"], 74, 2, want["agree_t"], 74)
    assert agree >= 2 and agree_t >= 2 and isinstance(agree_t, int) and isinstance(rows_t, int)
    for got, k in ((loss_sum, "row_sum"), (ce_sum, "ce_sum"), (d_sum, "d_sum")):
        assert abs(got - want[k]) <= 1e-5 * abs(want[k]), k
    dm.reset()
    assert dm.read() == (0.0, 0.0, 0, 0)
    # a NaN on either side: no agreement, and the loss is NaN in both modes
    z, t, y = D.inputs(2, 10)
    t[0] = z[0]
    t[1] = z[1]
    t[1, 3] = float("nan")
    for mode in ("soft", "hard"):
        dm.reset()
        loss, dz, _ = _emulate(be, z, t, y, 1.0, 0.5, mode, dmetrics=dm.buf)
        assert math.isnan(float(loss)) and dm.read()[2:] == (1, 2)
        assert bool(torch.isfinite(dz[0]).all()) and not bool(torch.isfinite(dz[1]).any())      # GradScaler skips the step


# ---- ops.DistillLossFn and trainer.distillation_loss ----------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,T,alpha,mode,scale,tdt", [(4, 1000, 2.0, 0.5, "soft", 1.0, "f32"), (5, 1001, 4.0, 0.3, "soft", 4.0, "f32"),
                                                       (3, 10, 1.0, 1.0, "soft", 1.0, "bf16"), (5, 1001, 1.0, 0.7, "hard", 1.0, "f32"),
                                                       (257, 10, 0.5, 0.5, "soft", 1.0, "f32"), (3, 10, 1.0, 0.0, "hard", 1.0, "bf16")])
def test_function_matches_autograd_through_the_torch_loss(B, C, T, alpha, mode, scale, tdt):
    z, t, y = D.inputs(B, C, scale, teacher=tdt)
    z64 = z.double().requires_grad_(True)
    ref = trainer.distill_loss_torch(z64, t.double(), y.double(), alpha, T, mode)
    (ref * 512.0).backward()
    zl = z.clone().requires_grad_(True)
    with calm.backend.use_backend(EmulatedDistillBackend()):
        loss = calm.ops.DistillLossFn.apply(zl, t, y, T, alpha, mode)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        (loss * 512.0).backward()
    assert rel_err(loss.detach(), ref.detach()) <= TOL
    assert rel_err(zl.grad, z64.grad) <= TOL
    # the literal formula of the issue
    if mode == "soft":
        lit = (1 - alpha) * F.cross_entropy(z64, y.double()) + alpha * T * T * F.kl_div(
            F.log_softmax(z64 / T, 1), F.softmax(t.double() / T, 1), reduction="batchmean")
    else:
        lit = (1 - alpha) * F.cross_entropy(z64, y.double()) + alpha * F.cross_entropy(z64, t.double().argmax(1))
    assert torch.equal(lit.detach(), ref.detach())


def test_alpha_zero_is_the_soft_target_cross_entropy():
    z, t, y = D.inputs(37, 1001, 2.0)
    be, ce = EmulatedDistillBackend(), EmulatedLossBackend()
    for mode in ("soft", "hard"):
        loss, dz, rs = _emulate(be, z, t, y, 2.0, 0.0, mode, dloss=3.0)
        rs2, loss2, dz2 = torch.empty(37, 2), torch.empty(()), torch.empty(37, 1001)
        ce.soft_ce_fwd(z, y, rs2, loss2, None, 37, 1001)
        ce.soft_ce_bwd(z, y, rs2, torch.tensor([3.0]), dz2, 37, 1001)
        assert torch.equal(loss, loss2) and torch.equal(dz, dz2) and torch.equal(rs[:, :2], rs2)


def test_loss_takes_the_kernels_under_the_conditions_of_the_cross_entropy_and_is_torch_elsewhere():
    z, t, y = D.inputs(6, 10)
    calls = []
    be = EmulatedDistillBackend()
    real = be.distill_fwd
    be.distill_fwd = lambda *a: (calls.append("fwd"), real(*a))[1]
    want = trainer.distill_loss_torch(z, t, y, 0.4, 2.0, "soft")
    calm.backend.set_loss_kernels(False)
    with calm.backend.use_backend(be):
        assert torch.equal(trainer.distillation_loss(z, t, y, 0.4, 2.0), want) and not calls
        calm.backend.set_loss_kernels(True)
        dm = trainer.DistillMetrics(torch.device("cpu"))
        got = trainer.distillation_loss(z, t, y, 0.4, 2.0, distill_metrics=dm)
        assert calls == ["fwd"] and rel_err(got, want) <= TOL and dm.read()[3] == 6
        assert torch.equal(trainer.distillation_loss(z[0], t[0], y[0], 0.4, 2.0), trainer.distill_loss_torch(z[0], t[0], y[0], 0.4, 2.0))
        assert torch.equal(trainer.distillation_loss(z.double(), t.double(), y.double(), 0.4, 2.0),
                           trainer.distill_loss_torch(z.double(), t.double(), y.double(), 0.4, 2.0))
        assert calls == ["fwd"]
    with calm.backend.use_backend(EmulatedLossBackend()):           # a backend without distill_fwd: torch
        assert torch.equal(trainer.distillation_loss(z, t, y, 0.4, 2.0), want)
    assert torch.equal(trainer.distillation_loss(z, t, y, 0.4, 2.0), want)        # CPU tensors on the product backend
    with pytest.raises(ValueError, match="mode"):
        trainer.distill_loss_torch(z, t, y, 0.4, 2.0, "both")


def test_function_saves_its_inputs_and_row_stats_only_and_gives_the_teacher_no_gradient():
    z, t, y = D.inputs(5, 10)
    sizes = []
    t = t.requires_grad_(True)
    with calm.backend.use_backend(EmulatedDistillBackend()), \
            torch.autograd.graph.saved_tensors_hooks(lambda x: (sizes.append(tuple(x.shape)), x)[1], lambda x: x):
        loss = calm.ops.DistillLossFn.apply(z.requires_grad_(True), t, y, 2.0, 0.5, "soft")
    assert sorted(sizes) == [(5, ROW_STATS), (5, 10), (5, 10), (5, 10)]
    with calm.backend.use_backend(EmulatedDistillBackend()):
        loss.backward()
    assert t.grad is None and z.grad is not None


# ---- the step classes and train(teacher=...) --------------------------------------------------------------------------------
EPOCHS, N_TRAIN, BATCH = 2, 16, 4
SOFT = dict(alpha=0.3, temperature=2.0, mode="soft")
HARD = dict(alpha=0.6, mode="hard")


def _models(rank=0, seed=50):
    """A tiny32_cls student and a teacher with other weights (build_model fills both from one fixed seed); the ranks start
    different, so the launcher has to sync both models.  `seed` is where the torch generator is left."""
    student, teacher = build_model("tiny32_cls", None).train(), build_model("tiny32_cls", None).train()
    g = torch.Generator().manual_seed(1234)
    with torch.no_grad():
        for p in teacher.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
        if rank:
            for p in list(student.parameters()) + list(teacher.parameters()):
                p.add_(0.01)
    torch.manual_seed(seed + rank)
    return student, teacher


def _train(distill, seed=50, rank=0, **kw):
    student, teacher = _models(rank, seed)
    with calm.backend.use_backend(EmulatedBackend()):
        out = trainer.train(student, trainer.make_optimizer(student), None, use_gpu=False, dataset=_TinySet(N_TRAIN),
                            epochs=EPOCHS, batch_size=BATCH, num_classes=10, collate_fn="mix", num_workers=0, log_every=1000,
                            teacher=teacher, distill=distill, **kw)
    return out, teacher


def _hand_loop(distill, rank=0, world=1, accumulate=1, seed=50):
    """What train(teacher=...) with the loss kernels off has to equal: the sampler's order, the CutMix / MixUp collate, an
    eval forward of the teacher without grad, F.cross_entropy + T^2 F.kl_div, clip_grad_norm_ and AdamW."""
    from torch.utils.data import DataLoader, DistributedSampler
    a, T, mode = distill.get("alpha", 0.5), distill.get("temperature", 1.0), distill.get("mode", "soft")
    m, teacher = _models(rank, seed)
    with calm.backend.use_backend(EmulatedBackend()):
        opt = trainer.make_optimizer(m)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=EPOCHS, eta_min=1e-6)
        trainer.sync_module_states(m)
        trainer.sync_module_states(teacher)
        teacher.eval()
        params = [p for p in m.parameters() if p.requires_grad]
        red = None
        if world > 1:
            red = trainer.HeldGradReducer(m) if accumulate > 1 else trainer.BucketedGradReducer(m)
            red.hold = accumulate > 1
        data = _TinySet(N_TRAIN)
        sampler = DistributedSampler(data, num_replicas=world, rank=rank, shuffle=True, seed=2006)
        loader = DataLoader(data, batch_size=BATCH, sampler=sampler, num_workers=0,
                            collate_fn=trainer.SoftMixCollate(num_classes=10, seed=2006 + rank))

        def optimizer_step(n):
            if red is not None:
                red.finish()
            if n > 1:
                torch._foreach_mul_([p.grad for p in params], 1.0 / n)
            torch.nn.utils.clip_grad_norm_(params, max_norm=1.0)
            opt.step()
            opt.zero_grad()

        for epoch in range(EPOCHS):
            sampler.set_epoch(epoch)
            window = 0
            for x, y in loader:
                with torch.no_grad():
                    t = teacher(x)[0].squeeze()
                z = m(x)[0].squeeze()
                if mode == "soft":
                    loss = (1 - a) * F.cross_entropy(z, y) + a * T * T * F.kl_div(F.log_softmax(z / T, 1), F.softmax(t / T, 1),
                                                                                  reduction="batchmean")
                else:
                    loss = (1 - a) * F.cross_entropy(z, y) + a * F.cross_entropy(z, t.argmax(1))
                loss.backward()
                window += 1
                if window == accumulate:
                    optimizer_step(window)
                    window = 0
            if window:
                optimizer_step(window)
            sched.step()
    return m


def _same(a, b, what):
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{what}: differs at {k}"


@pytest.mark.timeout(600)
@pytest.mark.parametrize("tag,distill,accumulate", [("soft", SOFT, 1), ("hard", HARD, 1), ("soft-accum2", SOFT, 2)])
def test_train_equals_the_hand_written_loop_bit_for_bit(tag, distill, accumulate, tmp_path):
    calm.backend.set_loss_kernels(False)
    _, fresh_teacher = _models()
    before = {k: v.clone() for k, v in fresh_teacher.state_dict().items()}
    ckpt = str(tmp_path / "model_cls.pth")
    out, teacher = _train(distill, accumulate=accumulate, checkpoint_path=ckpt, ema=0.9)
    _same(out, _hand_loop(distill, accumulate=accumulate), tag)
    # the teacher comes back as it went in, and no file holds it
    assert teacher.training and not any(p.requires_grad for p in teacher.parameters())
    after = teacher.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert all(v.device.type == "cpu" for v in after.values())
    for f in os.listdir(tmp_path):
        sd = torch.load(str(tmp_path / f))
        assert set(sd) == set(out.state_dict()), f
        assert not any(torch.equal(sd[k], before[k]) for k in sd if k.endswith("weight_orig")), f
    assert sorted(os.listdir(tmp_path)) == ["model_cls.pth", "model_cls_ema.pth"]
    assert not torch.distributed.is_initialized()


def test_no_teacher_builds_the_step_classes_of_today():
    built = []
    classes = ("TrainStep", "AccumTrainStep", "DistillTrainStep", "AccumDistillTrainStep")
    real = {n: getattr(trainer, n).__init__ for n in classes}

    def spy(name):
        def init(self, *a, **kw):
            if not built or built[-1][0] is not self:
                built.append((self, type(self).__name__))
            return real[name](self, *a, **kw)
        return init
    for n in classes:
        getattr(trainer, n).__init__ = spy(n)
    try:
        for kw, want in ((dict(), "TrainStep"), (dict(accumulate=2), "AccumTrainStep")):
            student, teacher = _models()
            with calm.backend.use_backend(EmulatedBackend()):
                for t, name in ((None, want), (teacher, want.replace("TrainStep", "DistillTrainStep"))):
                    del built[:]
                    trainer.train(student, trainer.make_optimizer(student), None, use_gpu=False, dataset=_TinySet(8), epochs=1,
                                  batch_size=4, num_classes=10, log_every=1000, max_steps=1, teacher=t, **kw)
                    assert [n for _, n in built] == [name]
    finally:
        for n in classes:
            getattr(trainer, n).__init__ = real[n]
    assert issubclass(trainer.AccumDistillTrainStep, trainer.AccumTrainStep)
    assert issubclass(trainer.AccumDistillTrainStep, trainer.DistillTrainStep)
    assert "_finish" not in vars(trainer.DistillTrainStep) and "_optimizer_step" not in vars(trainer.AccumDistillTrainStep)


def test_step_takes_a_module_or_a_predictor_and_freezes_the_teacher():
    student, teacher = _models()
    with calm.backend.use_backend(EmulatedBackend()):
        x, y = torch.randn(4, 3, 32, 32), torch.softmax(torch.randn(4, 10), 1)
        losses = []
        for wrap in (False, True):
            s, _ = _models()
            step = trainer.DistillTrainStep(s, trainer.make_optimizer(s), trainer.Predictor(teacher) if wrap else teacher,
                                            **SOFT)
            assert isinstance(step.teacher, trainer.Predictor) and step.teacher.model is teacher
            assert not any(p.requires_grad for p in teacher.parameters())
            rng = torch.get_rng_state()
            t_logits = step._teacher_forward(x)
            assert torch.equal(torch.get_rng_state(), rng) and teacher.training      # the teacher forward moves no stream
            assert not t_logits.requires_grad
            losses.append(step(x, y)[0])
        assert torch.equal(losses[0], losses[1])
        want = trainer.distill_loss_torch(student(x)[0].squeeze(), t_logits.squeeze(), y, **SOFT)
        assert torch.equal(losses[0], want.detach())
        for kw in (dict(mode="both"), dict(alpha=1.5), dict(temperature=0.0)):
            with pytest.raises(ValueError, match=next(iter(kw))):
                trainer.DistillTrainStep(student, trainer.make_optimizer(student), teacher, **kw)


@pytest.mark.timeout(600)
def test_train_resumes_exactly_with_the_same_teacher_handed_in_again(tmp_path):
    calm.backend.set_loss_kernels(False)
    fa, fb, fc, fn = (str(tmp_path / f"{n}.snap") for n in "abcn")
    a, _ = _train(SOFT, snapshot_path=fa, ema=0.99)
    _train(SOFT, snapshot_path=fb, max_steps=3, ema=0.99)
    assert trainer.TrainState.read_header(fb)[0]["host"]["progress"] == {"epoch": 0, "batch": 3, "step": 3}
    c, _ = _train(SOFT, seed=51, snapshot_path=fc, resume=fb, ema=0.99)          # another student seed, the same teacher
    _assert_same_run(a, c, fa, fc)
    # the snapshot holds what a run without a teacher holds
    student, _ = _models()
    with calm.backend.use_backend(EmulatedBackend()):
        trainer.train(student, trainer.make_optimizer(student), None, use_gpu=False, dataset=_TinySet(N_TRAIN), epochs=EPOCHS,
                      batch_size=BATCH, num_classes=10, log_every=1000, snapshot_path=fn, ema=0.99)
    ha, hn = trainer.TrainState.read_header(fa)[0], trainer.TrainState.read_header(fn)[0]
    assert len(ha["entries"]) == len(hn["entries"]) and ha["packed_bytes"] == hn["packed_bytes"]


# ---- two gloo ranks --------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


RANK_RUNS = [("soft", SOFT, 1), ("hard", HARD, 1), ("soft-accum2", SOFT, 2)]


def _two_rank_worker(rank, world, ports, outdir):
    torch.set_num_threads(2)
    calm.backend.set_loss_kernels(False)
    for i, (tag, distill, accumulate) in enumerate(RANK_RUNS):
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(ports[2 * i]), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        out, teacher = _train(distill, rank=rank, accumulate=accumulate)
        assert not torch.distributed.is_initialized()
        os.environ["MASTER_PORT"] = str(ports[2 * i + 1])
        torch.distributed.init_process_group(backend="gloo")
        hand = _hand_loop(distill, rank, world, accumulate)
        torch.distributed.destroy_process_group()
        torch.save({"train": out.state_dict(), "hand": hand.state_dict(), "teacher": teacher.state_dict()},
                   os.path.join(outdir, f"{tag}_rank{rank}.pt"))


@pytest.mark.timeout(900)
def test_train_equals_the_hand_written_loop_on_two_gloo_ranks(tmp_path):
    d = str(tmp_path)
    mp.spawn(_two_rank_worker, args=(2, [_free_port() for _ in range(2 * len(RANK_RUNS))], d), nprocs=2, join=True)
    _, teacher0 = _models(0)
    for tag, _, _ in RANK_RUNS:
        r0, r1 = (torch.load(os.path.join(d, f"{tag}_rank{r}.pt")) for r in range(2))
        for k in r0["train"]:
            assert torch.equal(r0["train"][k], r1["train"][k]), f"{tag}: ranks diverged at {k}"
            assert torch.equal(r0["train"][k], r0["hand"][k]), f"{tag}: hand-written loop differs at {k}"
        for k, v in teacher0.state_dict().items():                  # rank 0's teacher reached rank 1
            assert torch.equal(r1["teacher"][k], v), k


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_process_group_and_name_their_keyword():
    data = torch.utils.data.TensorDataset(torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,)))
    lin, teacher = torch.nn.Linear(4, 4), torch.nn.Linear(4, 4)
    sgd = torch.optim.SGD(lin.parameters(), lr=0.1)
    gen_teacher = torch.nn.Linear(4, 4)
    gen_teacher.generate = True
    run = lambda **kw: trainer.train(lin, kw.pop("optimizer", sgd), dataset=data, epochs=1, batch_size=2, num_classes=10,  # noqa: E731
                                     **dict(dict(use_gpu=False), **kw))
    for kw, word in ((dict(teacher=teacher, task="reg"), "teacher"),
                     (dict(teacher=teacher, graph=True, use_gpu=True, optimizer="fused"), "teacher"),
                     (dict(distill={"alpha": 0.3}), "distill"),
                     (dict(teacher=gen_teacher), "generate=True"),
                     (dict(teacher=trainer.Predictor(gen_teacher)), "generate=True"),
                     (dict(teacher=teacher, distill={"alpha": 0.3, "beta": 1.0}), "distill"),
                     (dict(teacher=teacher, distill={"mode": "both"}), "mode"),
                     (dict(teacher=teacher, distill={"alpha": 2.0}), "alpha"),
                     (dict(teacher=teacher, distill={"temperature": 0.0}), "temperature")):
        with pytest.raises(ValueError, match=word):
            run(**kw)
        assert not torch.distributed.is_initialized(), kw
    assert teacher.weight.requires_grad and teacher.training       # a refused call leaves the teacher alone
