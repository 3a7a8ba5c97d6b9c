"""Binary cross-entropy without a GPU: the two C-ABI additions are declared, exported and bound and refuse bad arguments
before any launch; the float64 checker (tests/bce_f64.py) passes the torch emulation of the entry points
(tests/emulated_bce.py) and reports each of its planted faults; trainer.soft_target_bce with the kernels off is
F.binary_cross_entropy_with_logits bit for bit and goes through ops.BinaryCrossEntropyFn with them on;
TrainStep(loss="bce") and train(loss="bce") against hand-written steps and loops on one and on two gloo ranks; what is
refused."""
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
import bce_f64 as K  # noqa: E402
import weights as W  # noqa: E402
from emulated_backend import EmulatedBackend  # noqa: E402
from emulated_bce import EmulatedBceBackend  # noqa: E402
from helpers import CONFIGS, load_golden  # noqa: E402
from test_host_logic_cpu import build_model  # noqa: E402
from test_loss_cpu import _KeepGrads  # noqa: E402
from test_snapshot_cpu import _TinySet  # noqa: E402
from importlib import import_module  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
HEADER = os.path.join(ROOT, "include", "calm_vit.h")


@pytest.fixture(autouse=True)
def _restore_switch():
    prev = calm.backend.get_loss_kernels()
    yield
    calm.backend.set_loss_kernels(prev)
    calm.ops.set_noise_override(None)


def _ids(v):
    B, C, scale, kind, flags, threshold, dloss, seed = v
    return f"{B}x{C}-s{scale:g}-{kind}-f{flags}-t{threshold:g}-d{dloss:g}"


def run_backend(be, v):
    """One forward on a zeroed metrics buffer and one backward of `be` on the inputs of variant v: (got, ref) of the checker."""
    B, C, scale, kind, flags, threshold, dloss, seed = v
    z, y = K.inputs(B, C, scale, kind, seed)
    loss, metrics, dlogits = torch.full((), -1.0), torch.zeros(4), torch.full((B, C), 7.0)
    be.bce_fwd(z, y, flags, threshold, loss, metrics, B, C)
    be.bce_bwd(z, y, flags, threshold, torch.tensor([dloss]), dlogits, B, C)
    return {"loss": loss, "dlogits": dlogits, "metrics": metrics}, K.reference(z, y, flags, threshold, dloss)


# ---- the checker on the emulation and on its planted faults ------------------------------------------------------------
@pytest.mark.parametrize("v", K.VARIANTS, ids=_ids)
def test_checker_passes_the_clean_emulation(v):
    got, ref = run_backend(EmulatedBceBackend(), v)
    assert K.check(got, ref) == []


def test_the_cases_hold_what_their_comments_say():
    assert len(set(K.VARIANTS)) == len(K.VARIANTS)
    assert {(v[0], v[1]) for v in K.VARIANTS} == set(K.CASES)
    assert {v[2] for v in K.VARIANTS} == {1.0, 8.0, 30.0, 100.0} and {v[6] for v in K.VARIANTS} == {1.0, 3.0}
    assert {(v[3], v[5]) for v in K.VARIANTS if v[4] & K.THRESHOLD} >= {("cutmix", 0.2), ("smoothed", 0.0), ("cutmix", 0.0)}
    # the two (3, 3) threshold variants: the count against the thresholded targets would be another one
    for kind, thr, seed in (("cutmix", 0.2, K.SEED_CUTMIX_02), ("smoothed", 0.0, K.SEED_SMOOTHED_00)):
        z, y = K.inputs(3, 3, 1.0, kind, seed)
        assert K.agreement(z, y) != K.agreement(z, K.effective_targets(y, K.THRESHOLD, thr))
    # a naive log(1 + exp(z)) overflows in fp32 at scale 100
    z, _ = K.inputs(4, 1000, 100.0)
    assert bool(torch.isinf(torch.exp(z)).any())


class _MeanOverBatch(EmulatedBceBackend):
    """mean over B where B * C is due"""
    _denominator = staticmethod(lambda flags, B, C: float(B))


class _ThresholdNotStrict(EmulatedBceBackend):
    """>= in place of > at the threshold"""
    _threshold = staticmethod(lambda y, threshold: (y >= threshold).to(y.dtype))


class _ThresholdForwardOnly(EmulatedBceBackend):
    """the threshold applied in the forward only"""

    def _bwd_targets(self, y, flags, threshold):
        return y


class _NaiveSoftplus(EmulatedBceBackend):
    """log(1 + exp(z)) - z t"""
    _terms = staticmethod(lambda z, t: torch.log(1.0 + torch.exp(z)) - z * t)


class _AgreementThresholded(EmulatedBceBackend):
    """the agreement taken against the thresholded targets"""
    _agreement_targets = staticmethod(lambda y, t: t)


class _UpstreamIgnored(EmulatedBceBackend):
    """dloss ignored"""
    _upstream = staticmethod(lambda dloss: torch.ones(()))


class _TargetSignFlipped(EmulatedBceBackend):
    """the sign of the target term flipped: max(z, 0) + z t + log1p(exp(-|z|))"""
    _terms = staticmethod(lambda z, t: z.clamp_min(0.0) + z * t + torch.log1p(torch.exp(-z.abs())))


class _TailDropped(EmulatedBceBackend):
    """the last C % 4 classes of a row dropped"""
    _classes = staticmethod(lambda z: z[:, :z.shape[1] - z.shape[1] % 4])


class _MetricsHoldTheMean(EmulatedBceBackend):
    """metrics[0] given the loss in place of B * loss"""
    _metrics_loss = staticmethod(lambda loss, B: loss)


FAULTS = [_MeanOverBatch, _ThresholdNotStrict, _ThresholdForwardOnly, _NaiveSoftplus, _AgreementThresholded,
          _UpstreamIgnored, _TargetSignFlipped, _TailDropped, _MetricsHoldTheMean]


@pytest.mark.parametrize("fault", FAULTS, ids=lambda f: f.__name__.strip("_"))
def test_checker_reports_every_planted_fault_on_at_least_one_case(fault):
    caught = [v for v in K.VARIANTS if K.check(*run_backend(fault(), v))]
    print(f"\n{fault.__doc__}: reported on {len(caught)} of {len(K.VARIANTS)} variants")
    assert caught, fault.__doc__


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
P = 0x7f0000010000                             # never dereferenced: every call below is refused before any launch


def _fwd_args(**kw):
    a = dict(logits=P, ld=10, targets=P, td=10, flags=0, threshold=0.0, loss=P, metrics=None, B=3, C=10, partials=P,
             stream=None)
    a.update(kw)
    return list(a.values())


def _bwd_args(**kw):
    a = dict(logits=P, ld=10, targets=P, td=10, flags=0, threshold=0.0, dloss=P, dlogits=P, B=3, C=10, stream=None)
    a.update(kw)
    return list(a.values())


def test_entry_points_are_declared_exported_bound_and_sized():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(calm_\w+)\s*\(", text, flags=re.M))
    lib = binding.load()
    for n in ("calm_bce_fwd", "calm_bce_bwd"):
        assert n in declared and n in binding.SIGNATURES and hasattr(lib, n), n
    assert int(re.search(r"#define\s+CALM_ABI_VERSION\s+(\d+)", raw).group(1)) == binding.ABI_VERSION == lib.calm_abi_version() == 7
    assert re.search(r"CALM_RED_BCE\s*=\s*10\b", text) and binding.RED_BCE == 10
    assert re.search(r"CALM_BCE_SUM_CLASSES\s*=\s*1\b", text) and re.search(r"CALM_BCE_THRESHOLD\s*=\s*2\b", text)
    assert (binding.BCE_SUM_CLASSES, binding.BCE_THRESHOLD) == (K.SUM_CLASSES, K.THRESHOLD) == (1, 2)
    for B, C in K.CASES + [(256, 1000)]:
        assert int(lib.calm_reduce_scratch_floats(binding.RED_BCE, B, C)) == 2 * B
    assert hasattr(calm.backend.HipBackend, "bce_fwd") and hasattr(calm.backend.HipBackend, "bce_bwd")


def test_every_refusal_is_returned_without_a_gpu():
    lib = binding.load()
    shared = [dict(logits=None), dict(targets=None), dict(B=0), dict(B=-1), dict(C=0), dict(C=-3), dict(flags=4), dict(flags=7),
              dict(flags=-1), dict(flags=K.THRESHOLD, threshold=math.nan), dict(flags=K.THRESHOLD, threshold=math.inf),
              dict(flags=K.THRESHOLD | K.SUM_CLASSES, threshold=-math.inf)]
    for kw in shared + [dict(loss=None), dict(partials=None)]:
        assert lib.calm_bce_fwd(*_fwd_args(**kw)) == binding.E_INVAL, kw
    for kw in shared + [dict(dloss=None), dict(dlogits=None)]:
        assert lib.calm_bce_bwd(*_bwd_args(**kw)) == binding.E_INVAL, kw
    for B, C in ((1 << 16, 1 << 15), (1 << 30, 2), (3, (1 << 31) - 1)):              # B * C >= 2^31
        assert lib.calm_bce_fwd(*_fwd_args(B=B, C=C, ld=C, td=C)) == binding.E_UNSUPP, (B, C)
        assert lib.calm_bce_bwd(*_bwd_args(B=B, C=C, ld=C, td=C)) == binding.E_UNSUPP, (B, C)
    # a bad argument wins over the size, and a NaN threshold without the flag is not looked at (the size still is)
    assert lib.calm_bce_fwd(*_fwd_args(B=1 << 16, C=1 << 15, flags=4)) == binding.E_INVAL
    assert lib.calm_bce_fwd(*_fwd_args(B=1 << 16, C=1 << 15, threshold=math.nan)) == binding.E_UNSUPP


# ---- trainer.soft_target_bce -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cutmix", "smoothed"])
def test_with_the_kernels_off_the_loss_is_torchs_bit_for_bit(kind):
    calm.backend.set_loss_kernels(False)
    z, y = K.inputs(6, 10, 1.0, kind)
    for thr in (None, 0.2, 0.0):
        t = y if thr is None else (y > thr).float()
        for sum_classes in (False, True):
            for rows in (slice(None), 0):                          # 2-D, and the 1-D logits of squeeze() at batch 1
                a = z[rows].clone().requires_grad_(True)
                b = z[rows].clone().requires_grad_(True)
                got = trainer.soft_target_bce(a, y[rows], None, thr, sum_classes)
                if sum_classes:
                    want = F.binary_cross_entropy_with_logits(b, t[rows], reduction="sum") / (6 if b.dim() == 2 else 1)
                else:
                    want = F.binary_cross_entropy_with_logits(b, t[rows])
                got.backward()
                want.backward()
                assert torch.equal(got, want) and torch.equal(a.grad, b.grad), (thr, sum_classes, rows)
    # switched on, what the kernels do not serve still is torch: CPU tensors on the product backend, 1-D logits, a backend
    # without bce_fwd
    calm.backend.set_loss_kernels(True)
    want = F.binary_cross_entropy_with_logits(z, y)
    assert torch.equal(trainer.soft_target_bce(z, y), want)
    with calm.backend.use_backend(EmulatedBceBackend()):
        assert torch.equal(trainer.soft_target_bce(z[0], y[0]), F.binary_cross_entropy_with_logits(z[0], y[0]))
        assert torch.equal(trainer.soft_target_bce(z.double(), y.double()), F.binary_cross_entropy_with_logits(z.double(), y.double()))
    with calm.backend.use_backend(EmulatedBackend()):
        assert torch.equal(trainer.soft_target_bce(z, y), want)


@pytest.mark.parametrize("thr,sum_classes", [(None, False), (0.2, True)])
def test_with_the_kernels_on_the_loss_is_the_function_and_the_metrics_accumulate(thr, sum_classes):
    calls = []
    be = EmulatedBceBackend()
    for fn in ("bce_fwd", "bce_bwd"):
        setattr(be, fn, (lambda real, fn=fn: lambda *a: (calls.append(fn), real(*a))[1])(getattr(be, fn)))
    flags = (K.SUM_CLASSES if sum_classes else 0) | (K.THRESHOLD if thr is not None else 0)
    z, y = K.inputs(5, 10, 1.0)
    ref = K.reference(z, y, flags, thr or 0.0, 3.0)
    m = trainer.StepMetrics(torch.device("cpu"))
    calm.backend.set_loss_kernels(True)
    sizes = []
    with calm.backend.use_backend(be), \
            torch.autograd.graph.saved_tensors_hooks(lambda t: (sizes.append(tuple(t.shape)), t)[1], lambda t: t):
        zl = z.clone().requires_grad_(True)
        yl = y.clone().requires_grad_(True)
        loss = trainer.soft_target_bce(zl, yl, m, thr, sum_classes)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        (loss * 3.0).backward()
        assert calls == ["bce_fwd", "bce_bwd"] and sorted(sizes) == [(5, 10), (5, 10)]      # logits and targets, nothing else
        assert yl.grad is None                                                            # the gradient goes to the logits alone
        assert K.check({"loss": loss.detach(), "dlogits": zl.grad, "metrics": m.buf}, ref) == []
        z2, y2 = K.inputs(5, 10, 1.0, seed=1)
        loss2 = trainer.soft_target_bce(z2, y2, m, thr, sum_classes)
    loss_sum, agree, rows, steps = m.read()
    assert (agree, rows, steps) == (ref["agree"] + K.agreement(z2, y2), 10, 2)
    want = 5 * (float(loss.detach()) + float(loss2))
    assert abs(loss_sum - want) <= 1e-5 * want


# ---- TrainStep(loss=) --------------------------------------------------------------------------------------------------
def _first_step(loss, hand=None, bs=2):
    """(loss, gradients after clipping) of the first trainer step of nano48_cls on the CPU, as first_step of
    tests/test_loss_cpu.py; hand: the loss function of a step written out here in place of TrainStep."""
    name = "nano48_cls"
    cfg = CONFIGS[name]
    m = build_model(name, load_golden(name), "cpu").train()
    x = torch.from_numpy(W.make_input((bs, 3, cfg.seq_length, cfg.seq_length), 2))
    y = K.inputs(bs, cfg.out_features, 1.0)[1]
    params = [p for p in m.parameters() if p.requires_grad]
    opt = _KeepGrads(params, lr=0.0)
    calm.ops.set_noise_override(W.NoiseStream(7))
    try:
        if hand is None:
            out, _ = trainer.TrainStep(m, opt, None, loss=loss)(x, y)
        else:
            out = hand(m(x)[0].squeeze(), y)
            out.backward()
            torch.nn.utils.clip_grad_norm_(params, max_norm=1.0)
            opt.step()
            opt.zero_grad()
            out = out.detach()
    finally:
        calm.ops.set_noise_override(None)
    return out, dict(zip([n for n, p in m.named_parameters() if p.requires_grad], opt.kept))


@pytest.mark.parametrize("loss,hand", [
    ("bce", lambda z, y: F.binary_cross_entropy_with_logits(z, y)),
    ({"name": "bce"}, lambda z, y: F.binary_cross_entropy_with_logits(z, y)),
    ({"name": "bce", "target_threshold": 0.2, "sum_classes": True},
     lambda z, y: F.binary_cross_entropy_with_logits(z, (y > 0.2).float(), reduction="sum") / z.shape[0]),
    (None, lambda z, y: F.cross_entropy(z, y)), ("ce", lambda z, y: F.cross_entropy(z, y))],
    ids=["bce", "bce-dict", "bce-threshold-sum", "none", "ce"])
def test_train_step_with_a_loss_equals_the_hand_written_step_bit_for_bit(loss, hand):
    calm.backend.set_loss_kernels(False)
    with calm.backend.use_backend(EmulatedBackend()):
        (l_step, g_step), (l_hand, g_hand) = _first_step(loss), _first_step(None, hand)
    assert torch.equal(l_step, l_hand)
    for n in g_hand:
        assert g_step[n] is not None and torch.equal(g_step[n], g_hand[n]), n


def test_bce_step_differs_from_the_cross_entropy_step():
    calm.backend.set_loss_kernels(False)
    with calm.backend.use_backend(EmulatedBackend()):
        (l_bce, g_bce), (l_ce, g_ce) = _first_step("bce"), _first_step(None)
    assert not torch.equal(l_bce, l_ce) and any(not torch.equal(g_bce[n], g_ce[n]) for n in g_ce)


def test_loss_settings_normalise_and_refuse():
    ls = trainer._loss_settings
    assert ls("x", None) == ls("x", "ce") == ls("x", {"name": "ce"}) == {"name": "ce"}
    assert ls("x", "bce") == ls("x", {"name": "bce"}) == {"name": "bce", "target_threshold": None, "sum_classes": False}
    full = {"name": "bce", "target_threshold": 0.25, "sum_classes": True}
    assert ls("x", full) == full and ls("x", ls("x", full)) == full
    assert ls("x", {"name": "bce", "target_threshold": 0})["target_threshold"] == 0.0
    for bad, word in (("focal", "name"), ({"name": "hinge"}, "name"), ({"target_threshold": 0.2}, "name"), (3, "loss"),
                      ({"name": "bce", "pos_weight": 2.0}, "pos_weight"), ({"name": "ce", "sum_classes": True}, "sum_classes"),
                      ({"name": "bce", "target_threshold": math.inf}, "target_threshold"),
                      ({"name": "bce", "target_threshold": math.nan}, "target_threshold"),
                      ({"name": "bce", "target_threshold": "0.2"}, "target_threshold"),
                      ({"name": "bce", "target_threshold": True}, "target_threshold"),
                      ({"name": "bce", "sum_classes": 1}, "sum_classes")):
        with pytest.raises(ValueError, match=word):
            ls("who", bad)
    with pytest.raises(ValueError, match="TrainStep"):
        m = torch.nn.Linear(2, 2)
        trainer.TrainStep(m, torch.optim.SGD(m.parameters(), lr=0.1), loss="focal")


def test_distillation_and_generative_steps_refuse_another_loss():
    student, teacher = build_model("tiny32_cls", None), build_model("tiny32_cls", None)
    gen = build_model("nano48_gen", None)
    with calm.backend.use_backend(EmulatedBackend()):
        for cls, args, kw in ((trainer.DistillTrainStep, (student, trainer.make_optimizer(student), teacher), {}),
                              (trainer.AccumDistillTrainStep, (student, trainer.make_optimizer(student), teacher), {"accumulate": 2}),
                              (trainer.RegTrainStep, (gen, trainer.make_optimizer(gen)), {}),
                              (trainer.AccumRegTrainStep, (gen, trainer.make_optimizer(gen)), {"accumulate": 2})):
            for loss in ("bce", {"name": "bce", "sum_classes": True}):
                with pytest.raises(ValueError, match=f"{cls.__name__}.*loss="):
                    cls(*args, loss=loss, **kw)
            for loss in (None, "ce"):
                cls(*args, loss=loss, **kw)                         # the cross-entropy, named or not, is today's step
        with pytest.raises(ValueError, match="name"):
            trainer.RegTrainStep(gen, trainer.make_optimizer(gen), loss="focal")


def test_train_refusals_come_before_any_process_group():
    data = torch.utils.data.TensorDataset(torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,)))
    lin, teacher = torch.nn.Linear(4, 4), torch.nn.Linear(4, 4)
    sgd = torch.optim.SGD(lin.parameters(), lr=0.1)
    for kw, word in ((dict(task="reg", loss="bce"), 'task="reg"'), (dict(task="reg", loss="ce"), 'task="reg"'),
                     (dict(teacher=teacher, loss="bce"), "teacher"),
                     (dict(teacher=teacher, loss={"name": "bce", "target_threshold": 0.2}), "teacher"),
                     (dict(loss="focal"), "name"), (dict(loss={"name": "bce", "smoothing": 0.1}), "smoothing"),
                     (dict(loss={"name": "bce", "target_threshold": math.inf}), "target_threshold"),
                     (dict(loss={"name": "bce", "sum_classes": "yes"}), "sum_classes")):
        with pytest.raises(ValueError, match=word):
            trainer.train(lin, sgd, use_gpu=False, dataset=data, epochs=1, batch_size=2, num_classes=10, **kw)
        assert not torch.distributed.is_initialized(), kw
    assert teacher.weight.requires_grad and teacher.training       # a refused call leaves the teacher alone


# ---- train(loss=) ------------------------------------------------------------------------------------------------------
EPOCHS, N_TRAIN, BATCH = 2, 16, 4
THRESHOLD_SUM = {"name": "bce", "target_threshold": 0.2, "sum_classes": True}


def _model(rank=0, seed=50):
    """tiny32_cls; the ranks start different, so the launcher has to sync.  `seed` is where the torch generator is left."""
    m = build_model("tiny32_cls", None).train()
    if rank:
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.01)
    torch.manual_seed(seed + rank)
    return m


def _train(optimizer="torch", rank=0, **kw):
    m = _model(rank)
    with calm.backend.use_backend(EmulatedBackend()):
        return trainer.train(m, "fused" if optimizer == "fused" else trainer.make_optimizer(m), None, use_gpu=False,
                             dataset=_TinySet(N_TRAIN), epochs=EPOCHS, batch_size=BATCH, num_classes=10, collate_fn="mix",
                             num_workers=0, log_every=1000, **kw)


def _hand_bce(z, y, loss):
    s = trainer._loss_settings("hand", loss)
    if s["target_threshold"] is not None:
        y = (y > s["target_threshold"]).float()
    if s["sum_classes"]:
        return F.binary_cross_entropy_with_logits(z, y, reduction="sum") / z.shape[0]
    return F.binary_cross_entropy_with_logits(z, y)


def _hand_loop(loss, rank=0, world=1, accumulate=1, label_smoothing=0.0):
    """What train(loss="bce") with the loss kernels off and a torch optimizer has to equal: the sampler's order, the
    CutMix / MixUp collate, F.binary_cross_entropy_with_logits called here, clip_grad_norm_ and AdamW."""
    from torch.utils.data import DataLoader, DistributedSampler
    m = _model(rank)
    with calm.backend.use_backend(EmulatedBackend()):
        opt = trainer.make_optimizer(m)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=EPOCHS, eta_min=1e-6)
        trainer.sync_module_states(m)
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
                if label_smoothing:                                # y (1 - eps) + eps / C, rounded as train()'s one op rounds it
                    y = torch.add(torch.tensor(label_smoothing / 10, dtype=torch.float32), y, alpha=1.0 - label_smoothing)
                _hand_bce(m(x)[0].squeeze(), y, loss).backward()
                window += 1
                if window == accumulate:
                    optimizer_step(window)
                    window = 0
            if window:
                optimizer_step(window)
            sched.step()
    return m


class HandBceStep(trainer.TrainStep):
    """The step of train(optimizer="fused") with the BCE written out here; train() is not told about the loss."""
    hand_loss = "bce"

    def __call__(self, x, y_soft):
        y_hat, _ = self.model(x)
        return self._finish(_hand_bce(y_hat.squeeze(), y_soft, self.hand_loss), y_hat)


def _same(a, b, what):
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{what}: differs at {k}"


def _differ(a, b):
    return any(not torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("tag,loss,kw", [("bce", "bce", {}), ("threshold-sum-accum2", THRESHOLD_SUM, {"accumulate": 2}),
                                         ("bce-smoothing", "bce", {"label_smoothing": 0.1})])
def test_train_equals_the_hand_written_loop_bit_for_bit(tag, loss, kw, capsys):
    calm.backend.set_loss_kernels(False)
    out = _train(loss=loss, **kw)
    s = trainer._loss_settings("test", loss)
    assert (f"loss: binary cross-entropy with logits, target_threshold {s['target_threshold']}, sum_classes {s['sum_classes']}"
            in capsys.readouterr().out)
    _same(out, _hand_loop(loss, **kw), tag)
    assert all(bool(torch.isfinite(p).all()) for p in out.parameters())
    assert not torch.distributed.is_initialized()


@pytest.mark.timeout(600)
def test_train_with_the_fused_optimizer_equals_the_hand_written_step_and_none_is_todays_run(capsys):
    calm.backend.set_loss_kernels(False)
    out = _train("fused", loss="bce", ema=0.9)
    capsys.readouterr()
    real = trainer._STEP_CLASSES["cls", False]
    trainer._STEP_CLASSES["cls", False] = HandBceStep
    try:
        hand = _train("fused", ema=0.9)
    finally:
        trainer._STEP_CLASSES["cls", False] = real
    _same(out, hand, 'train("fused", loss="bce") against the hand-written step')
    plain = _train("fused", ema=0.9)
    assert "binary cross-entropy" not in capsys.readouterr().out
    assert _differ(out, plain)
    _same(plain, _train("fused", ema=0.9, loss=None), "loss=None against a run that never mentions the argument")
    _same(plain, _train("fused", ema=0.9, loss="ce"), 'loss="ce" against a run that never mentions the argument')


# ---- two gloo ranks ----------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


RANK_RUNS = [("bce", "bce", 1), ("threshold-sum-accum2", THRESHOLD_SUM, 2)]


def _two_rank_worker(rank, world, ports, outdir):
    torch.set_num_threads(2)
    calm.backend.set_loss_kernels(False)
    for i, (tag, loss, accumulate) in enumerate(RANK_RUNS):
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(ports[2 * i]), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        out = _train(rank=rank, loss=loss, accumulate=accumulate)
        assert not torch.distributed.is_initialized()
        os.environ["MASTER_PORT"] = str(ports[2 * i + 1])
        torch.distributed.init_process_group(backend="gloo")
        hand = _hand_loop(loss, rank, world, accumulate)
        torch.distributed.destroy_process_group()
        torch.save({"train": out.state_dict(), "hand": hand.state_dict()}, os.path.join(outdir, f"{tag}_rank{rank}.pt"))


@pytest.mark.timeout(900)
def test_train_equals_the_hand_written_loop_on_two_gloo_ranks(tmp_path):
    d = str(tmp_path)
    mp.spawn(_two_rank_worker, args=(2, [_free_port() for _ in range(2 * len(RANK_RUNS))], d), nprocs=2, join=True)
    for tag, _, _ in RANK_RUNS:
        r0, r1 = (torch.load(os.path.join(d, f"{tag}_rank{r}.pt")) for r in range(2))
        for k in r0["train"]:
            assert torch.equal(r0["train"][k], r1["train"][k]), f"{tag}: ranks diverged at {k}"
            assert torch.equal(r0["train"][k], r0["hand"][k]), f"{tag}: hand-written loop differs at {k}"
