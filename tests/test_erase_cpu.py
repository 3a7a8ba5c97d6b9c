"""RandomErasing in the device collate and label smoothing, without a GPU: the float64 emulation the kernel is tested
against (tests/emulated_erase.py) against a hand-written composition, the cap on the pixels its GPU cases leave out, the
draws of trainer.DeviceErase, the C boundary of calm_augment_collate_erase, and train(label_smoothing=) /
train(random_erasing=) as far as they run on a host."""
import ctypes
import math
import os
import subprocess
import sys
import tempfile
from importlib import import_module

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import calm_vit_dte_amd as calm  # noqa: E402
import emulated_augment as EA  # noqa: E402
import emulated_erase as EE  # noqa: E402
from emulated_backend import EmulatedBackend  # noqa: E402
from test_host_logic_cpu import build_model  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
MAX_NEAR = 0.005                                          # the cap of tests/test_augment_gpu.py


# ---- the emulation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EE.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{'noise' if c[2] else 'const'}")
def test_emulation_equals_a_hand_written_composition(case):
    """EA.augment_collate(mode 0) per sample, a slice assignment of the fill, a numpy mix — within 1e-12 of the emulation
    in every mode and both layouts."""
    shape, boxset, noise_fill = case
    src, t, H, W = EE.case_inputs(shape)
    recs = EE.box_sets(H, W)[boxset]
    e = EA.augment_collate(src, t, H, W, 0, 1.0, None, EE.MEAN, EE.STD)[0].copy()
    for b, (y, x, h, w) in enumerate(recs):
        if h == 0 or w == 0:
            continue
        if noise_fill:
            e[b, :, y:y + h, x:x + w] = EE.noise(EE.KEY, b, H, W)[:, y:y + h, x:x + w]
        else:
            for c in range(3):
                e[b, c, y:y + h, x:x + w] = float(np.float32(EE.VALUE[c]))
    partner = e[[2, 0, 1]]                                # sample b's partner is (b - 1) mod 3
    y1, y2, x1, x2 = EE.CUTMIX[shape]
    cut = e.copy()
    cut[:, :, y1:y2, x1:x2] = partner[:, :, y1:y2, x1:x2]
    want = {0: e, 1: e * 0.3 + partner * 0.7, 2: cut}
    for mode in (0, 1, 2):
        for tokens in (False, True):
            ref = want[mode].transpose(0, 2, 3, 1).reshape(3, H, 3 * W) if tokens else want[mode]
            got = EE.case_reference(shape, boxset, noise_fill, mode, tokens)[0]
            assert np.abs(got - ref).max() <= 1e-12, (mode, tokens)


@pytest.mark.parametrize("case", EE.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{'noise' if c[2] else 'const'}")
def test_gpu_cases_leave_out_at_most_half_a_percent(case):
    for mode in (0, 1, 2):
        near = EE.case_reference(*case, mode, False)[2]
        assert near.mean() <= MAX_NEAR, (case, mode, near.mean())
    boxes = EE.case_samples(*case)[4]
    trainer.DeviceErase.check(boxes, *EE.case_inputs(case[0])[2:])


def test_noise_of_the_emulation_is_bounded_and_keyed_by_sample_and_pixel():
    a = EE.noise(EE.KEY, 1, 19, 70)
    assert a.shape == (3, 19, 70) and np.abs(a).max() <= math.sqrt(48.0 * math.log(2.0))
    assert np.array_equal(a, EE.noise(EE.KEY, 1, 19, 70))
    assert not np.array_equal(a, EE.noise(EE.KEY, 2, 19, 70))
    # p = (s H + y) W + x: sample 1's first row is the counter that follows sample 0's last row
    both = EE.noise(EE.KEY, 0, 38, 70)
    assert np.array_equal(both[:, 19:], a)


# ---- DeviceErase's draws -----------------------------------------------------------------------------------------------------
def test_boxes_are_strictly_inside_and_their_area_is_in_scale():
    er = trainer.DeviceErase(p=1.0, seed=1)
    for H, W in ((224, 224), (32, 48), (19, 70)):
        t, key = er.draw(512, H, W)
        hit = (t["h"] > 0) & (t["w"] > 0)
        assert hit.mean() > 0.9
        t = t[hit]
        assert (t["h"] < H).all() and (t["w"] < W).all() and (t["y"] >= 0).all() and (t["x"] >= 0).all()
        assert (t["y"] + t["h"] <= H).all() and (t["x"] + t["w"] <= W).all()
        # h = round(sqrt(area aspect)), w = round(sqrt(area / aspect)): each side is within half a pixel of its real value
        h, w = t["h"].astype(np.float64), t["w"].astype(np.float64)
        lo, hi = (h - 0.5) * (w - 0.5) / (H * W), (h + 0.5) * (w + 0.5) / (H * W)
        assert (hi >= er.scale[0]).all() and (lo <= er.scale[1]).all()
        ratio = h / w
        assert ((h + 0.5) / (w - 0.5) >= er.ratio[0]).all() and ((h - 0.5) / (w + 0.5) <= er.ratio[1]).all(), ratio
        trainer.DeviceErase.check(t, H, W)
        assert 0 <= key[0] < 2 ** 64 and 0 <= key[1] < 2 ** 64 and key[0] == er.seed


def test_probability_frequency_and_the_ten_attempts():
    none, _ = trainer.DeviceErase(p=0.0, seed=2).draw(64, 224, 224)
    assert not none["h"].any() and not none["w"].any()
    assert np.array_equal(none, trainer.DeviceErase.identity(64))
    every, _ = trainer.DeviceErase(p=1.0, seed=2).draw(256, 224, 224)
    assert ((every["h"] > 0) & (every["w"] > 0)).all()
    n, p = 4096, 0.25
    t, _ = trainer.DeviceErase(p=p, seed=3).draw(n, 224, 224)
    count = int(((t["h"] > 0) & (t["w"] > 0)).sum())
    assert abs(count - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p)), count
    # a 3 x 3 window cannot hold 90 % of its area in a box with h < 3 and w < 3: ten attempts, then not erased
    small, _ = trainer.DeviceErase(p=1.0, scale=(0.9, 1.0), seed=4).draw(32, 3, 3)
    assert np.array_equal(small, trainer.DeviceErase.identity(32))


def test_same_seed_same_tables_and_one_offset_per_batch():
    a, b = trainer.DeviceErase(p=0.5, seed=9), trainer.DeviceErase(p=0.5, seed=9)
    offsets = []
    for _ in range(4):
        (ta, ka), (tb, kb) = a.draw(16, 64, 64), b.draw(16, 64, 64)
        assert np.array_equal(ta, tb) and ka == kb
        offsets.append(ka[1])
    assert len(set(offsets)) == 4 and a.seed == b.seed
    assert trainer.DeviceErase(p=0.5, seed=10).seed != a.seed
    assert trainer.DeviceErase(value=0.5).value == (0.5, 0.5, 0.5) and trainer.DeviceErase(value=(1, 2, 3)).value == (1.0, 2.0, 3.0)
    assert trainer.DeviceErase().value is None
    for bad in (dict(p=1.5), dict(scale=(0.5, 0.2)), dict(ratio=(0.0, 1.0)), dict(value="mean"), dict(value=(1.0, 2.0))):
        with pytest.raises(ValueError):
            trainer.DeviceErase(**bad)
    assert "not claimed" in trainer.DeviceErase.__doc__


def test_check_refuses_boxes_outside_the_window_and_negative_fields():
    ok = EE.boxes_of([(0, 0, 19, 70), (18, 69, 1, 1), (0, 0, 0, 0)])
    trainer.DeviceErase.check(ok, 19, 70)
    for rec in ((0, 0, 20, 1), (0, 0, 1, 71), (18, 0, 2, 1), (0, 69, 1, 2), (-1, 0, 1, 1), (0, -1, 1, 1), (0, 0, -1, 1),
                (0, 0, 1, -1), (2 ** 31 - 1, 0, 2, 1)):
        with pytest.raises(ValueError):
            trainer.DeviceErase.check(EE.boxes_of([(0, 0, 0, 0), rec]), 19, 70)
    packed = trainer.DeviceErase.pack(ok, device="cpu")
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (3, 16)
    assert np.array_equal(np.frombuffer(packed.numpy().tobytes(), dtype=trainer.DeviceErase.dtype()), ok)


_AUG_FIELDS = ("order", "brightness", "contrast", "saturation", "hue", "solarize_thr", "blur_sigma")


class _Recorder:
    """Stands where the backend stands and keeps what DeviceCollate decided (tests/test_augment_cpu.py's, with the erase
    entry point)."""

    def __init__(self):
        self.calls, self.erase_calls = [], []

    def collate_crop_mix(self, img_u8, crop_yx, flip, out, mode, lam, box, mean, std, tokens=False):
        self.calls.append(("plain", mode, lam, box, crop_yx.tolist(), flip.tolist(), None))
        out.zero_()

    def augment_collate(self, img_u8, samples, gray_mean, out, mode, lam, box, mean, std, tokens=False):
        rec = np.frombuffer(samples.numpy().tobytes(), dtype=trainer.DeviceAugment.dtype())
        corners = np.stack([rec["y0"], rec["x0"]], axis=1).tolist()
        fields = tuple(rec[f].tolist() for f in _AUG_FIELDS)
        self.calls.append(("plain", mode, lam, box, corners, (rec["flags"] & 1).tolist(), fields))
        out.zero_()

    def augment_collate_erase(self, img_u8, samples, gray_mean, out, mode, lam, box, mean, std, boxes, value, key, tokens=False):
        self.erase_calls.append((np.frombuffer(boxes.numpy().tobytes(), dtype=trainer.DeviceErase.dtype()).copy(), value, key))
        self.augment_collate(img_u8, samples, gray_mean, out, mode, lam, box, mean, std, tokens=tokens)


def test_collate_and_augment_draws_do_not_shift_with_an_erase_object():
    u8 = torch.zeros(6, 3, 20, 24, dtype=torch.uint8)
    labels = torch.arange(6)
    for with_aug in (True, False):
        runs = []
        for er in (None, trainer.DeviceErase(p=0.5, seed=77)):
            col, rec = trainer.DeviceCollate(num_classes=10, seed=2006), _Recorder()
            aug = trainer.DeviceAugment(seed=99) if with_aug else None
            ys = []
            with calm.backend.use_backend(rec):
                for _ in range(5):
                    _, y = col(u8, labels, crop=(16, 16), tokens=True, augment=aug, erase=er)
                    ys.append(y)
            runs.append((rec, ys))
        (plain, ys0), (erased, ys1) = runs
        if with_aug:
            assert plain.calls == erased.calls
        else:                                             # the identity table stands in: same decisions, corners and flips
            assert [c[:6] for c in plain.calls] == [c[:6] for c in erased.calls]
            ident = trainer.DeviceAugment.identity(6)
            assert all(c[6] == tuple(ident[f].tolist() for f in _AUG_FIELDS) for c in erased.calls)
        assert len(plain.calls) == 5 and not plain.erase_calls and len(erased.erase_calls) == 5
        assert all(torch.equal(a, b) for a, b in zip(ys0, ys1))
        want = trainer.DeviceErase(p=0.5, seed=77)
        for boxes, value, key in erased.erase_calls:      # the erase object's own stream, nothing else drawn from it
            t, k = want.draw(6, 16, 16)
            assert np.array_equal(boxes, t) and key == k and value is None
    # a table given instead of drawn is checked before it reaches the kernel
    col, rec = trainer.DeviceCollate(num_classes=10, seed=1), _Recorder()
    with calm.backend.use_backend(rec):
        with pytest.raises(ValueError):
            col(u8, labels, crop=(16, 16), erase_table=(EE.boxes_of([(0, 0, 17, 1)] * 6), (1, 2)))
        with pytest.raises(ValueError):
            col(u8, labels, crop=(16, 16), erase_table=(EE.boxes_of([(0, 0, 1, 1)] * 5), (1, 2)))
        col(u8, labels, crop=(16, 16), erase_table=(EE.boxes_of([(0, 0, 16, 16)] * 6), (1, 2)),
            erase=trainer.DeviceErase(value=(0.5, 0.25, 0.0)))
    assert len(rec.erase_calls) == 1 and rec.erase_calls[0][1:] == ((0.5, 0.25, 0.0), (1, 2))


# ---- the C boundary -------------------------------------------------------------------------------------------------------
def test_erase_box_layout_matches_the_header():
    fields = ("y", "x", "h", "w")
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "calm_vit.h"\nint main(void){printf("%zu", sizeof(calm_erase_box));\n' + \
          "".join(f'printf(" %zu", offsetof(calm_erase_box, {f}));\n' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == 16 == ctypes.sizeof(binding.EraseBox) == trainer.DeviceErase.dtype().itemsize
    assert got[1:] == [getattr(binding.EraseBox, f).offset for f in fields]
    assert got[1:] == [trainer.DeviceErase.dtype().fields[f][1] for f in fields]


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "calm_vit.h")).read()
    assert "int calm_augment_collate_erase(" in header and "#define CALM_ABI_VERSION 7" in header.replace("  ", " ")
    lib = binding.load()
    assert lib.calm_abi_version() == 7
    fn = lib.calm_augment_collate_erase
    restype, argtypes = binding.SIGNATURES["calm_augment_collate_erase"]
    assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert argtypes[:15] == binding.SIGNATURES["calm_augment_collate"][1][:15]  # calm_augment_collate's up to std, then
    assert argtypes[15:] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    assert hasattr(calm.backend.HipBackend, "augment_collate_erase")


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Everything calm_augment_collate refuses, a null boxes_dev, a value_mode outside {0, 1} and a null value in mode 0:
    every call below is turned down before a launch, so the fake addresses are never read."""
    lib = binding.load()
    P = 0x7f0000010000
    mean, std, box = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.25, 0.25, 0.25), (ctypes.c_int32 * 4)(0, 1, 0, 1)
    value = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    valid = [P, 40, 36, P, P, P, 2, 32, 32, 1, 2, 0.5, box, mean, std, P, 0, value, 1, 2, None]
    assert len(valid) == len(binding.SIGNATURES["calm_augment_collate_erase"][1])
    for i in (0, 3, 4, 5, 12, 13, 14, 15, 17):              # img, samples, gray_mean, out, box (CutMix), mean, std, boxes, value
        args = list(valid)
        args[i] = None
        assert lib.calm_augment_collate_erase(*args) == binding.E_INVAL, i
    for change in ({6: 0}, {7: 0}, {8: -1}, {7: 41}, {8: 37}, {10: 3}, {10: -1}, {16: 2}, {16: -1}, {16: 1, 15: None}):
        args = list(valid)
        for i, v in change.items():
            args[i] = v
        assert lib.calm_augment_collate_erase(*args) == binding.E_INVAL, change
    args = list(valid)
    args[6] = 65536
    assert lib.calm_augment_collate_erase(*args) == binding.E_UNSUPP


# ---- label smoothing --------------------------------------------------------------------------------------------------------
class _TinySet(torch.utils.data.Dataset):
    def __init__(self, n=8):
        g = torch.Generator().manual_seed(7)
        self.x = torch.randn(n, 3, 32, 32, generator=g)
        self.y = torch.randint(0, 10, (n,), generator=g)

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return self.x[i], int(self.y[i])


def _onehot_collate(batch):
    """An unmixed collate: the images stacked, the labels as one-hot probabilities."""
    x = torch.stack([b[0] for b in batch])
    return x, torch.nn.functional.one_hot(torch.tensor([b[1] for b in batch]), 10).to(torch.float32)


class _Noise:
    """The latent noise as a function of the call count alone, so that two runs draw the same."""

    def __init__(self):
        self.n = 0

    def __call__(self, like):
        self.n += 1
        return torch.randn(like.shape, generator=torch.Generator().manual_seed(1000 + self.n), dtype=like.dtype)


def _train(record=None, epochs=2, **kw):
    torch.manual_seed(50)
    m = build_model("tiny32_cls", None).train()
    real = trainer.soft_target_cross_entropy

    def spy(logits, targets, metrics=None):
        loss = real(logits, targets, metrics)
        record.append((targets.detach().clone(), float(loss.detach().double())))
        return loss

    calm.ops.set_noise_override(_Noise())
    if record is not None:
        trainer.soft_target_cross_entropy = spy
    try:
        with calm.backend.use_backend(EmulatedBackend()):
            return trainer.train(m, trainer.make_optimizer(m), scheduler=False, use_gpu=False, dataset=_TinySet(), epochs=epochs,
                                 batch_size=4, num_classes=10, collate_fn=_onehot_collate, num_workers=0, log_every=1000, **kw)
    finally:
        trainer.soft_target_cross_entropy = real
        calm.ops.set_noise_override(None)


@pytest.mark.timeout(600)
def test_label_smoothing_equals_torch_cross_entropy_with_label_smoothing():
    """train(label_smoothing=0.1) on one gloo rank against the hand-written loop of cls:79-96 with
    torch.nn.CrossEntropyLoss(label_smoothing=0.1) on the one-hot-as-probabilities targets: the same formula summed in
    another order in fp32, 1e-6 relative per step; the targets that reach the step are y (1 - eps) + eps / K."""
    eps, K = 0.1, 10
    seen = []
    _train(seen, label_smoothing=eps)
    data = _TinySet()
    torch.manual_seed(50)
    m = build_model("tiny32_cls", None).train()
    opt = trainer.make_optimizer(m)
    ce = torch.nn.CrossEntropyLoss(label_smoothing=eps)
    calm.ops.set_noise_override(_Noise())
    losses, targets = [], []
    try:
        with calm.backend.use_backend(EmulatedBackend()):
            for epoch in range(2):
                order = torch.randperm(len(data), generator=torch.Generator().manual_seed(2006 + epoch)).tolist()
                for i in range(0, len(order), 4):
                    x, y = _onehot_collate([data[j] for j in order[i:i + 4]])
                    y_hat, _ = m(x)
                    loss = ce(y_hat.squeeze(), y)
                    loss.backward()
                    torch.nn.utils.clip_grad_norm_([p for p in m.parameters() if p.requires_grad], max_norm=1.0)
                    opt.step()
                    opt.zero_grad()
                    losses.append(float(loss.detach().double()))
                    targets.append(y)
    finally:
        calm.ops.set_noise_override(None)
    assert len(seen) == len(losses) == 4
    for (got_y, got_loss), y, loss in zip(seen, targets, losses):
        want_y = y.double() * (1.0 - eps) + eps / K
        assert (got_y.double() - want_y).abs().max().item() <= 1e-7       # one fp32 rounding of values <= 1
        assert abs(got_y.sum(1) - 1.0).max().item() <= 1e-6 and torch.equal(got_y.argmax(1), y.argmax(1))
        print(f"label smoothing: train() {got_loss:.9f}, torch loop {loss:.9f}")
        assert abs(got_loss - loss) <= 1e-6 * abs(loss), (got_loss, loss)
    assert not torch.distributed.is_initialized()


@pytest.mark.timeout(600)
def test_label_smoothing_zero_is_the_run_without_the_argument():
    seen_a, seen_b = [], []
    a, b = _train(seen_a, epochs=1), _train(seen_b, epochs=1, label_smoothing=0.0)
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert all(torch.equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(seen_a, seen_b)) and len(seen_a) == 2
    assert set(seen_a[0][0].unique().tolist()) == {0.0, 1.0}             # unsmoothed: the one-hot targets as they came
    inp = trainer._TrainInput(False, False, None, None, None, None, _onehot_collate, 10, 0, False, torch.device("cpu"))
    assert inp._smooth is None and inp.generators(0) == {}


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_process_group():
    data = torch.utils.data.TensorDataset(torch.zeros(4, 3, 32, 32, dtype=torch.uint8), torch.randint(0, 10, (4,)))
    lin = torch.nn.Linear(4, 4)
    sgd = torch.optim.SGD(lin.parameters(), lr=0.1)
    kw = dict(use_gpu=False, dataset=data, epochs=1, batch_size=2, num_classes=10)
    with pytest.raises(ValueError, match="random_erasing needs device_collate=True"):
        trainer.train(lin, sgd, random_erasing=0.25, **kw)
    with pytest.raises(ValueError, match="random_erasing needs device_collate=True"):
        trainer.train(lin, "fused", random_erasing=trainer.DeviceErase(), **dict(kw, use_gpu=True))
    gpu = dict(kw, use_gpu=True, device_collate=True)
    with pytest.raises(ValueError, match='random_erasing excludes task="reg"'):
        trainer.train(lin, "fused", random_erasing=0.25, task="reg", **gpu)
    with pytest.raises(ValueError, match='"p", "scale", "ratio", "value", "seed"'):
        trainer.train(lin, "fused", random_erasing={"prob": 0.25}, **gpu)
    with pytest.raises(ValueError, match="DeviceErase: p is a probability"):
        trainer.train(lin, "fused", random_erasing=1.5, **gpu)
    with pytest.raises(ValueError, match="random_erasing is a probability, a dict"):
        trainer.train(lin, "fused", random_erasing="on", **gpu)
    for bad in (1.0, -0.1, 1.5, "0.1", True):
        with pytest.raises(ValueError, match=r"label_smoothing is an epsilon in \[0, 1\)"):
            trainer.train(lin, sgd, label_smoothing=bad, **kw)
    with pytest.raises(ValueError, match='label_smoothing excludes task="reg"'):
        trainer.train(lin, sgd, label_smoothing=0.1, task="reg", **kw)
    assert not torch.distributed.is_initialized()
    # the generator joins the snapshot's set, so a file written without it is refused by TrainState.load
    inp = trainer._TrainInput(True, True, None, None, None, (32, 32), "mix", 10, 3, False, torch.device("cpu"), random_erasing={"p": 0.5})
    assert set(inp.generators(0)) == {"collate", "augment", "erase"} and inp.erase.p == 0.5
    assert inp.erase.seed == trainer.DeviceErase(seed=2006 + 3).seed     # seeded 2006 + rank when built there
    own = trainer.DeviceErase(seed=1)
    assert trainer._TrainInput(True, False, None, None, None, None, "mix", 10, 0, False, torch.device("cpu"),
                               random_erasing=own).erase is own
