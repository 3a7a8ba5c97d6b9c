"""Device-side photometric augmentation without a GPU: the float64 emulation the kernel is tested against
(tests/emulated_augment.py) against PIL, colorsys and scipy, operation by operation; the host logic of
trainer.DeviceAugment (ranges, orders, frequencies, seeding, DeviceCollate's draws untouched); the argument checks of
train(device_augment=True) and of calm_augment_collate; the layout of struct calm_aug_sample.

The reference applies these operations to 8-bit PIL images (distributed_trainer_cls.py:131-135) and rounds after each one;
the device path keeps float on [0, 1] throughout.  The bounds below are that difference per operation, in 8-bit levels:
  brightness / contrast / saturation  <= 1.5   PIL blends the image with a degenerate image that is itself rounded to 8 bits
                                                (<= 0.5 level, times |1 - f|) and truncates the result (< 1 level)
  gray vs convert("L")                <= 0.52  PIL's 16-bit fixed-point weights differ from 0.2989 / 0.587 / 0.114 by
                                                < 2e-5 each, plus its rounding to a level (0.5)
  solarize                            exact on uint8 input (the threshold 223.5 / 255 lies between two levels)"""
import colorsys
import ctypes
import os
import subprocess
import sys
import tempfile
from importlib import import_module

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import calm_vit_dte_amd as calm  # noqa: E402,F401
import emulated_augment as EA  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")


def _u8(seed=0, H=40, W=40):
    return np.random.default_rng(seed).integers(0, 256, (3, H, W), dtype=np.uint8)


def _pil(u8):
    Image = pytest.importorskip("PIL.Image")
    return Image.fromarray(np.ascontiguousarray(u8.transpose(1, 2, 0)), "RGB")


def _levels(im):
    a = np.asarray(im, dtype=np.float64)
    return a.transpose(2, 0, 1) if a.ndim == 3 else a


@pytest.mark.parametrize("f", [0.5, 0.6180339887, 0.75, 0.9, 1.0])
def test_brightness_contrast_saturation_within_a_level_and_a_half_of_pil(f):
    ImageEnhance = pytest.importorskip("PIL.ImageEnhance")
    u8 = _u8(1)
    x = u8 / 255.0
    for name, op, enh in (("brightness", EA.brightness, ImageEnhance.Brightness), ("contrast", EA.contrast, ImageEnhance.Contrast),
                          ("saturation", EA.saturation, ImageEnhance.Color)):
        d = np.abs(op(x, f) * 255.0 - _levels(enh(_pil(u8)).enhance(f))).max()
        print(f"{name} f={f}: max |emulation - PIL| = {d:.3f} levels")
        assert d <= 1.5, (name, f, d)


def test_solarize_equals_pil_exactly_on_uint8_input():
    ImageOps = pytest.importorskip("PIL.ImageOps")
    u8 = np.arange(3 * 16 * 16, dtype=np.int64).reshape(3, 16, 16) % 256          # every level, in every channel
    u8 = u8.astype(np.uint8)
    thr = float(np.float32(223.5 / 255.0))                                        # what DeviceAugment passes, as the kernel sees it
    got = EA.solarize(u8 / 255.0, thr) * 255.0
    want = _levels(ImageOps.solarize(_pil(u8), 224))
    assert np.array_equal(np.rint(got), want) and np.abs(got - want).max() < 1e-9
    assert not (np.abs(u8 / 255.0 - thr) <= EA.NEAR).any()                        # no 8-bit level is near the threshold


def test_gray_within_half_a_level_of_pil_luma():
    u8 = _u8(2)
    d = np.abs(EA.gray(u8 / 255.0) * 255.0 - _levels(_pil(u8).convert("L"))).max()
    print(f"gray: max |emulation - PIL L| = {d:.3f} levels")
    assert d <= 0.52
    g = EA.grayscale(u8 / 255.0)
    assert np.array_equal(g[0], g[1]) and np.array_equal(g[1], g[2]) and np.array_equal(g[0], EA.gray(u8 / 255.0))


@pytest.mark.parametrize("f", [-0.125, -0.03, 0.0, 0.07, 0.125])
def test_hue_equals_colorsys(f):
    x = _u8(3) / 255.0
    x[:, 0, :8] = x[0, 0, :8]                                 # flat pixels (s = 0) and pixels with two equal channels
    x[1, 1, :8] = x[0, 1, :8]
    x[2, 2, :8] = x[1, 2, :8]
    got = EA.hue(x, f)
    want = np.empty_like(x)
    for i in range(x.shape[1]):
        for j in range(x.shape[2]):
            h, s, v = colorsys.rgb_to_hsv(*x[:, i, j])
            want[:, i, j] = colorsys.hsv_to_rgb((h + f) % 1.0, s, v)
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("sigma", [0.1, 0.8, 2.0])
def test_blur_equals_scipy_mirror_correlation(sigma):
    ndimage = pytest.importorskip("scipy.ndimage")
    x = _u8(4, 23, 31) / 255.0
    w = EA.blur_weights(sigma)
    assert abs(w.sum() - 1.0) < 1e-15 and w[0] == w[2]
    want = ndimage.correlate1d(ndimage.correlate1d(x, w, axis=2, mode="mirror"), w, axis=1, mode="mirror")
    assert np.abs(EA.blur(x, sigma) - want).max() <= 1e-12
    two = np.abs(EA.blur(x[:, :2, :2], sigma) - ndimage.correlate1d(ndimage.correlate1d(x[:, :2, :2], w, axis=2, mode="mirror"),
                                                                    w, axis=1, mode="mirror")).max()
    assert two <= 1e-12                                       # the smallest window the blur takes


def test_emulated_collate_order_partner_and_layout():
    """The whole-sample emulation: contrast takes its mean after the operations in front of it, flip comes after
    solarize and before the blur, the partner is the batch rolled by one with its own parameters, tokens are the
    channels-last image, and an identity table is the plain collate."""
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, (3, 3, 12, 14), dtype=np.uint8)
    t = trainer.DeviceAugment.identity(3)
    mean, std = trainer.DeviceCollate.MEAN, trainer.DeviceCollate.STD
    t["y0"], t["x0"] = [0, 2, 1], [3, 0, 4]
    out, gm, near = EA.augment_collate(src, t, 10, 9, 0, 1.0, None, mean, std)
    m, s = np.asarray(mean)[:, None, None], np.asarray(std)[:, None, None]
    for b in range(3):
        win = src[b, :, t["y0"][b]:t["y0"][b] + 10, t["x0"][b]:t["x0"][b] + 9] / 255.0
        assert np.array_equal(out[b], (win - m) / s)
    assert not near.any() and not gm.any()
    t["order"][1] = [binding.AUG_OP_BRIGHTNESS, binding.AUG_OP_CONTRAST, 255, 255]
    t["brightness"][1], t["contrast"][1] = 0.5, 0.75
    t["flags"][1] = binding.AUG_FLIP
    out, gm, _ = EA.augment_collate(src, t, 10, 9, 1, 0.25, None, mean, std, tokens=True)
    win = src[1, :, 2:12, 0:9] / 255.0 * 0.5
    assert abs(gm[1] - EA.gray(win).mean()) < 1e-15 and gm[0] == 0.0
    s1 = ((np.clip(0.75 * win + 0.25 * EA.gray(win).mean(), 0, 1))[:, :, ::-1] - m) / s
    s2 = (src[2, :, 1:11, 4:13] / 255.0 - m) / s
    want = s2 * 0.25 + s1 * 0.75                             # sample 2's partner is sample 1
    assert np.abs(out[2] - want.transpose(1, 2, 0).reshape(10, 27)).max() < 1e-15


# ---- DeviceAugment ------------------------------------------------------------------------------------------------------
def test_draw_ranges_orders_frequencies_and_seeding():
    aug = trainer.DeviceAugment(seed=11)
    n = 10000
    t = aug.draw(n)
    assert t.dtype.itemsize == 48 and len(t) == n
    for name, (lo, hi) in (("brightness", (0.5, 1)), ("contrast", (0.5, 1)), ("saturation", (0.5, 1)), ("hue", (-0.125, 0.125)),
                           ("blur_sigma", (0.1, 2.0))):
        v = t[name].astype(np.float64)
        assert v.min() >= np.float32(lo) and v.max() <= np.float32(hi), name
        assert abs(v.mean() - (lo + hi) / 2) < 0.02 * (hi - lo), name                  # uniform: sd of the mean is 0.003 (hi - lo)
    assert (np.sort(t["order"], axis=1) == np.arange(4)).all()                          # every order is a permutation
    seen = {tuple(o) for o in t["order"]}
    assert len(seen) == 24                                                              # ... and every permutation occurs
    first = np.bincount(t["order"][:, 0], minlength=4) / n
    assert np.abs(first - 0.25).max() < 0.02                                            # sd 0.0043
    fl = t["flags"]
    assert abs((fl & binding.AUG_SOLARIZE != 0).mean() - 0.5) < 0.02                    # sd 0.005
    assert abs((fl & binding.AUG_GRAYSCALE != 0).mean() - 0.1) < 0.012                  # sd 0.003
    assert (fl & binding.AUG_BLUR != 0).all() and not (fl & binding.AUG_FLIP).any()
    assert (t["solarize_thr"] == np.float32(223.5 / 255.0)).all()
    again = trainer.DeviceAugment(seed=11).draw(n)
    assert t.tobytes() == again.tobytes()
    assert trainer.DeviceAugment(seed=12).draw(n).tobytes() != t.tobytes()
    off = trainer.DeviceAugment(seed=1, hue=None, contrast=None, blur_sigma=None, solarize_p=0.0, grayscale_p=0.0).draw(64)
    assert (np.sort(off["order"], axis=1) == [0, 2, 255, 255]).all() and (off["order"][:, 2:] == 255).all()
    assert not off["flags"].any()


def test_pack_fills_corners_and_flips_into_the_records():
    t = trainer.DeviceAugment(seed=3).draw(5)
    corners = np.array([[0, 1], [2, 3], [4, 5], [6, 7], [8, 9]])
    flips = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8)
    dev = trainer.DeviceAugment.pack(t, corners, flips, device="cpu")
    assert dev.dtype == torch.uint8 and tuple(dev.shape) == (5, 48) and dev.is_contiguous()
    back = np.frombuffer(dev.numpy().tobytes(), dtype=trainer.DeviceAugment.dtype())
    assert (back["y0"] == corners[:, 0]).all() and (back["x0"] == corners[:, 1]).all()
    assert ((back["flags"] & binding.AUG_FLIP) != 0).tolist() == [True, False, True, True, False]
    assert ((back["flags"] & ~np.uint32(1)) == t["flags"]).all() and not (t["flags"] & 1).any()      # the table is not modified
    for name in ("order", "brightness", "contrast", "saturation", "hue", "solarize_thr", "blur_sigma"):
        assert np.array_equal(back[name], t[name]), name
    rec = binding.AugSample.from_buffer_copy(dev[1].numpy().tobytes())                  # the ctypes mirror reads the same record
    assert (rec.y0, rec.x0, rec.flags, list(rec.order)) == (2, 3, int(back["flags"][1]), list(t["order"][1]))
    assert rec.blur_sigma == t["blur_sigma"][1] and rec.hue == t["hue"][1]
    with pytest.raises(ValueError):
        trainer.DeviceAugment.check_window(t, 1, 8)
    trainer.DeviceAugment.check_window(trainer.DeviceAugment.identity(2), 1, 1)


class _Recorder:
    """Stands where the backend stands and keeps what DeviceCollate decided."""

    def __init__(self):
        self.calls = []

    def collate_crop_mix(self, img_u8, crop_yx, flip, out, mode, lam, box, mean, std, tokens=False):
        self.calls.append(("plain", mode, lam, box, crop_yx.tolist(), flip.tolist()))
        out.zero_()

    def augment_collate(self, img_u8, samples, gray_mean, out, mode, lam, box, mean, std, tokens=False):
        rec = np.frombuffer(samples.numpy().tobytes(), dtype=trainer.DeviceAugment.dtype())
        corners = np.stack([rec["y0"], rec["x0"]], axis=1).tolist()
        self.calls.append(("plain", mode, lam, box, corners, (rec["flags"] & 1).tolist()))
        out.zero_()


def test_device_collate_draws_do_not_shift_with_an_augment_object():
    u8 = torch.zeros(6, 3, 20, 24, dtype=torch.uint8)
    labels = torch.arange(6)
    runs = []
    for aug in (None, trainer.DeviceAugment(seed=99)):
        col, rec = trainer.DeviceCollate(num_classes=10, seed=2006), _Recorder()
        ys = []
        with calm.backend.use_backend(rec):
            for _ in range(5):
                _, y = col(u8, labels, crop=(16, 16), tokens=True, augment=aug)
                ys.append(y)
        runs.append((rec.calls, ys))
    assert runs[0][0] == runs[1][0] and len(runs[0][0]) == 5
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert len({c[1] for c in runs[0][0]} | {2, 1}) == 2 and len({str(c[4]) for c in runs[0][0]}) == 5


def test_train_refuses_device_augment_without_device_collate_or_on_a_cpu_run():
    data = torch.utils.data.TensorDataset(torch.zeros(4, 3, 32, 32, dtype=torch.uint8), torch.randint(0, 10, (4,)))
    for kw in (dict(device_augment=True), dict(device_augment=True, device_collate=True)):
        with pytest.raises(ValueError):
            trainer.train(torch.nn.Linear(4, 4), torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1), use_gpu=False,
                          dataset=data, epochs=1, batch_size=2, num_classes=10, destroy_process_group=True, **kw)
    with pytest.raises(ValueError):                        # without device_collate it is refused on a GPU run as well
        trainer.train(torch.nn.Linear(4, 4), "fused", use_gpu=True, dataset=data, epochs=1, batch_size=2, num_classes=10,
                      device_augment=True)
    assert not torch.distributed.is_initialized()


# ---- the C boundary ---------------------------------------------------------------------------------------------------
def test_aug_sample_layout_matches_the_header():
    fields = ("y0", "x0", "flags", "order", "brightness", "contrast", "saturation", "hue", "solarize_thr", "blur_sigma", "reserved")
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "calm_vit.h"\nint main(void){printf("%zu", sizeof(calm_aug_sample));\n' + \
          "".join(f'printf(" %zu", offsetof(calm_aug_sample, {f}));\n' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == 48 == ctypes.sizeof(binding.AugSample) == trainer.DeviceAugment.dtype().itemsize
    assert got[1:] == [getattr(binding.AugSample, f).offset for f in fields]
    assert got[1:] == [trainer.DeviceAugment.dtype().fields[f][1] for f in fields]
    assert (binding.AUG_FLIP, binding.AUG_SOLARIZE, binding.AUG_GRAYSCALE, binding.AUG_BLUR) == (EA.FLIP, EA.SOLARIZE, EA.GRAYSCALE, EA.BLUR)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """calm_augment_collate's argument checks (those of calm_collate_crop_mix, and a null samples_dev / gray_mean) on a
    host without a GPU: every call below is turned down before a launch, so the fake addresses are never read."""
    lib = binding.load()
    P = 0x7f0000010000
    mean, std, box = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.25, 0.25, 0.25), (ctypes.c_int32 * 4)(0, 1, 0, 1)
    valid = [P, 40, 36, P, P, P, 2, 32, 32, 1, 2, 0.5, box, mean, std, None]
    assert len(valid) == len(binding.SIGNATURES["calm_augment_collate"][1])
    for i in (0, 3, 4, 5, 12, 13, 14):                       # img, samples, gray_mean, out, box (CutMix), mean, std
        args = list(valid)
        args[i] = None
        assert lib.calm_augment_collate(*args) == binding.E_INVAL, i
    for change in ({6: 0}, {7: 0}, {8: -1}, {7: 41}, {8: 37}, {10: 3}, {10: -1}):
        args = list(valid)
        for i, v in change.items():
            args[i] = v
        assert lib.calm_augment_collate(*args) == binding.E_INVAL, change
    args = list(valid)
    args[6] = 65536
    assert lib.calm_augment_collate(*args) == binding.E_UNSUPP
