"""Device RandAugment without a GPU: the numpy emulation the kernel is tested against (tests/emulated_randaug.py) against
PIL, byte for byte; the draws, tables and refusals of trainer.DeviceRandAugment; the C boundary of calm_randaugment_u8;
and train(rand_augment=) on one and two gloo ranks on the emulated backend.

train(device_collate=True) is refused without a GPU (the collate is a HIP kernel), so the gloo runs here hand
`_check_train_args` use_gpu=True and the job itself use_gpu=False: every refusal is still made, and the input pipeline then
runs on the host through an emulated backend that computes the stage with the numpy emulation."""
import ctypes
import math
import os
import socket
import subprocess
import sys
import tempfile
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import calm_vit_dte_amd as calm  # noqa: E402
import emulated_randaug as R  # noqa: E402
from emulated_backend import EmulatedBackend  # noqa: E402
from test_host_logic_cpu import build_model  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
DRA = trainer.DeviceRandAugment
KINDS = ("noise", "ramp", "constant", "two_level")


# ---- PIL: what torchvision's RandAugment calls for each operation -----------------------------------------------------------
def to_pil(x):
    return Image.fromarray(np.ascontiguousarray(x.transpose(1, 2, 0)))


def from_pil(im):
    return np.ascontiguousarray(np.asarray(im).transpose(2, 0, 1))


def pil_op(im, name, value, fill):
    W, H = im.size
    warp = lambda a: im.transform((W, H), Image.AFFINE, a, Image.NEAREST, fillcolor=fill)
    if name == "Identity":
        return im
    if name == "ShearX":
        return warp((1.0, value, 0.0, 0.0, 1.0, 0.0))
    if name == "ShearY":
        return warp((1.0, 0.0, 0.0, value, 1.0, 0.0))
    if name == "TranslateX":
        return warp((1.0, 0.0, -float(int(value)), 0.0, 1.0, 0.0))
    if name == "TranslateY":
        return warp((1.0, 0.0, 0.0, 0.0, 1.0, -float(int(value))))
    if name == "Rotate":
        return im.rotate(value, Image.NEAREST, fillcolor=fill)
    if name in ("Brightness", "Color", "Contrast", "Sharpness"):
        return getattr(ImageEnhance, name)(im).enhance(1.0 + value)
    if name == "Posterize":
        return ImageOps.posterize(im, int(value)) if int(value) > 0 else Image.new("RGB", (W, H))     # (PIL refuses 0 bits)
    if name == "Solarize":
        return ImageOps.solarize(im, value)
    if name == "AutoContrast":
        return ImageOps.autocontrast(im)
    if name == "Equalize":
        return ImageOps.equalize(im)
    raise ValueError(name)


def values_of(name, H, W):
    """The signed magnitudes an operation is tried with: both signs, factors on both sides of 1, the ends of the ranges."""
    if name in ("Identity", "AutoContrast", "Equalize"):
        return (0.0,)
    if name in ("ShearX", "ShearY"):
        return (0.09, -0.3, 0.99, -0.47, 0.0)
    if name in ("TranslateX", "TranslateY"):
        side = W if name == "TranslateX" else H
        return (150.0 / 331.0 * side * 0.3, -150.0 / 331.0 * side, 32.0, -1.7, 0.0)
    if name == "Rotate":
        return (9.0, -30.0, 135.0, -71.3, 0.0, 3.3)                      # 0 and non-multiples of 90
    if name in ("Brightness", "Color", "Contrast", "Sharpness"):
        return (0.27, -0.27, 0.9, -0.9, 0.99, -0.99, 0.0)
    if name == "Posterize":
        return (7.0, 4.0, 2.0, 1.0, 8.0, 0.0)
    return (178.5, 255.0, 0.0, 1.0, 128.0)                               # Solarize


def emulated_op(x, name, value, fill):
    op, factor, param, coef = DRA.slot(name, value, *x.shape[1:])
    return R.apply_op(x, op, factor, param, coef, fill)


@pytest.mark.parametrize("window", R.WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
@pytest.mark.parametrize("name", DRA.OPS)
def test_every_operation_equals_pil(name, window):
    H, W = window
    for kind in KINDS:
        x = R.image(11, H, W, kind)
        im = to_pil(x)
        for value in values_of(name, H, W):
            for fill in ((0, 0, 0), R.FILL):
                got, want = emulated_op(x, name, value, fill), from_pil(pil_op(im, name, value, fill))
                assert got.tobytes() == want.tobytes(), (name, window, kind, value, fill, int((got != want).sum()))


def test_smooth_and_the_blend_outside_0_1_equal_pil():
    for H, W in R.WINDOWS + ((224, 224),):
        x = R.image(12, H, W)
        assert R.smooth(x).tobytes() == from_pil(to_pil(x).filter(ImageFilter.SMOOTH)).tobytes()
    a, b = R.image(13, 17, 33), R.image(14, 17, 33)
    for f in (-0.5, 0.0, 0.3, 1.0, 1.7, 2.5):
        assert R.blend(a, b, f).tobytes() == from_pil(Image.blend(to_pil(a), to_pil(b), f)).tobytes()


def test_histogram_edge_cases_equal_pil():
    """A constant channel; two levels; an image small enough for step = 0; at least 510 pixels; one non-empty bin."""
    cases = [R.image(20, 17, 33, "constant"), R.image(21, 17, 33, "two_level"), R.image(22, 7, 5, "noise"),
             R.image(23, 3, 3, "two_level"), R.image(24, 64, 48, "ramp"), R.image(25, 17, 30, "ramp"),
             np.full((3, 9, 9), 77, dtype=np.uint8)]
    assert cases[2][0].size < 255 and cases[5][0].size == 510 and cases[4][0].size >= 510
    for x in cases:
        im = to_pil(x)
        assert R.equalize(x).tobytes() == from_pil(ImageOps.equalize(im)).tobytes()
        assert R.autocontrast(x).tobytes() == from_pil(ImageOps.autocontrast(im)).tobytes()
        for f in (0.55, 1.45):
            assert R.contrast(x, f).tobytes() == from_pil(ImageEnhance.Contrast(im).enhance(float(np.float32(f)))).tobytes()
    assert (R.equalize(cases[2]) == cases[2]).all()                     # step = 0: unchanged
    assert (R.equalize(cases[4]) != cases[4]).any() and (R.autocontrast(cases[4]) != cases[4]).any()
    assert (R.autocontrast(cases[0])[1] == 93).all()                    # the constant channel stays


CHAINS = [[("Rotate", 17.0), ("Equalize", 0.0)], [("Contrast", 0.45), ("ShearX", -0.3)],
          [("Color", 0.9), ("Rotate", -29.5), ("Posterize", 4.0), ("AutoContrast", 0.0)],
          [("Sharpness", 0.81), ("Solarize", 128.0), ("TranslateY", 7.0), ("Contrast", -0.45)],
          [("Equalize", 0.0), ("Brightness", 0.63), ("ShearY", 0.17), ("Sharpness", -0.81)]]


@pytest.mark.parametrize("chain", CHAINS, ids=lambda c: "-".join(n for n, _ in c))
def test_chains_with_crop_and_flip_equal_the_pil_chain(chain):
    """randaugment() on a batch — crop from a larger source, flip, then the chain — against Image.crop + transpose + the
    same PIL calls."""
    Hs, Ws, H, W, n = 40, 52, 31, 37, 4
    src = R.batch(30, n, Hs, Ws, "ramp")
    corners = np.array([(0, 0), (Hs - H, Ws - W), (3, 11), (9, 2)])
    flips = np.array([0, 1, 1, 0])
    t = R.table_of([[DRA.slot(name, v, H, W) for name, v in chain]] * n, corners, flips)
    DRA.check(t, H, W)
    got = R.randaugment(src, t, H, W, R.FILL, *DRA.launch_plan(t))
    for b in range(n):
        (y0, x0) = corners[b]
        im = to_pil(src[b]).crop((x0, y0, x0 + W, y0 + H))
        if flips[b]:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        for name, v in chain:
            im = pil_op(im, name, v, R.FILL)
        assert got[b].tobytes() == from_pil(im).tobytes(), (b, chain)
    # a corner outside the source is clamped as calm_augment_collate clamps it
    t["y0"][0], t["x0"][0] = -7, 10 ** 6
    assert (R.randaugment(src[:1], t[:1], H, W, R.FILL)[0] == R.randaugment(src[:1], R.table_of([t_chain(t, 0)], [(0, Ws - W)], [0]),
                                                                           H, W, R.FILL)[0]).all()


def t_chain(t, b):
    return [(int(t["op"][b, k]), float(t["factor"][b, k]), int(t["param"][b, k]), tuple(int(v) for v in t["coef"][b, k]))
            for k in range(int(t["n_ops"][b]))]


def test_emulation_skips_what_the_contract_says_it_skips():
    x = R.batch(31, 2, 24, 24)           # (576 pixels: Equalize moves it)
    ops = R.every_op(24, 24)
    t = R.table_of([[ops["brightness+"], ops["equalize"]], [ops["posterize4"]]])
    full = R.randaugment(x, t, 24, 24)
    assert (R.randaugment(x, t, 24, 24, n_slots=1)[0] == R.brightness(x[0], 1.63)).all()
    assert (R.randaugment(x, t, 24, 24, stats_mask=0)[0] == R.brightness(x[0], 1.63)).all() and (full[0] != R.brightness(x[0], 1.63)).any()
    t["op"][1, 0], t["param"][1, 0] = 99, 0
    assert (R.randaugment(x, t, 24, 24)[1] == x[1]).all()
    t["op"][1, 0], t["param"][1, 0] = R.POSTERIZE, 12
    assert (R.randaugment(x, t, 24, 24)[1] == x[1]).all()                 # bits outside 0 .. 8: 8


# ---- DeviceRandAugment's tables and draws -----------------------------------------------------------------------------------
def test_magnitude_table_follows_the_formulas():
    ra = DRA(num_bins=31)
    i = np.arange(31)
    for name in ("ShearX", "ShearY"):
        assert np.array_equal(ra.magnitudes(name, 224, 200), np.linspace(0.0, 0.3, 31))
    assert np.array_equal(ra.magnitudes("TranslateX", 224, 200), np.linspace(0.0, 150.0 / 331.0 * 200, 31))
    assert np.array_equal(ra.magnitudes("TranslateY", 224, 200), np.linspace(0.0, 150.0 / 331.0 * 224, 31))
    assert np.array_equal(ra.magnitudes("Rotate", 224, 200), np.linspace(0.0, 30.0, 31))
    for name in ("Brightness", "Color", "Contrast", "Sharpness"):
        assert np.array_equal(ra.magnitudes(name, 224, 200), np.linspace(0.0, 0.9, 31))
    assert np.array_equal(ra.magnitudes("Posterize", 224, 200), 8 - np.round(i / (30 / 4)))
    assert ra.magnitudes("Posterize", 1, 1).tolist()[::6] == [8.0, 7.0, 6.0, 6.0, 5.0, 4.0]
    assert np.array_equal(ra.magnitudes("Solarize", 224, 200), np.linspace(255.0, 0.0, 31))
    assert all(ra.magnitudes(n, 8, 8) is None for n in ("Identity", "AutoContrast", "Equalize"))
    wide = DRA.trivial_wide()
    assert wide.num_ops == 1 and wide.wide
    assert wide.magnitudes("ShearX", 8, 8)[-1] == 0.99 and wide.magnitudes("TranslateY", 224, 224)[-1] == 32.0
    assert wide.magnitudes("Rotate", 8, 8)[-1] == 135.0 and wide.magnitudes("Color", 8, 8)[-1] == 0.99
    assert np.array_equal(wide.magnitudes("Posterize", 8, 8), 8 - np.round(i / (30 / 6)))
    # bin 9 of 31 at 224 x 224: the records
    H = W = 224
    assert DRA.slot("ShearX", 0.09, H, W) == (binding.RA_OP_AFFINE, 1.0, 0, R.fixed_coeffs(R.shear_x(0.09)))
    assert DRA.slot("TranslateX", -30.45, H, W)[3] == R.fixed_coeffs(R.translate_x(-30))
    assert DRA.slot("Rotate", -9.0, H, W)[3] == R.fixed_coeffs(R.rotate(-9.0, H, W))
    assert DRA.slot("Color", -0.27, H, W)[:3] == (binding.RA_OP_COLOR, float(np.float32(0.73)), 0)
    assert DRA.slot("Posterize", 7.0, H, W)[:3] == (binding.RA_OP_POSTERIZE, 1.0, 7)
    assert DRA.slot("Solarize", 178.5, H, W)[:3] == (binding.RA_OP_SOLARIZE, 1.0, 179)      # i < 178.5 is i < 179
    assert DRA.fixed_coeffs((1, 0, 0, 0, 1, 0)) == (65536, 0, 32768, 0, 65536, 32768) == R.IDENT_COEF


def test_draws_use_the_magnitude_bin_and_a_fair_sign():
    n = 4096
    t = DRA(num_ops=1, ops=("Brightness",), seed=5).draw(n, 64, 64)
    lo, hi = float(np.float32(0.73)), float(np.float32(1.27))
    assert set(np.unique(t["factor"][:, 0]).tolist()) == {lo, hi} and (t["op"][:, 0] == binding.RA_OP_BRIGHTNESS).all()
    neg = int((t["factor"][:, 0] < 1).sum())
    assert abs(neg - n / 2) <= 5.0 * math.sqrt(n / 4), neg
    t = DRA(num_ops=2, ops=("Posterize", "Solarize"), seed=6).draw(256, 64, 64)             # unsigned: one value each
    assert set(zip(t["op"][:, :2].ravel().tolist(), t["param"][:, :2].ravel().tolist())) == {(binding.RA_OP_POSTERIZE, 7),
                                                                                             (binding.RA_OP_SOLARIZE, 179)}
    assert not t["op"][:, 2:].any() and (t["n_ops"] == 2).all()                             # the unused slots: identity
    t = DRA(num_ops=4, seed=7).draw(2048, 224, 224)                                          # every operation turns up
    assert (t["n_ops"] == 4).all() and set(np.unique(t["op"]).tolist()) == set(range(10))
    counts = np.bincount(t["op"].ravel(), minlength=10) / t["op"].size
    assert abs(counts[binding.RA_OP_AFFINE] - 5 / 14) < 0.03 and abs(counts[binding.RA_OP_EQUALIZE] - 1 / 14) < 0.02
    DRA.check(t, 224, 224)
    w = DRA.trivial_wide(seed=8).draw(2048, 224, 224)
    assert (w["n_ops"] == 1).all() and len(np.unique(w["factor"][:, 0])) > 40               # many bins, both signs
    DRA.check(w, 224, 224)
    zero = DRA(num_ops=0, seed=9).draw(8, 32, 32)
    assert np.array_equal(zero, DRA.identity(8)) and DRA.launch_plan(zero) == (0, 0)
    assert "not claimed" in DRA.__doc__


def test_same_seed_same_tables():
    a, b, c = DRA(seed=3), DRA(seed=3), DRA(seed=4)
    same = [np.array_equal(a.draw(16, 48, 64), b.draw(16, 48, 64)) for _ in range(4)]
    assert all(same) and not np.array_equal(a.draw(16, 48, 64), c.draw(16, 48, 64))
    wa, wb = DRA.trivial_wide(seed=3), DRA.trivial_wide(seed=3)
    assert np.array_equal(wa.draw(16, 48, 64), wb.draw(16, 48, 64))


def test_check_and_constructor_refusals():
    ops = R.every_op(19, 70)
    ok = R.table_of([[ops["rotate+"], ops["posterize0"]], [], [ops["equalize"]] * 4])
    DRA.check(ok, 19, 70)
    assert DRA.launch_plan(ok) == (4, 0b1111)

    def bad(field, idx, value, H=19, W=70):
        t = ok.copy()
        t[field][idx] = value
        with pytest.raises(ValueError):
            DRA.check(t, H, W)

    bad("n_ops", 0, 5), bad("n_ops", 1, -1), bad("op", (0, 0), 10), bad("op", (0, 1), -1), bad("param", (0, 1), 9)
    bad("param", (0, 1), -1), bad("factor", (2, 3), float("nan")), bad("factor", (0, 0), float("inf"))
    bad("coef", (0, 0, 0), 2 ** 17 + 1), bad("coef", (0, 0, 4), -2 ** 17 - 1), bad("coef", (0, 0, 2), 2 ** 30 + 1)
    with pytest.raises(ValueError):
        DRA.check(ok, 4097, 70)
    with pytest.raises(ValueError):
        DRA.check(ok, 19, 0)
    t = ok.copy()                                           # an unused slot may hold anything
    t["op"][1, 0], t["coef"][1, 0] = 77, 2 ** 31 - 1
    DRA.check(t, 19, 70)
    for kw in (dict(num_ops=5), dict(num_ops=-1), dict(num_ops=1.5), dict(magnitude=31), dict(magnitude=-1), dict(num_bins=1),
               dict(ops=()), dict(ops=("Invert",)), dict(fill=256), dict(fill=(1, 2)), dict(fill=0.5), dict(fill=(-1, 0, 0))):
        with pytest.raises(ValueError):
            DRA(**kw)
    assert DRA(fill=7).fill == (7, 7, 7) and DRA(fill=(1, 2, 3)).fill == (1, 2, 3)
    packed = DRA.pack(ok, corners=[(1, 2), (3, 4), (5, 6)], flips=[1, 0, 1], device="cpu")
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (3, 160)
    back = np.frombuffer(packed.numpy().tobytes(), dtype=DRA.dtype())
    assert back["y0"].tolist() == [1, 3, 5] and back["x0"].tolist() == [2, 4, 6] and back["flip"].tolist() == [1, 0, 1]
    assert np.array_equal(back["op"], ok["op"]) and np.array_equal(back["coef"], ok["coef"])


class _Recorder:
    """Stands where the backend stands and keeps what was decided."""

    def __init__(self):
        self.calls, self.stage = [], []

    def collate_crop_mix(self, img_u8, crop_yx, flip, out, mode, lam, box, mean, std, tokens=False):
        self.calls.append((mode, lam, box, None if crop_yx is None else crop_yx.tolist(), flip.tolist()))
        out.zero_()

    def collate_mix(self, img_u8, flip, out, mode, lam, box, mean, std):
        self.collate_crop_mix(img_u8, None, flip, out, mode, lam, box, mean, std)

    def randaugment_scratch_bytes(self, B, H, W):
        return 16

    def randaugment_u8(self, img_u8, samples, out, n_slots, stats_mask, fill=None, scratch=None):
        self.stage.append((np.frombuffer(samples.numpy().tobytes(), dtype=DRA.dtype()).copy(), n_slots, stats_mask, fill))
        out.zero_()


def test_draws_of_the_other_generators_do_not_shift():
    """_TrainInput with and without the stage: the collate's decisions and corners are the same draws, the stage gets the
    corners and the flips, and the collate behind it gets crop=None and no flips."""
    u8 = torch.zeros(6, 3, 20, 24, dtype=torch.uint8)
    labels = torch.arange(6)
    runs = []
    for ra in (None, {"num_ops": 3}):
        inp = trainer._TrainInput(True, False, None, None, None, (16, 16), "mix", 10, 1, False, torch.device("cpu"),
                                  rand_augment=ra)
        rec, ys = _Recorder(), []
        with calm.backend.use_backend(rec):
            for _ in range(4):
                ys.append(inp((u8, labels))[1])
        runs.append((inp, rec, ys))
    (plain, rec0, ys0), (staged, rec1, ys1) = runs
    assert set(plain.generators(0)) == {"collate"} and set(staged.generators(0)) == {"collate", "rand_augment"}
    assert len(rec0.calls) == len(rec1.calls) == len(rec1.stage) == 4 and not rec0.stage
    assert all(torch.equal(a, b) for a, b in zip(ys0, ys1))
    want = DRA(num_ops=3, seed=2006 + 1)
    for (mode, lam, box, corners, flips), (mode1, lam1, box1, corners1, flips1), (t, n_slots, mask, fill) in zip(rec0.calls, rec1.calls, rec1.stage):
        assert (mode, lam, box) == (mode1, lam1, box1) and corners1 is None and flips1 == [0] * 6
        assert np.stack([t["y0"], t["x0"]], axis=1).tolist() == corners and t["flip"].tolist() == flips
        w = want.draw(6, 16, 16)                            # the stage's own stream, nothing else drawn from it
        assert all(np.array_equal(t[f], w[f]) for f in ("n_ops", "op", "factor", "param", "coef"))
        assert (n_slots, mask) == DRA.launch_plan(w) and fill == (0, 0, 0)
    assert plain.collate.rng.bit_generator.state == staged.collate.rng.bit_generator.state


# ---- the C boundary -------------------------------------------------------------------------------------------------------
def test_record_layout_matches_the_header():
    fields = ("y0", "x0", "flip", "n_ops", "op", "factor", "param", "coef")
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "calm_vit.h"\nint main(void){printf("%zu %d %d", sizeof(calm_ra_sample), ' \
          "CALM_RA_MAX_OPS, CALM_RA_MAX_SIDE);\n" + \
          "".join(f'printf(" %zu", offsetof(calm_ra_sample, {f}));\n' for f in fields) + \
          'printf(" %d %d %d %d", CALM_RA_OP_IDENTITY, CALM_RA_OP_AFFINE, CALM_RA_OP_CONTRAST, CALM_RA_OP_EQUALIZE);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == 160 == ctypes.sizeof(binding.RaSample) == DRA.dtype().itemsize
    assert got[1:3] == [binding.RA_MAX_OPS, binding.RA_MAX_SIDE] == [4, 4096] == [R.MAX_OPS, R.MAX_SIDE]
    assert got[3:11] == [getattr(binding.RaSample, f).offset for f in fields] == [DRA.dtype().fields[f][1] for f in fields]
    assert got[11:] == [binding.RA_OP_IDENTITY, binding.RA_OP_AFFINE, binding.RA_OP_CONTRAST, binding.RA_OP_EQUALIZE]
    assert (R.IDENTITY, R.AFFINE, R.BRIGHTNESS, R.COLOR, R.CONTRAST, R.SHARPNESS, R.POSTERIZE, R.SOLARIZE, R.AUTOCONTRAST,
            R.EQUALIZE) == tuple(getattr(binding, "RA_OP_" + n) for n in ("IDENTITY", "AFFINE", "BRIGHTNESS", "COLOR", "CONTRAST",
                                                                         "SHARPNESS", "POSTERIZE", "SOLARIZE", "AUTOCONTRAST", "EQUALIZE"))
    assert "160 bytes" in open(os.path.join(ROOT, "include", "calm_vit.h")).read().split("typedef struct calm_ra_sample")[1][:40]


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "calm_vit.h")).read()
    assert "int calm_randaugment_u8(" in header and "int64_t calm_randaugment_scratch_bytes(" in header
    assert "#define CALM_ABI_VERSION 7" in header.replace("  ", " ")
    lib = binding.load()
    assert lib.calm_abi_version() == 7
    for name in ("calm_randaugment_u8", "calm_randaugment_scratch_bytes"):
        fn = getattr(lib, name)
        restype, argtypes = binding.SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert len(binding.SIGNATURES["calm_randaugment_u8"][1]) == 14
    assert hasattr(calm.backend.HipBackend, "randaugment_u8") and hasattr(calm.backend.HipBackend, "randaugment_scratch_bytes")
    assert "randaugment.hip" in import_module("calm_vit_dte_amd.build").SOURCES


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Every call below is turned down before a launch, so the fake addresses are never read."""
    lib = binding.load()
    P = 0x7f0000010000
    need = lib.calm_randaugment_scratch_bytes(2, 32, 32)
    assert need == 2 * 1024 * 4 + 2 * 2 * 3 * 32 * 32
    assert lib.calm_randaugment_scratch_bytes(3, 5, 7) == 3 * 4096 + 2 * 320              # images padded to 16 bytes
    fill = (ctypes.c_uint8 * 3)(1, 2, 3)
    valid = [P, 40, 36, P, P, 2, 32, 32, 2, 1, fill, P, need, None]
    assert len(valid) == len(binding.SIGNATURES["calm_randaugment_u8"][1])
    for i in (0, 3, 4, 11):                                 # img, samples, out, scratch
        args = list(valid)
        args[i] = None
        assert lib.calm_randaugment_u8(*args) == binding.E_INVAL, i
    for change in ({5: 0}, {5: -1}, {6: 0}, {7: -1}, {6: 41}, {7: 37}, {8: -1}, {8: 5}, {12: need - 1}, {12: 0}, {11: P + 4}):
        args = list(valid)
        for i, v in change.items():
            args[i] = v
        assert lib.calm_randaugment_u8(*args) == binding.E_INVAL, change
    for change in ({5: 65536, 12: 1 << 40}, {1: 5000, 6: 4097, 12: 1 << 40}, {2: 5000, 7: 4097, 12: 1 << 40}):
        args = list(valid)
        for i, v in change.items():
            args[i] = v
        assert lib.calm_randaugment_u8(*args) == binding.E_UNSUPP, change
    assert lib.calm_randaugment_scratch_bytes(0, 8, 8) == binding.E_INVAL
    assert lib.calm_randaugment_scratch_bytes(1, 8, 4097) == binding.E_UNSUPP
    assert lib.calm_randaugment_scratch_bytes(65535, 4096, 4096) == 65535 * 4096 + 2 * 65535 * 3 * 4096 * 4096
    be = calm.backend.HipBackend.__new__(calm.backend.HipBackend)         # the Python side refuses host tensors
    with pytest.raises(TypeError):
        be.randaugment_u8(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), None, None, 0, 0)


# ---- train(rand_augment=) on the gloo path ----------------------------------------------------------------------------------
class EmulatedRandAugBackend(EmulatedBackend):
    """EmulatedBackend with the stage computed by the numpy emulation."""

    def randaugment_scratch_bytes(self, B, H, W):
        return 16

    def randaugment_u8(self, img_u8, samples, out, n_slots, stats_mask, fill=None, scratch=None):
        t = np.frombuffer(samples.numpy().tobytes(), dtype=DRA.dtype())
        H, W = out.shape[2:]
        out.copy_(torch.from_numpy(R.randaugment(img_u8.numpy(), t, H, W, fill or (0, 0, 0), n_slots, stats_mask)))


class _U8Set(torch.utils.data.Dataset):
    def __init__(self, n=16, side=36):
        self.x = torch.from_numpy(np.stack([R.image(900 + i, side, side, "ramp") for i in range(n)]))
        self.y = torch.randint(0, 10, (n,), generator=torch.Generator().manual_seed(7))

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return self.x[i], int(self.y[i])


def _train(seen=None, seed=50, n=16, **kw):
    """train(device_collate=True, crop=(32, 32)) on the host (see the module's docstring); seen: collects the (tokens, soft
    labels) that reach the model."""
    torch.manual_seed(seed)
    m = build_model("tiny32_cls", None).train()
    real_check, real_ce = trainer._check_train_args, trainer.soft_target_cross_entropy
    hook = m.register_forward_pre_hook(lambda mod, args: seen.append([args[0].detach().clone()])) if seen is not None else None

    def checks(initializer, optimizer, use_gpu, *a, **k):
        return real_check(initializer, optimizer, True, *a, **k)

    def spy(logits, targets, metrics=None):
        seen[-1].append(targets.detach().clone())
        return real_ce(logits, targets, metrics)

    trainer._check_train_args = checks
    if seen is not None:
        trainer.soft_target_cross_entropy = spy
    try:
        with calm.backend.use_backend(EmulatedRandAugBackend()):
            out = trainer.train(m, trainer.make_optimizer(m), scheduler=False, use_gpu=False, dataset=_U8Set(n), epochs=2,
                                batch_size=4, num_classes=10, num_workers=0, log_every=1000, device_collate=True, crop=(32, 32),
                                **kw)
    finally:
        trainer._check_train_args, trainer.soft_target_cross_entropy = real_check, real_ce
        if hook is not None:
            hook.remove()
    return out


RA_KW = {"num_ops": 3, "magnitude": 12, "fill": (9, 8, 7)}


def _hand_written_batches(n, rank, world, epochs=2):
    """What train(rand_augment=RA_KW) feeds the model, written out: the sampler's order, the collate's decisions and
    corners, the stage's table, the emulation, the plain collate without crop and flips."""
    data, be = _U8Set(n), EmulatedBackend()
    col, ra = trainer.DeviceCollate(num_classes=10, seed=2006 + rank), DRA(seed=2006 + rank, **RA_KW)
    out = []
    for epoch in range(epochs):
        order = torch.randperm(n, generator=torch.Generator().manual_seed(2006 + epoch)).tolist()[rank::world]
        for i in range(0, len(order), 4):
            x = torch.stack([data[j][0] for j in order[i:i + 4]])
            y = torch.tensor([data[j][1] for j in order[i:i + 4]])
            mode, lam, box, flips = col.draw(len(x), 32, 32)
            corners = col.draw_corners(len(x), 36, 36, 32, 32)
            t = ra.draw(len(x), 32, 32)
            t["y0"], t["x0"], t["flip"] = corners[:, 0], corners[:, 1], flips.numpy()
            u8 = torch.from_numpy(R.randaugment(x.numpy(), t, 32, 32, ra.fill, *DRA.launch_plan(t)))
            tokens = torch.empty(len(x), 32, 96)
            be.collate_crop_mix(u8, None, torch.zeros_like(flips), tokens, mode, lam, box, col.MEAN, col.STD, tokens=True)
            onehot = torch.nn.functional.one_hot(y, 10).float()
            out.append((tokens, onehot * lam + onehot.roll(1, 0) * (1.0 - lam)))
    return out


def _assert_fed(seen, want):
    assert len(seen) == len(want)
    for (x, y), (wx, wy) in zip(seen, want):
        assert torch.equal(x, wx) and torch.equal(y, wy)


def _same(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.mark.timeout(600)
def test_train_with_rand_augment_equals_the_hand_written_loop():
    seen = []
    _train(seen, rand_augment=RA_KW)
    _assert_fed(seen, _hand_written_batches(16, 0, 1))
    assert not torch.distributed.is_initialized()


@pytest.mark.timeout(600)
def test_num_ops_zero_is_the_run_without_the_argument():
    a, b, c = _train(n=8), _train(n=8, rand_augment={"num_ops": 0}), _train(n=8, rand_augment=RA_KW)
    assert _same(a, b) and not _same(a, c)
    assert _same(a, _train(n=8, rand_augment=None)) and _same(a, _train(n=8, rand_augment=False))


@pytest.mark.timeout(600)
def test_train_with_rand_augment_resumes_bit_for_bit(tmp_path):
    fa, fb, fc = (str(tmp_path / f"{n}.snap") for n in "abc")
    a = _train(rand_augment=RA_KW, snapshot_path=fa)
    _train(rand_augment=RA_KW, snapshot_path=fb, snapshot_every=3, max_steps=3)
    host = trainer.TrainState.read_header(fb)[0]["host"]
    assert host["progress"] == {"epoch": 0, "batch": 3, "step": 3} and "rand_augment" in host["generators"]
    c = _train(seed=51, rand_augment=RA_KW, snapshot_path=fc, resume=fb)
    assert _same(a, c)
    assert trainer.TrainState.read_header(fa)[0]["host"]["generators"] == trainer.TrainState.read_header(fc)[0]["host"]["generators"]
    with pytest.raises(Exception):                          # a snapshot written with the stage, a run without it
        _train(seed=51, snapshot_path=fc, resume=fb)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _two_rank_worker(rank, world, ports, outdir):
    torch.set_num_threads(2)
    f = {n: os.path.join(outdir, f"{n}.snap") for n in "abc"}
    runs = [("a", dict(snapshot_path=f["a"])), ("b", dict(snapshot_path=f["b"], snapshot_every=3, max_steps=3)),
            ("c", dict(snapshot_path=f["c"], resume=f["b"], seed=51))]
    for (name, kw), port in zip(runs, ports):
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        seen = []
        out = _train(seen, n=32, rand_augment=RA_KW, **kw)
        if name == "a":
            _assert_fed(seen, _hand_written_batches(32, rank, world))
        torch.save(out.state_dict(), os.path.join(outdir, f"{name}_rank{rank}.pt"))


@pytest.mark.timeout(600)
def test_train_with_rand_augment_on_two_gloo_ranks(tmp_path):
    """Each rank feeds its model what the hand-written loop gives for its shard and its seed 2006 + rank, and the run
    resumes bit for bit from the snapshot and the ranks' sidecars."""
    d = str(tmp_path)
    mp.spawn(_two_rank_worker, args=(2, [_free_port() for _ in range(3)], d), nprocs=2, join=True)
    for r in range(2):
        a, c = torch.load(os.path.join(d, f"a_rank{r}.pt")), torch.load(os.path.join(d, f"c_rank{r}.pt"))
        assert set(a) == set(c) and all(torch.equal(a[k], c[k]) for k in a)
    a0, a1 = (torch.load(os.path.join(d, f"a_rank{r}.pt")) for r in range(2))
    assert all(torch.equal(a0[k], a1[k]) for k in a0)       # the ranks hold one model
    s0, s1 = (__import__("json").load(open(os.path.join(d, f"a.snap.rank{r}.json"))) for r in range(2))
    assert s0["generators"]["rand_augment"] != s1["generators"]["rand_augment"]


def test_refusals_come_before_any_process_group():
    data = torch.utils.data.TensorDataset(torch.zeros(4, 3, 36, 36, dtype=torch.uint8), torch.randint(0, 10, (4,)))
    lin = torch.nn.Linear(4, 4)
    sgd = torch.optim.SGD(lin.parameters(), lr=0.1)
    kw = dict(use_gpu=False, dataset=data, epochs=1, batch_size=2, num_classes=10)
    with pytest.raises(ValueError, match="rand_augment needs device_collate=True"):
        trainer.train(lin, sgd, rand_augment=True, **kw)
    with pytest.raises(ValueError, match="rand_augment needs device_collate=True"):
        trainer.train(lin, "fused", rand_augment=DRA(), **dict(kw, use_gpu=True))
    gpu = dict(kw, use_gpu=True, device_collate=True)
    with pytest.raises(ValueError, match='"num_ops", "magnitude", "num_bins", "fill", "ops", "seed"'):
        trainer.train(lin, "fused", rand_augment={"n": 2}, **gpu)
    with pytest.raises(ValueError, match="num_ops counts operations per sample"):
        trainer.train(lin, "fused", rand_augment={"num_ops": 5}, **gpu)
    with pytest.raises(ValueError, match="magnitude is a bin"):
        trainer.train(lin, "fused", rand_augment={"magnitude": 31}, **gpu)
    with pytest.raises(ValueError, match="rand_augment is None, True, a dict"):
        trainer.train(lin, "fused", rand_augment="on", **gpu)
    with pytest.raises(ValueError, match="at most 4096 x 4096"):
        trainer.train(lin, "fused", rand_augment=True, crop=(4100, 32), **gpu)
    assert not torch.distributed.is_initialized()
    inp = trainer._TrainInput(True, True, None, None, None, (32, 32), "mix", 10, 3, False, torch.device("cpu"),
                              random_erasing={"p": 0.5}, rand_augment={})
    assert set(inp.generators(0)) == {"collate", "augment", "erase", "rand_augment"}
    assert inp.randaug.rng.bit_generator.state == DRA(seed=2006 + 3).rng.bit_generator.state and inp.randaug.num_ops == 2
    own = DRA.trivial_wide(seed=1)
    assert trainer._TrainInput(True, False, None, None, None, None, "mix", 10, 0, False, torch.device("cpu"),
                               rand_augment=own).randaug is own
