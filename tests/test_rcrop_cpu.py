"""Device resized crop without a GPU: the numpy emulation the kernel is tested against (tests/emulated_rcrop.py) against
PIL's crop().resize() itself and against the committed PIL outputs, byte for byte; the records trainer.DeviceResizedCrop
builds (.center against hand-computed values, .random_resized against RandomResizedCrop's rules, .window against
DeviceCollate's corners); the record predicate calm_resized_crop_check — the function the kernel guards every address
with — against a Python predicate; the argument checks of the entry point, of train() and of evaluate(); the layout of
struct calm_rcrop_sample."""
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

import calm_vit_dte_amd as calm  # noqa: E402,F401
import emulated_rcrop as EC  # noqa: E402
import emulated_resize as ER  # noqa: E402
import make_golden_rcrop as MG  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
DRC = trainer.DeviceResizedCrop
FIELDS = ("offset", "h", "w", "by0", "bx0", "bh", "bw", "vh", "vw", "wy0", "wx0")


def _meta(sizes):
    """[B, 3] of (offset, h, w) with the images one after the other, and the bytes they take."""
    meta, end = [], 0
    for h, w in sizes:
        meta.append((end, h, w))
        end += 3 * h * w
    return np.asarray(meta, dtype=np.int64), end


# ---- the emulation is PIL's crop().resize() -------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(EC.CASES)), ids=lambda i: "case%d_%dx%d" % ((i,) + EC.CASES[i][0]))
def test_emulation_equals_pil_crop_then_resize_byte_for_byte(i):
    (h, w), box, size, window = EC.CASES[i]
    assert box[2] <= 16 * box[3] and box[3] <= 16 * box[2]          # PIL keeps the horizontal-then-vertical order here
    src = EC.source(i)
    want = MG.pil_rcrop(src, box, size, window)
    got = EC.rcrop(src, box, size, window)
    differing = int((got != want).sum())
    print(f"{h}x{w} box {box} -> {size} window {window}: {differing} differing bytes of {want.size}")
    assert got.shape == want.shape == (window[2], window[3], 3) and differing == 0


def test_there_are_the_cases_the_contract_names():
    boxes = [(c[0], c[1]) for c in EC.CASES]
    assert len(EC.CASES) >= 12
    assert any(b[2:] == (1, 1) and c[2] > (1, 1) for c in EC.CASES for b in [c[1]])                 # a 1x1 box upscaled
    for corner in ("tl", "tr", "bl", "br"):                                                          # a box at each corner
        assert any((by0 == 0 if corner[0] == "t" else by0 + bh == h) and (bx0 == 0 if corner[1] == "l" else bx0 + bw == w)
                   and (bh, bw) != (h, w) for (h, w), (by0, bx0, bh, bw) in boxes), corner
    assert any(b[1] % 2 == 1 for _, b in boxes)                                                      # an odd bx0
    assert any((c[2][0] < c[1][2]) != (c[2][1] < c[1][3]) and c[2][0] != c[1][2] and c[2][1] != c[1][3] for c in EC.CASES)
    assert any(c[2] == c[1][2:] for c in EC.CASES)                                                   # the identity size


def test_resize_with_a_box_argument_is_another_function():
    """Image.resize(size, BILINEAR, box=box) reads pixels around the box: it is not crop-then-resize, the contract."""
    differing = 0
    for i in (1, 10):
        (h, w), box, size, window = EC.CASES[i]
        src = EC.source(i)
        differing += int((MG.pil_resize_box(src, box, size, window) != MG.pil_rcrop(src, box, size, window)).sum())
    assert differing > 0


def test_emulation_equals_the_committed_pil_outputs():
    g = np.load(MG.PATH)
    for i, ((h, w), box, size, window) in enumerate(EC.CASES):
        src = EC.source(i)
        if h * w <= MG.SRC_KEPT_PIXELS:
            assert np.array_equal(g[f"src_{i}"], src)                # the seeded inputs reproduce
        assert np.array_equal(MG.kept(EC.rcrop(src, box, size, window)), g[f"out_{i}"]), i
    assert os.path.getsize(MG.PATH) < 256 * 1024


# ---- the records of DeviceResizedCrop ------------------------------------------------------------------------------------
def test_center_records_equal_hand_computed_values():
    """Resize(256): the short side to 256, the long one to int(256 * long / short); CenterCrop(224): top =
    int(round((vh - 224) / 2.0)) — 500x375 gives 341 x 256 and (58, 16): round(58.5) is 58 in Python."""
    sizes = [(500, 375), (375, 500), (333, 500), (256, 256), (224, 1000)]
    meta, n = _meta(sizes)
    t = DRC.center(256, (224, 224)).records(meta, n)
    assert t.dtype.itemsize == 48
    want = [(341, 256, 58, 16), (256, 341, 16, 58), (256, 384, 16, 80), (256, 256, 16, 16), (256, 1142, 16, 459)]
    assert [tuple(int(r[f]) for f in ("vh", "vw", "wy0", "wx0")) for r in t] == want
    assert [tuple(int(r[f]) for f in ("by0", "bx0", "bh", "bw")) for r in t] == [(0, 0, h, w) for h, w in sizes]
    assert t["offset"].tolist() == meta[:, 0].tolist()
    for k, i in enumerate(EC.CENTER_CASES):                          # the cases the emulation is held to PIL on
        (h, w), box, size, window = EC.CASES[i]
        assert (h, w) == sizes[k] and size == want[k][:2] and window == want[k][2:] + (224, 224) and box == (0, 0, h, w)
    t = DRC.center(56, (48, 40)).records(*_meta([(60, 91), (91, 60)]))
    assert [tuple(int(r[f]) for f in ("vh", "vw", "wy0", "wx0")) for r in t] == [(56, 84, 4, 22), (84, 56, 18, 8)]
    with pytest.raises(ValueError):                                  # 40 x 300 resizes to 56 x 420: 48 rows fit, 48 x 440 does not
        DRC.center(56, (48, 440)).records(*_meta([(40, 300)]))
    with pytest.raises(ValueError):
        DRC.center(56, (60, 40)).records(*_meta([(40, 300)]))        # the short side is the height: 60 rows do not fit 56
    for bad in (dict(resize=0), dict(resize=(56, 56)), dict(resize=56, crop=48), dict(resize=56, crop=(0, 48)),
                dict(resize=56, crop=(60, 60)), dict(resize=16385)):
        with pytest.raises(ValueError):
            DRC.center(**bad)


def test_random_resized_records_follow_random_resized_crop():
    sizes = [(500, 375), (375, 500), (64, 64), (97, 31), (33, 200)] * 8
    meta, n = _meta(sizes)
    a = DRC.random_resized((24, 20), seed=5)
    t = a.records(meta, n)
    assert a.last_records is t and int((~a.last_fallback).sum()) >= 30
    for r, (h, w), fallback in zip(t, sizes, a.last_fallback):
        by0, bx0, bh, bw = (int(r[f]) for f in ("by0", "bx0", "bh", "bw"))
        assert 0 <= by0 and 0 <= bx0 and bh >= 1 and bw >= 1 and by0 + bh <= h and bx0 + bw <= w      # inside the image
        assert (int(r["vh"]), int(r["vw"]), int(r["wy0"]), int(r["wx0"])) == (24, 20, 0, 0)
        if fallback:
            continue
        # bh = round(sqrt(A / r)), bw = round(sqrt(A r)) with A in [0.08, 1] h w and r in [3/4, 4/3]: each side is within
        # one half of its unrounded value
        lo_a, hi_a = 0.08 * h * w, 1.0 * h * w
        assert (bh - 0.5) * (bw - 0.5) <= hi_a and (bh + 0.5) * (bw + 0.5) >= lo_a
        assert (bw - 0.5) / (bh + 0.5) <= 4.0 / 3.0 and (bw + 0.5) / (bh - 0.5) >= 3.0 / 4.0
    assert len({(int(r["bh"]), int(r["bw"])) for r in t}) > 20                                         # drawn per image
    again = DRC.random_resized((24, 20), seed=5).records(meta, n)
    assert np.array_equal(again, t)                                                                    # reproducible per seed
    assert not np.array_equal(DRC.random_resized((24, 20), seed=6).records(meta, n), t)
    # ten failed attempts on 10 x 400 (every box of the area range is taller than 10 rows): the central box, ratio clamped
    b = DRC.random_resized((24, 20), seed=1)
    t = b.records(*_meta([(10, 400), (400, 10), (64, 64)]))
    assert b.last_fallback.tolist() == [True, True, False]
    assert tuple(int(t[0][f]) for f in ("by0", "bx0", "bh", "bw")) == (0, (400 - 13) // 2, 10, 13)      # round(10 * 4 / 3)
    assert tuple(int(t[1][f]) for f in ("by0", "bx0", "bh", "bw")) == ((400 - 13) // 2, 0, 13, 10)      # round(10 / (3 / 4))
    one = DRC.random_resized((8, 8), scale=(1.0, 1.0), ratio=(1.0, 1.0), seed=0).records(*_meta([(30, 30)]))
    assert tuple(int(one[0][f]) for f in ("by0", "bx0", "bh", "bw")) == (0, 0, 30, 30)
    for bad in (dict(size=8), dict(scale=(0.0, 1.0)), dict(scale=(0.5, 0.1)), dict(ratio=(2.0, 1.0)), dict(ratio=1.0)):
        with pytest.raises(ValueError):
            DRC.random_resized(**bad)


def test_random_resized_leaves_the_stream_of_device_collate_alone():
    """The transform owns its generator: a DeviceCollate draws the same decisions and corners whether or not one is used."""
    def stream(use):
        c = trainer.DeviceCollate(num_classes=10, seed=77)
        rrc = DRC.random_resized((24, 20), seed=77)
        out = []
        for _ in range(3):
            if use:
                rrc.records(*_meta([(64, 64), (50, 70)]))
            mode, lam, box, flips = c.draw(2, 24, 20)
            out.append((mode, lam, box, flips.tolist(), c.draw_corners(2, 28, 28, 24, 20).tolist()))
        return out
    assert stream(False) == stream(True)


def test_window_and_draw_corners_reproduce_the_corners_of_device_collate(monkeypatch):
    """DeviceCollate.__call__(crop=(H, W)) draws draw() and then the corners; draw() followed by draw_corners() on a
    second object of the same seed gives the same decisions and the same corners, batch after batch, and .window puts them
    into the records."""
    class _Dev:                                                     # __call__ needs a backend only to launch
        def collate_crop_mix(self, *a, **k):
            pass
    monkeypatch.setattr(import_module("calm_vit_dte_amd.backend"), "get_backend", lambda: _Dev())
    a, b = (trainer.DeviceCollate(num_classes=10, seed=31) for _ in range(2))
    win = DRC.window((56, 60), (48, 40))
    meta, n = _meta([(70, 90)] * 6)
    img = torch.zeros(6, 3, 56, 60, dtype=torch.uint8)
    labels = torch.arange(6)
    for _ in range(3):
        seen = {}
        monkeypatch.setattr(a, "draw", lambda B, H, W, d=trainer.DeviceCollate.draw: seen.setdefault("d", d(a, B, H, W)))
        a(img, labels, crop=(48, 40), tokens=True)
        mode, lam, box, flips = b.draw(6, 48, 40)
        corners = b.draw_corners(6, 56, 60, 48, 40)
        assert (mode, lam, box) == seen["d"][:3] and torch.equal(flips, seen["d"][3])
        assert corners.dtype == np.int32 and np.array_equal(corners, a.last_corners.numpy())
        t = win.records(meta, n, corners=corners)
        assert np.array_equal(t["wy0"], corners[:, 0]) and np.array_equal(t["wx0"], corners[:, 1])
        assert (t["vh"] == 56).all() and (t["vw"] == 60).all() and (t["bh"] == 70).all() and (t["bw"] == 90).all()
    with pytest.raises(ValueError):
        win.records(meta, n)                                         # .window needs its corners
    with pytest.raises(ValueError):
        win.records(meta, n, corners=np.asarray([[9, 0]] * 6))       # 9 + 48 > 56: the kernel would write zeros
    with pytest.raises(ValueError):
        win.records(meta, n, corners=np.asarray([[0, -1]] * 6))
    with pytest.raises(ValueError):
        DRC.center(56, (48, 48)).records(meta, n, corners=corners)
    with pytest.raises(ValueError):
        DRC.window((56, 56), (57, 48))


def test_records_refuse_what_the_kernel_would_zero():
    meta, n = _meta([(60, 70), (80, 64)])
    tr = DRC.center(56, (48, 48))
    assert len(tr.records(meta, n)) == 2
    for bad in ([[0, 0, 4]], [[0, 4, 0]], [[0, 16385, 100]], [[-16, 60, 70]], [[n - 11, 60, 70]]):
        with pytest.raises(ValueError):
            tr.records(np.asarray(bad), n)
    with pytest.raises(ValueError):
        tr.records(meta, n - 1)                                      # the last image ends past the buffer
    with pytest.raises(ValueError):
        tr.records(np.zeros((3, 2), dtype=np.int64), 100)
    with pytest.raises(ValueError):
        DRC.center(56, (48, 48))(torch.zeros(n, dtype=torch.uint8), meta, out="rows")


# ---- calm_resized_crop_check: the guard of the kernel, on the host ------------------------------------------------------
def _valid(r, nbytes, H, W):
    """The conditions of include/calm_vit.h on Python integers (which do not wrap)."""
    side = 16384
    return (1 <= r["h"] <= side and 1 <= r["w"] <= side and 0 <= r["offset"] and r["offset"] + 3 * r["h"] * r["w"] <= nbytes
            and r["by0"] >= 0 and r["bx0"] >= 0 and r["bh"] >= 1 and r["bw"] >= 1
            and r["by0"] + r["bh"] <= r["h"] and r["bx0"] + r["bw"] <= r["w"]
            and 1 <= r["vh"] <= side and 1 <= r["vw"] <= side and r["wy0"] >= 0 and r["wx0"] >= 0 and H >= 1 and W >= 1
            and r["wy0"] + H <= r["vh"] and r["wx0"] + W <= r["vw"])


def _check_table():
    """(record, nbytes, H, W, expected) — a good record and every bound of it off by one, both ways."""
    good = dict(offset=64, h=100, w=80, by0=10, bx0=7, bh=90, bw=73, vh=60, vw=50, wy0=12, wx0=2)
    nbytes, H, W = 64 + 3 * 100 * 80, 48, 48
    rows = [(good, nbytes, H, W, True)]

    def vary(expected, nb=nbytes, hh=H, ww=W, **change):
        rows.append((dict(good, **change), nb, hh, ww, expected))
    i32 = 2 ** 31 - 1
    vary(True, by0=0, bx0=0, bh=100, bw=80)                          # the whole image
    vary(True, by0=99, bx0=79, bh=1, bw=1)                           # its last pixel
    vary(False, nb=nbytes - 1)                                       # the image ends one byte past the buffer
    vary(True, nb=nbytes + 1)
    vary(True, offset=0)
    vary(False, offset=-1)
    vary(False, offset=65)
    vary(False, h=0), vary(False, w=0), vary(False, h=-1), vary(False, w=-1)
    vary(False, h=16385, nb=1 << 40), vary(False, w=16385, nb=1 << 40)
    vary(True, h=16384, nb=1 << 40), vary(True, w=16384, nb=1 << 40)
    vary(True, h=16384, w=16384, nb=64 + 3 * 16384 * 16384)          # 3 h w = 805306368 fits 32 bits,
    vary(False, h=16384, w=16384, nb=64 + 3 * 16384 * 16384 - 1)
    vary(False, h=i32, w=i32, nb=1 << 40)                            # sides whose product overflows 32 (and 64) bits
    vary(False, h=65536, w=65536, nb=1 << 40)                        # 3 h w = 3 * 2^32
    vary(False, h=46341, w=46341, nb=1 << 40)                        # h w just above 2^31
    vary(False, by0=-1), vary(False, bx0=-1), vary(False, bh=0), vary(False, bw=0), vary(False, bh=-5), vary(False, bw=-5)
    vary(False, by0=11), vary(False, bx0=8)                          # by0 + bh = h + 1, bx0 + bw = w + 1
    vary(False, bh=91), vary(False, bw=74)
    vary(False, by0=i32, bh=i32), vary(False, bx0=i32, bw=i32)      # sums that wrap in 32 bits
    vary(False, by0=i32, bh=2), vary(False, bx0=i32, bw=2)
    vary(False, vh=0), vary(False, vw=0), vary(False, vh=16385, wy0=0), vary(False, vw=16385, wx0=0)
    vary(True, vh=16384), vary(True, vw=16384), vary(True, vh=16384, wy0=16384 - 48), vary(True, vw=16384, wx0=16384 - 48)
    vary(False, vh=16384, wy0=16384 - 47), vary(False, vw=16384, wx0=16384 - 47)
    vary(False, wy0=-1), vary(False, wx0=-1)
    vary(True, wy0=12, vh=60), vary(False, wy0=13)                   # wy0 + H = vh, vh + 1
    vary(True, wx0=2, vw=50), vary(False, wx0=3)
    vary(False, vh=59), vary(False, vw=49)
    vary(False, wy0=i32), vary(False, wx0=i32)                       # wy0 + H wraps in 32 bits
    vary(False, hh=49), vary(False, ww=49), vary(True, hh=1, ww=1), vary(False, hh=0), vary(False, ww=0)
    vary(False, hh=-1), vary(False, ww=i32), vary(False, hh=i32)
    # an offset near 2^62: inside a buffer that large, outside one byte smaller; nbytes - offset must not wrap either
    big = 1 << 62
    vary(True, offset=big, nb=big + 3 * 100 * 80)
    vary(False, offset=big, nb=big + 3 * 100 * 80 - 1)
    vary(False, offset=big, nb=nbytes)
    vary(False, offset=big + 1, nb=big)
    vary(False, offset=(1 << 63) - 1, nb=(1 << 63) - 1)
    vary(False, offset=-(1 << 63), nb=(1 << 63) - 1)                 # nbytes - offset would wrap
    vary(False, nb=0), vary(False, nb=-1), vary(False, nb=-(1 << 63))
    return rows


def test_check_entry_point_equals_the_python_predicate():
    lib = binding.load()
    rows = _check_table()
    assert len(rows) > 70
    n_good = 0
    for r, nbytes, H, W, expected in rows:
        assert _valid(r, nbytes, H, W) == expected, (r, nbytes, H, W)            # the table states what it means
        s = binding.RCropSample(**r)
        assert lib.calm_resized_crop_check(ctypes.byref(s), nbytes, H, W) == int(expected), (r, nbytes, H, W)
        rec = np.zeros(1, dtype=DRC.dtype())
        for f in FIELDS:
            rec[f] = r[f]
        assert bool(DRC.valid(rec, nbytes, H, W)[0]) == expected, (r, nbytes, H, W)      # trainer's host check agrees
        n_good += expected
    assert 10 < n_good < len(rows) - 40
    assert lib.calm_resized_crop_check(None, 1 << 20, 8, 8) == 0
    # a seeded sweep around the bounds: small integers on every field, so that sums meet their limits often
    rng = np.random.default_rng(12)
    seen = set()
    for _ in range(3000):
        r = dict(offset=int(rng.integers(-1, 4)), h=int(rng.integers(0, 6)), w=int(rng.integers(0, 6)),
                 by0=int(rng.integers(-1, 4)), bx0=int(rng.integers(-1, 4)), bh=int(rng.integers(0, 6)),
                 bw=int(rng.integers(0, 6)), vh=int(rng.integers(0, 6)), vw=int(rng.integers(0, 6)),
                 wy0=int(rng.integers(-1, 3)), wx0=int(rng.integers(-1, 3)))
        nbytes, H, W = int(rng.integers(0, 80)), int(rng.integers(0, 4)), int(rng.integers(0, 4))
        want = _valid(r, nbytes, H, W)
        seen.add(want)
        assert lib.calm_resized_crop_check(ctypes.byref(binding.RCropSample(**r)), nbytes, H, W) == int(want), (r, nbytes, H, W)
    assert seen == {True, False}


# ---- the C boundary ---------------------------------------------------------------------------------------------------------
def test_rcrop_sample_layout_matches_the_header():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "calm_vit.h"\nint main(void){printf("%zu", sizeof(calm_rcrop_sample));\n' + \
          "".join(f'printf(" %zu", offsetof(calm_rcrop_sample, {f}));\n' for f in FIELDS) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == 48 == ctypes.sizeof(binding.RCropSample) == DRC.dtype().itemsize
    assert got[1:] == [getattr(binding.RCropSample, f).offset for f in FIELDS]
    assert got[1:] == [DRC.dtype().fields[f][1] for f in FIELDS]


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """On a host without a GPU: every call below is turned down by the argument checks, so the fake device addresses are
    never read and nothing is launched."""
    lib = binding.load()
    P = 0x7f0000010000
    ms = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    valid = [P, 1 << 20, P, P, 4, 224, 224, 2, ms, ms, None]
    assert len(valid) == len(binding.SIGNATURES["calm_resized_crop"][1])
    E, U = binding.E_INVAL, binding.E_UNSUPP
    for change, code in (({0: None}, E), ({2: None}, E), ({3: None}, E), ({1: 0}, E), ({1: -5}, E), ({4: 0}, E), ({4: -1}, E),
                         ({5: 0}, E), ({6: 0}, E), ({6: -3}, E), ({7: 3}, E), ({7: -1}, E), ({8: None}, E), ({9: None}, E),
                         ({7: 1, 8: None}, E), ({7: 1, 9: None}, E), ({4: 65536}, U), ({5: 16385}, U), ({6: 16385}, U),
                         ({7: 0, 8: None, 9: None, 4: 65536}, U)):
        args = list(valid)
        for i, v in change.items():
            args[i] = v
        assert lib.calm_resized_crop(*args) == code, change


def test_train_and_evaluate_refuse_bad_combinations():
    data = torch.utils.data.TensorDataset(torch.zeros(4, 32, 32, 3, dtype=torch.uint8), torch.randint(0, 10, (4,)))
    rrc = DRC.random_resized((24, 24), seed=0)
    kw = dict(use_gpu=True, dataset=data, epochs=1, batch_size=2, num_classes=10)
    for bad in (dict(resize_window=True), dict(resize_window=True, device_collate=True, device_resize=(28, 28)),
                dict(resize_window=True, device_collate=True, crop=(24, 24)),
                dict(resize_window=True, device_collate=True, device_resize=(28, 28), crop=(24, 30)),
                dict(random_resized_crop=rrc), dict(random_resized_crop=rrc, device_collate=True, crop=(24, 24)),
                dict(random_resized_crop=rrc, device_collate=True, device_resize=(28, 28)),
                dict(random_resized_crop=DRC.center(28, (24, 24)), device_collate=True),
                dict(random_resized_crop=(24, 24), device_collate=True)):
        with pytest.raises(ValueError):
            trainer.train(torch.nn.Linear(4, 4), "fused", **dict(kw, **bad))
    assert not torch.distributed.is_initialized()
    m = torch.nn.Linear(4, 4)
    with pytest.raises(TypeError):
        trainer.evaluate(m, [], transform=trainer.DeviceResize((24, 24)))
    with pytest.raises(ValueError):
        trainer.evaluate(m, [], transform=DRC.window((28, 28), (24, 24)))
    with pytest.raises(ValueError):
        trainer.evaluate(m, [], transform=rrc)                                          # no random crops in an evaluation
    with pytest.raises(ValueError):
        trainer.evaluate(m, [], transform=DRC.center(28, (24, 24)), transform_out="u8")
    with pytest.raises(ValueError):
        trainer.evaluate(m, [], transform=DRC.center(28, (24, 24)))                    # a model on the CPU
    assert math.isclose(DRC.MEAN[0], 0.485) and DRC.STD == trainer.DeviceCollate.STD
