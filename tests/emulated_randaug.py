"""Numpy restatement of calm_randaugment_u8 (include/calm_vit.h): the crop window and the flip, then a chain of uint8 -> uint8
operations, each rounded as PIL rounds it.  tests/test_randaug_cpu.py holds it against PIL byte for byte and
tests/test_randaug_gpu.py holds the kernel against it.  Nothing follows the kernel's organisation: whole-image numpy
expressions, one operation after the other.

It also holds the record builders and the cases both test files share."""
import functools
import math

import numpy as np

# device operation ids (CALM_RA_OP_*)
IDENTITY, AFFINE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, POSTERIZE, SOLARIZE, AUTOCONTRAST, EQUALIZE = range(10)
MAX_OPS = 4
MAX_SIDE = 4096
f32 = np.float32


# ---- host side: the six coefficients and their 16.16 form -----------------------------------------------------------------
def fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def fixed_coeffs(a):
    """(A0 .. A5) of the inverse map a[0..5] (doubles), PIL's affine_fixed."""
    a = [float(v) for v in a]
    return (fix(a[0]), fix(a[1]), fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[3]), fix(a[4]), fix(a[5] + a[3] * 0.5 + a[4] * 0.5))


def shear_x(s):
    return (1.0, float(s), 0.0, 0.0, 1.0, 0.0)


def shear_y(s):
    return (1.0, 0.0, 0.0, float(s), 1.0, 0.0)


def translate_x(t):
    return (1.0, 0.0, -float(int(t)), 0.0, 1.0, 0.0)


def translate_y(t):
    return (1.0, 0.0, 0.0, 0.0, 1.0, -float(int(t)))


def rotate(angle, H, W):
    """Image.rotate's matrix about (W / 2, H / 2), counter-clockwise degrees."""
    r = -math.radians(angle % 360.0)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


# ---- the operations on one [3,H,W] uint8 window ------------------------------------------------------------------------------
def affine(x, A, fill=(0, 0, 0)):
    _, H, W = x.shape
    A = [np.int64(v) for v in A]
    yy, xx = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    wrap = lambda v: ((v + 2 ** 31) % 2 ** 32) - 2 ** 31          # the device's 32-bit arithmetic
    xin = wrap(A[2] + A[1] * yy + A[0] * xx) >> 16
    yin = wrap(A[5] + A[4] * yy + A[3] * xx) >> 16
    ok = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    out = np.empty_like(x)
    xi, yi = np.clip(xin, 0, W - 1), np.clip(yin, 0, H - 1)
    for c in range(3):
        out[c] = np.where(ok, x[c][yi, xi], np.uint8(fill[c]))
    return out


def blend(d, s, f):
    """Image.blend(d, s, f) on uint8 arrays: fp32, one rounding per operation."""
    f = f32(f)
    d, s = d.astype(f32), s.astype(f32)
    t = d + (f * (s - d)).astype(f32)
    t = t.astype(f32)
    if 0.0 <= float(f) <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0.0, 0, np.where(t >= 255.0, 255, t.astype(np.int32))).astype(np.uint8)


def luma(x):
    r, g, b = (x[c].astype(np.int64) for c in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16).astype(np.uint8)


def brightness(x, f):
    return blend(np.zeros_like(x), x, f)


def color(x, f):
    return blend(np.broadcast_to(luma(x), x.shape), x, f)


def contrast(x, f):
    L = luma(x).astype(np.int64)
    n = L.size
    m = (2 * int(L.sum()) + n) // (2 * n)
    return blend(np.full_like(x, m), x, f)


def smooth(x):
    _, H, W = x.shape
    if H < 3 or W < 3:
        return x.copy()
    k = [f32(v) / f32(13.0) for v in (1, 1, 1, 1, 5, 1, 1, 1, 1)]
    acc = np.full((3, H - 2, W - 2), 0.5, dtype=f32)
    i = 0
    for dy in range(3):
        for dx in range(3):
            acc = (acc + (x[:, dy:dy + H - 2, dx:dx + W - 2].astype(f32) * k[i]).astype(f32)).astype(f32)
            i += 1
    out = x.copy()
    out[:, 1:-1, 1:-1] = np.clip(acc.astype(np.int32), 0, 255).astype(np.uint8)
    return out


def sharpness(x, f):
    return blend(smooth(x), x, f)


def posterize(x, bits):
    bits = bits if 0 <= bits <= 8 else 8
    return x & np.uint8((0xFF << (8 - bits)) & 0xFF)


def solarize(x, thr):
    return np.where(x.astype(np.int32) < thr, x, 255 - x).astype(np.uint8)


def autocontrast_lut(h):
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    off = -lo * scale
    return np.array([min(max(int(i * scale + off), 0), 255) for i in range(256)], dtype=np.uint8)


def equalize_lut(h):
    nz = np.nonzero(h)[0]
    ident = np.arange(256, dtype=np.uint8)
    if len(nz) < 2:
        return ident
    step = (int(h.sum()) - int(h[nz[-1]])) // 255
    if step == 0:
        return ident
    before = np.concatenate([[0], np.cumsum(h.astype(np.int64))[:-1]])
    return np.minimum((step // 2 + before) // step, 255).astype(np.uint8)


def _per_channel(x, make_lut):
    return np.stack([make_lut(np.bincount(x[c].ravel(), minlength=256))[x[c]] for c in range(3)])


def autocontrast(x):
    return _per_channel(x, autocontrast_lut)


def equalize(x):
    return _per_channel(x, equalize_lut)


def apply_op(x, op, factor=1.0, param=0, coef=(65536, 0, 32768, 0, 65536, 32768), fill=(0, 0, 0)):
    """One slot of a record on a [3,H,W] window; an id outside the table is skipped."""
    if op == AFFINE:
        return affine(x, coef, fill)
    if op == BRIGHTNESS:
        return brightness(x, factor)
    if op == COLOR:
        return color(x, factor)
    if op == CONTRAST:
        return contrast(x, factor)
    if op == SHARPNESS:
        return sharpness(x, factor)
    if op == POSTERIZE:
        return posterize(x, int(param))
    if op == SOLARIZE:
        return solarize(x, int(param))
    if op == AUTOCONTRAST:
        return autocontrast(x)
    if op == EQUALIZE:
        return equalize(x)
    return x


def window(img, y0, x0, flip, H, W):
    """The crop window of a [3,Hs,Ws] image, corner clamped as calm_augment_collate clamps it, then the flip."""
    _, Hs, Ws = img.shape
    y0, x0 = min(max(int(y0), 0), Hs - H), min(max(int(x0), 0), Ws - W)
    w = img[:, y0:y0 + H, x0:x0 + W]
    return np.ascontiguousarray(w[:, :, ::-1] if flip else w)


def randaugment(img_u8, table, H, W, fill=(0, 0, 0), n_slots=MAX_OPS, stats_mask=0xF):
    """[B,3,H,W] uint8: calm_randaugment_u8 on a [B,3,Hs,Ws] batch and a record table (trainer.DeviceRandAugment's dtype).
    n_slots / stats_mask as the entry point takes them: a sample runs min(n_ops, n_slots) slots, and a statistics
    operation in a slot whose bit is not set is skipped."""
    img_u8 = np.asarray(img_u8)
    out = np.empty((img_u8.shape[0], 3, H, W), dtype=np.uint8)
    for b in range(img_u8.shape[0]):
        r = table[b]
        x = window(img_u8[b], r["y0"], r["x0"], int(r["flip"]) != 0, H, W)
        for k in range(min(max(int(r["n_ops"]), 0), n_slots)):
            op = int(r["op"][k])
            if op in (CONTRAST, AUTOCONTRAST, EQUALIZE) and not (stats_mask >> k) & 1:
                continue
            x = apply_op(x, op, r["factor"][k], r["param"][k], r["coef"][k], fill)
        out[b] = x
    return out


# ---- records ------------------------------------------------------------------------------------------------------------------
IDENT_COEF = (65536, 0, 32768, 0, 65536, 32768)


def slot(op, factor=1.0, param=0, a=None):
    """(op, factor, param, coef): a is the six doubles of a geometric operation."""
    return (op, float(f32(factor)), int(param), fixed_coeffs(a) if a is not None else IDENT_COEF)


def table_of(chains, corners=None, flips=None):
    """The record table of B chains (lists of slot(...) tuples)."""
    from importlib import import_module
    t = import_module("calm_vit_dte_amd.trainer").DeviceRandAugment.identity(len(chains))
    for b, chain in enumerate(chains):
        t["n_ops"][b] = len(chain)
        for k, (op, factor, param, coef) in enumerate(chain):
            t["op"][b, k], t["factor"][b, k], t["param"][b, k], t["coef"][b, k] = op, factor, param, coef
    if corners is not None:
        c = np.asarray(corners)
        t["y0"], t["x0"] = c[:, 0], c[:, 1]
    if flips is not None:
        t["flip"] = np.asarray(flips).astype(np.uint32)
    return t


def every_op(H, W):
    """name -> slot: every operation of the table once, both signs of the signed ones, factors on both sides of 1."""
    return {
        "identity": slot(IDENTITY),
        "shear_x+": slot(AFFINE, a=shear_x(0.23)), "shear_x-": slot(AFFINE, a=shear_x(-0.3)),
        "shear_y+": slot(AFFINE, a=shear_y(0.17)), "shear_y-": slot(AFFINE, a=shear_y(-0.29)),
        "translate_x+": slot(AFFINE, a=translate_x(max(W // 3, 1))), "translate_x-": slot(AFFINE, a=translate_x(-max(W // 4, 1))),
        "translate_y+": slot(AFFINE, a=translate_y(max(H // 3, 1))), "translate_y-": slot(AFFINE, a=translate_y(-max(H // 4, 1))),
        "rotate+": slot(AFFINE, a=rotate(17.0, H, W)), "rotate-": slot(AFFINE, a=rotate(-29.5, H, W)),
        "rotate0": slot(AFFINE, a=rotate(0.0, H, W)), "rotate135": slot(AFFINE, a=rotate(135.0, H, W)),
        "brightness+": slot(BRIGHTNESS, 1.63), "brightness-": slot(BRIGHTNESS, 0.31),
        "color+": slot(COLOR, 1.9), "color-": slot(COLOR, 0.1),
        "contrast+": slot(CONTRAST, 1.45), "contrast-": slot(CONTRAST, 0.55),
        "sharpness+": slot(SHARPNESS, 1.81), "sharpness-": slot(SHARPNESS, 0.19),
        "posterize4": slot(POSTERIZE, param=4), "posterize1": slot(POSTERIZE, param=1), "posterize0": slot(POSTERIZE, param=0),
        "posterize8": slot(POSTERIZE, param=8),
        "solarize": slot(SOLARIZE, param=128), "solarize0": slot(SOLARIZE, param=0), "solarize255": slot(SOLARIZE, param=255),
        "autocontrast": slot(AUTOCONTRAST), "equalize": slot(EQUALIZE),
    }


OP_NAMES = tuple(every_op(8, 8))
WINDOWS = ((1, 1), (2, 2), (3, 3), (7, 5), (17, 33), (64, 48))          # H, W
FILL = (7, 130, 251)


def image(seed, H, W, kind="noise"):
    """[3,H,W] uint8 test images: noise / a low-contrast ramp (autocontrast and equalize move it) / a constant channel /
    two levels."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    if kind == "ramp":
        return (60 + rng.integers(0, 120, (3, H, W)) * np.linspace(0.3, 1.0, W)[None, None, :]).astype(np.uint8)
    if kind == "constant":
        x = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
        x[1] = 93
        return x
    if kind == "two_level":
        return np.where(rng.random((3, H, W)) < 0.3, 40, 200).astype(np.uint8)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def batch(seed, B, Hs, Ws, kind="noise"):
    x = np.stack([image(seed + b, Hs, Ws, kind) for b in range(B)])
    x.setflags(write=False)
    return x
