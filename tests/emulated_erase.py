"""Float64 restatement of calm_augment_collate_erase (include/calm_vit.h) in numpy, built on the emulation of the
augmenting collate (emulated_augment.augment_sample) and on the numpy Philox of emulated_dropout: each sample's normalised
image, its box overwritten with the constant or the noise, then the mix.  Nothing follows the kernel's organisation.

It also holds the cases tests/test_erase_gpu.py runs, so that tests/test_erase_cpu.py can check them (the share of
pixels near the solarize threshold) without a GPU."""
import functools

import numpy as np

import emulated_augment as EA
from emulated_dropout import philox4x32_10

_LO, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)           # trainer.DeviceCollate.MEAN / STD


def noise(key, s, H, W):
    """Sample s's standard normal fill over its whole H x W window, [3,H,W] float64: Box-Muller on the four words of
    Philox4x32-10 at counter (lo32(p), hi32(p), lo32(offset), hi32(offset)), p = (s H + y) W + x, key (lo32, hi32 of seed)."""
    seed, offset = (int(k) & (2 ** 64 - 1) for k in key)
    p = ((np.uint64(s * H) + np.arange(H, dtype=np.uint64))[:, None] * np.uint64(W) + np.arange(W, dtype=np.uint64)[None, :])
    z = np.zeros_like(p)
    w = philox4x32_10((p & _LO, p >> _S32, z + np.uint64(offset & 0xFFFFFFFF), z + np.uint64(offset >> 32)),
                      (seed & 0xFFFFFFFF, seed >> 32))
    w = [x.astype(np.float64) for x in (w[0] >> np.uint32(8), w[1] >> np.uint32(8), w[2] >> np.uint32(8), w[3] >> np.uint32(8))]
    u1, u2, u3, u4 = (w[0] + 1.0) * 2.0 ** -24, w[1] * 2.0 ** -24, (w[2] + 1.0) * 2.0 ** -24, w[3] * 2.0 ** -24
    r1, r3 = np.sqrt(-2.0 * np.log(u1)), np.sqrt(-2.0 * np.log(u3))
    return np.stack([r1 * np.cos(2.0 * np.pi * u2), r1 * np.sin(2.0 * np.pi * u2), r3 * np.cos(2.0 * np.pi * u4)])


def fill(value, key, s, H, W):
    """[3,H,W] float64: the constant as the kernel holds it (float32), or the noise (value None)."""
    if value is None:
        return noise(key, s, H, W)
    v = np.asarray(value, dtype=np.float32).astype(np.float64)
    return np.broadcast_to(v[:, None, None], (3, H, W)).copy()


def erased_samples(img_u8, table, boxes, value, key, H, W, mean=MEAN, std=STD):
    """(e [B,3,H,W] float64, gray_mean [B], near [B,H,W] bool, erased [B,H,W] bool): every sample normalised, then its box
    overwritten.  An erased pixel no longer depends on the sample's solarize comparison: it is not `near`."""
    img_u8 = np.asarray(img_u8)
    B = img_u8.shape[0]
    m, s = np.asarray(mean, dtype=np.float64)[:, None, None], np.asarray(std, dtype=np.float64)[:, None, None]
    e, means, nears, masks = [], [], [], []
    for b in range(B):
        x, gm, near = EA.augment_sample(img_u8[b], table[b], H, W)
        x = (x - m) / s
        y0, x0, h, w = (int(boxes[b][f]) for f in ("y", "x", "h", "w"))
        mask = np.zeros((H, W), dtype=bool)
        if h > 0 and w > 0:
            mask[y0:y0 + h, x0:x0 + w] = True
            x[:, y0:y0 + h, x0:x0 + w] = fill(value, key, b, H, W)[:, y0:y0 + h, x0:x0 + w]
            near = near & ~mask
        e.append(x)
        means.append(gm)
        nears.append(near)
        masks.append(mask)
    return np.stack(e), np.asarray(means), np.stack(nears), np.stack(masks)


def mix(own, own_near, mode, lam, box, tokens=False):
    """The batch mix of EA.augment_collate on already erased samples: (out, near) in out's layout."""
    B, _, H, W = own.shape
    oth, oth_near = np.roll(own, 1, axis=0), np.roll(own_near, 1, axis=0)
    if mode == 0:
        out, near = own, own_near
    elif mode == 1:
        out, near = own * lam + oth * (1.0 - lam), own_near | oth_near
    else:
        y1, y2, x1, x2 = box
        out, near = own.copy(), own_near.copy()
        out[:, :, y1:y2, x1:x2] = oth[:, :, y1:y2, x1:x2]
        near[:, y1:y2, x1:x2] = oth_near[:, y1:y2, x1:x2]
    near = np.repeat(near[:, None], 3, axis=1)
    if tokens:
        out = out.transpose(0, 2, 3, 1).reshape(B, H, 3 * W)
        near = near.transpose(0, 2, 3, 1).reshape(B, H, 3 * W)
    return out, near


def erase_collate(img_u8, table, boxes, value, key, H, W, mode, lam, box, mean=MEAN, std=STD, tokens=False):
    """(out, gray_mean [B], near) like EA.augment_collate."""
    e, means, near, _ = erased_samples(img_u8, table, boxes, value, key, H, W, mean, std)
    out, near = mix(e, near, mode, lam, box, tokens)
    return out, means, near


# ---- the cases of tests/test_erase_gpu.py ------------------------------------------------------------------------------
# A workgroup's tile is 16 x 64 output pixels and a thread owns 4 pixels of a row.  19 x 70: ragged tiles both ways, and
# W % 4 != 0 takes the scalar stores; 32 x 64: the 16-byte stores.  B = 3: sample 0's partner is sample 2.
SHAPES = {"19x70": (24, 80, 19, 70), "32x64": (40, 72, 32, 64)}      # Hs, Ws, H, W
CUTMIX = {"19x70": (2, 17, 8, 66), "32x64": (2, 17, 8, 62)}          # y1, y2, x1, x2: through own and partner boxes
KEY = (0x9E3779B97F4A7C15, 0xD1B54A32D192ED03)                      # both halves of seed and offset in use
VALUE = (0.1, -0.7, 1.3)                                             # none of them a float32
B = 3
THR = np.float32(223.5 / 255.0)


def box_sets(H, W):
    """name -> [B] (y, x, h, w): none / across row 16 and column 64 (where the window has one) / x % 4 != 0 and
    w % 4 != 0; 1 x 1 / anchored at (0, 0) / anchored at (H - h, W - w); (H - 1) x (W - 1) at both corners / none."""
    cross = (10, 60, 8, 8) if W > 64 else (10, 50, 8, 9)
    return {"none_cross_odd": [(0, 0, 0, 0), cross, (3, 5, 7, 10)],
            "one_first_last": [(7, 9, 1, 1), (0, 0, 5, 11), (H - 6, W - 13, 6, 13)],
            "nearly_all": [(0, 0, H - 1, W - 1), (1, 1, H - 1, W - 1), (0, 0, 0, 3)]}


BOX_SETS = tuple(box_sets(19, 70))


def boxes_of(recs):
    from importlib import import_module
    t = import_module("calm_vit_dte_amd.trainer").DeviceErase.identity(len(recs))
    for b, r in enumerate(recs):
        t[b] = r
    return t


def varied_table(seed, n, Hs, Ws, H, W):
    """Every sample with its own factors, corner and order: all four jitter operations, blur on, solarize / flip /
    grayscale alternating over the samples (the records of test_augment_gpu.varied_table)."""
    from importlib import import_module
    rng = np.random.default_rng(seed)
    t = import_module("calm_vit_dte_amd.trainer").DeviceAugment.identity(n)
    t["y0"], t["x0"] = rng.integers(0, Hs - H + 1, n), rng.integers(0, Ws - W + 1, n)
    t["solarize_thr"] = THR
    t["order"] = rng.permuted(np.tile(np.arange(4, dtype=np.uint8), (n, 1)), axis=1)
    for name in ("brightness", "contrast", "saturation"):
        t[name] = rng.uniform(0.5, 1.0, n)
    t["hue"] = rng.uniform(-0.125, 0.125, n)
    t["blur_sigma"] = rng.uniform(0.1, 2.0, n)
    b = np.arange(n)
    t["flags"] = (EA.BLUR | np.where(b % 2 == 1, EA.SOLARIZE, 0) | np.where(b % 3 == 0, EA.FLIP, 0)
                  | np.where(b % 5 == 2, EA.GRAYSCALE, 0)).astype(np.uint32)
    return t


def source(seed, n, Hs, Ws):
    return np.random.default_rng(seed).integers(0, 256, (n, 3, Hs, Ws), dtype=np.uint8)


SEEDS = {"19x70": (70, 71), "32x64": (72, 73)}                       # source, table


@functools.lru_cache(maxsize=None)
def case_inputs(shape):
    """(src, table, H, W) of a shape: shared by every case on it, never modified."""
    Hs, Ws, H, W = SHAPES[shape]
    src, t = source(SEEDS[shape][0], B, Hs, Ws), varied_table(SEEDS[shape][1], B, Hs, Ws, H, W)
    src.setflags(write=False)
    t.setflags(write=False)
    return src, t, H, W


@functools.lru_cache(maxsize=None)
def case_samples(shape, boxset, noise_fill):
    """The erased samples of a case, computed once: (e, gray_mean, near, erased, boxes)."""
    src, t, H, W = case_inputs(shape)
    boxes = boxes_of(box_sets(H, W)[boxset])
    out = erased_samples(src, t, boxes, None if noise_fill else VALUE, KEY, H, W) + (boxes,)
    for a in out:
        a.setflags(write=False)
    return out


MODES = {0: (0, 1.0), 1: (1, 0.3), 2: (2, 1.0)}                      # mode -> (mode, lam)


def case_reference(shape, boxset, noise_fill, mode, tokens):
    """(out, gray_mean, near, erased in out's layout) of one GPU case."""
    e, gm, near, erased, _ = case_samples(shape, boxset, noise_fill)
    m, lam = MODES[mode]
    out, near = mix(e, near, m, lam, CUTMIX[shape] if m == 2 else None, tokens)
    return out, gm, near


CASES = [(shape, boxset, noise_fill) for shape in SHAPES for boxset in BOX_SETS for noise_fill in (False, True)]
