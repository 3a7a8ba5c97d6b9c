"""Float64 restatement of calm_augment_collate (include/calm_vit.h) on whole images, in numpy: what the GPU tests compare
the kernel against and what tests/test_augment_cpu.py compares with PIL, colorsys and scipy.  Nothing here follows the
kernel's organisation (tiles, halos, two launches): an operation takes a [3,H,W] image and returns one.

Per sample, on the cropped window, v = u8 / 255:  the jitter operations in the sample's order (brightness, contrast,
saturation, hue), solarize, horizontal flip, grayscale, 3x3 Gaussian blur with reflect padding of the window, Normalize;
then MixUp / CutMix with the partner (b - 1) mod B, which went through the same steps with its own parameters.

`table` is a record array with the fields of struct calm_aug_sample (y0, x0, flags, order, brightness, contrast,
saturation, hue, solarize_thr, blur_sigma); its float32 entries are widened exactly, so the emulation and the kernel
use the same factors and the same threshold."""
import numpy as np

FLIP, SOLARIZE, GRAYSCALE, BLUR = 1, 2, 4, 8
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
GRAY_WEIGHTS = np.array([0.2989, 0.587, 0.114])
NEAR = 1e-5                      # a pre-solarize value this close to the threshold may fall on either side in fp32


def gray(x):
    return np.tensordot(GRAY_WEIGHTS, x, axes=(0, 0))


def blend(a, b, r):
    return np.clip(r * a + (1.0 - r) * b, 0.0, 1.0)


def brightness(x, f):
    return blend(x, 0.0, f)


def contrast(x, f):
    return blend(x, gray(x).mean(), f)


def saturation(x, f):
    return blend(x, gray(x)[None], f)


def rgb_to_hsv(x):
    r, g, b = x
    maxc, minc = x.max(0), x.min(0)
    d = maxc - minc
    flat = d == 0.0
    dd = np.where(flat, 1.0, d)
    s = np.where(flat, 0.0, d / np.where(maxc == 0.0, 1.0, maxc))
    rc, gc, bc = (maxc - r) / dd, (maxc - g) / dd, (maxc - b) / dd
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, 2.0 + rc - bc, 4.0 + gc - rc))
    h = np.where(flat, 0.0, (h / 6.0) % 1.0)
    return np.stack([h, s, maxc])


def hsv_to_rgb(hsv):
    h, s, v = hsv
    i = np.floor(h * 6.0)
    f = h * 6.0 - i
    p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    i = i.astype(np.int64) % 6
    r = np.choose(i, [v, q, p, p, t, v])
    g = np.choose(i, [t, v, v, q, p, p])
    b = np.choose(i, [p, p, t, v, v, q])
    return np.stack([r, g, b])


def hue(x, f):
    hsv = rgb_to_hsv(x)
    hsv[0] = (hsv[0] + f) % 1.0
    return hsv_to_rgb(hsv)


def solarize(x, thr):
    return np.where(x >= thr, 1.0 - x, x)


def grayscale(x):
    return np.repeat(gray(x)[None], 3, axis=0)


def blur_weights(sigma):
    w1 = np.exp(-0.5 / (sigma * sigma))
    return np.array([w1, 1.0, w1]) / (1.0 + 2.0 * w1)


def blur(x, sigma):
    w = blur_weights(sigma)
    H, W = x.shape[1:]
    p = np.pad(x, ((0, 0), (1, 1), (1, 1)), mode="reflect")
    rows = w[0] * p[:, :, 0:W] + w[1] * p[:, :, 1:W + 1] + w[2] * p[:, :, 2:W + 2]
    return w[0] * rows[:, 0:H] + w[1] * rows[:, 1:H + 1] + w[2] * rows[:, 2:H + 2]


JITTER = {BRIGHTNESS: brightness, CONTRAST: contrast, SATURATION: saturation, HUE: hue}
FACTOR = {BRIGHTNESS: "brightness", CONTRAST: "contrast", SATURATION: "saturation", HUE: "hue"}


def augment_sample(img_u8, rec, H, W):
    """One sample up to (not including) Normalize: (image [3,H,W] float64, the contrast mean or 0.0, near [H,W] bool —
    output pixels to which a pre-solarize channel value within NEAR of the threshold contributes)."""
    y0, x0, flags = int(rec["y0"]), int(rec["x0"]), int(rec["flags"])
    x = np.asarray(img_u8)[:, y0:y0 + H, x0:x0 + W].astype(np.float64) / 255.0
    assert x.shape == (3, H, W)
    mean = 0.0
    for op in [int(o) for o in rec["order"]]:
        if op not in JITTER:
            continue
        if op == CONTRAST:
            mean = float(gray(x).mean())
        x = JITTER[op](x, float(rec[FACTOR[op]]))
    near = np.zeros((H, W), dtype=bool)
    if flags & SOLARIZE:
        thr = float(rec["solarize_thr"])
        near = (np.abs(x - thr) <= NEAR).any(0)
        x = solarize(x, thr)
    if flags & FLIP:
        x, near = x[:, :, ::-1], near[:, ::-1]
    if flags & GRAYSCALE:
        x = grayscale(x)
    if flags & BLUR:
        x = blur(x, float(rec["blur_sigma"]))
        p = np.pad(near, 1, mode="reflect")
        near = np.zeros_like(near)
        for dy in range(3):
            for dx in range(3):
                near |= p[dy:dy + H, dx:dx + W]
    return x, mean, near


def augment_collate(img_u8, table, H, W, mode, lam, box, mean, std, tokens=False):
    """(out, gray_mean [B], near): out [B,3,H,W] or [B,H,3W] float64; near in out's layout."""
    img_u8 = np.asarray(img_u8)
    B = img_u8.shape[0]
    m, s = np.asarray(mean, dtype=np.float64)[:, None, None], np.asarray(std, dtype=np.float64)[:, None, None]
    imgs, means, nears = [], [], []
    for b in range(B):
        x, gm, near = augment_sample(img_u8[b], table[b], H, W)
        imgs.append((x - m) / s)
        means.append(gm)
        nears.append(near)
    own, own_near = np.stack(imgs), np.stack(nears)
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
    return out, np.asarray(means), near
