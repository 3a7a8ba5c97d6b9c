"""numpy restatement of calm_resize_u8 / calm_resize_coeffs (include/calm_vit.h): PIL's Image.resize(size, BILINEAR) on an
8-bit RGB image — a horizontal and then a vertical antialiased pass, the intermediate rounded to uint8, coefficients in
double converted to 22-bit fixed point.  What the GPU tests compare the kernel with, bit for bit; tests/test_resize_cpu.py
compares this file with PIL itself.

Every floating-point step below is one IEEE double operation in the order of the header's formulas; the weight sum is
taken in tap order (np.cumsum adds sequentially, np.sum does not)."""
import numpy as np

PRECISION_BITS = 22

# source h x w -> output h x w: a single tap, upscaling, identity, n clamped at both edges, tall and wide extremes
CASES = [((1, 1), (8, 8)), ((2, 3), (8, 8)), ((7, 5), (8, 8)), ((8, 8), (8, 8)), ((9, 8), (8, 8)), ((13, 29), (8, 8)),
         ((8, 31), (8, 16)), ((37, 64), (16, 16)), ((100, 75), (16, 24)), ((333, 500), (256, 256)),
         ((500, 375), (256, 256)), ((256, 256), (256, 256)), ((255, 257), (256, 256)), ((1200, 37), (32, 32)),
         ((64, 2049), (16, 16)), ((3, 700), (256, 256))]
# the sources of the ragged GPU batch: every case's source that is small enough to sit in one
SMALL_SOURCES = [(1, 1), (2, 3), (7, 5), (8, 8), (9, 8), (13, 29), (8, 31), (37, 64), (100, 75), (255, 257), (1200, 37),
                 (64, 2049), (3, 700)]


def image(seed, h, w):
    """Seeded random RGB [h, w, 3] uint8 with saturated blocks in the top half: columns of 0 and of 255 side by side, so
    the clamp at both ends of the 8-bit range and the largest accumulator are met."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    top = (h + 1) // 2
    a[:top, : w // 3] = 0
    a[:top, w // 3: 2 * (w // 3)] = 255
    return a


def coeffs(n_in, n_out):
    """lo [out], n [out] and k [out, ksize] int64 (zero past n), ksize = 2 ceil(max(in / out, 1)) + 1."""
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    ksize = 2 * (-(-n_in // n_out) if n_in > n_out else 1) + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)            # astype truncates toward zero, as (int)
    hi = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    n = hi - lo
    assert n.max() <= ksize
    j = np.arange(ksize, dtype=np.int64)[None, :]
    t = np.abs(((j + lo[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where((t < 1.0) & (j < n[:, None]), 1.0 - t, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                                        # the zeros past n add nothing
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    k = (0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64)
    k[j >= n[:, None]] = 0
    return lo, n, k


def _pass(src, n_out, axis):
    """One pass along `axis` of an integer array [h, w, 3] holding 8-bit levels."""
    src = np.moveaxis(src, axis, 0).astype(np.int64)
    lo, n, k = coeffs(src.shape[0], n_out)
    out = np.empty((n_out,) + src.shape[1:], dtype=np.int64)
    for o in range(n_out):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k[o, :n[o]], src[lo[o]:lo[o] + n[o]], axes=(0, 0))
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, oh, ow):
    """uint8 [h, w, 3] -> uint8 [oh, ow, 3]: horizontal pass, rounded to 8 bits, then the vertical pass."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    return _pass(_pass(img, ow, 1), oh, 0).astype(np.uint8)


def resize_batch(imgs, oh, ow):
    """A list of [h, w, 3] images -> uint8 [B, 3, oh, ow], the kernel's output layout."""
    return np.ascontiguousarray(np.stack([resize(a, oh, ow).transpose(2, 0, 1) for a in imgs]))


def pack(imgs, pad=None):
    """The images' bytes one after the other.  pad: bytes of filler (value 0xA5) in front of image b, cycling through the
    sequence — (1, 2, 3) puts the images at odd offsets; None pads each start to a multiple of 16.  -> packed uint8 [N],
    meta int64 [B, 3] of (offset, h, w)."""
    chunks, meta, end = [], [], 0
    for b, a in enumerate(imgs):
        fill = (-end) % 16 if pad is None else pad[b % len(pad)]
        chunks.append(np.full(fill, 0xA5, dtype=np.uint8))
        meta.append((end + fill, a.shape[0], a.shape[1]))
        chunks.append(np.ascontiguousarray(a).reshape(-1))
        end += fill + a.size
    return np.concatenate(chunks), np.asarray(meta, dtype=np.int64)
