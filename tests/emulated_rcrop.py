"""numpy restatement of calm_resized_crop (include/calm_vit.h): crop the box, resize it with the emulation of
tests/emulated_resize.py (PIL's Image.resize(size, BILINEAR), horizontal pass then vertical pass), keep the window — i.e.
`emulated_resize.resize(img[box], vh, vw)[window]` — plus n(v) = (v / 255 - mean) / std in float64 for the fp32 kinds.
What the GPU tests compare the kernel with; tests/test_rcrop_cpu.py compares this file with PIL's crop().resize()."""
import numpy as np

import emulated_resize as ER

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)        # trainer.DeviceCollate's

# (source h x w, box (by0, bx0, bh, bw), size (vh, vw), window (wy0, wx0, H, W)) — every box within an aspect of 16:
# a 1x1 box upscaled; an odd bx0; a box at each corner of the source (up, one axis up and the other down, the identity
# size, down); the identity on a whole image; the .center(256, (224, 224)) records of 500x375, 375x500 and 333x500; two
# more boxes with odd corners; a single pixel
CASES = [
    ((9, 9), (4, 4, 1, 1), (8, 8), (0, 0, 8, 8)),
    ((37, 53), (3, 5, 27, 36), (17, 24), (0, 0, 17, 24)),
    ((40, 33), (0, 0, 10, 12), (16, 16), (1, 3, 8, 8)),
    ((40, 33), (0, 21, 10, 12), (7, 20), (0, 0, 7, 20)),
    ((40, 33), (30, 0, 10, 12), (10, 12), (0, 0, 10, 12)),
    ((40, 33), (30, 21, 10, 12), (5, 6), (1, 1, 4, 4)),
    ((19, 23), (0, 0, 19, 23), (19, 23), (2, 3, 8, 8)),
    ((500, 375), (0, 0, 500, 375), (341, 256), (58, 16, 224, 224)),
    ((375, 500), (0, 0, 375, 500), (256, 341), (16, 58, 224, 224)),
    ((333, 500), (0, 0, 333, 500), (256, 384), (16, 80, 224, 224)),
    ((100, 75), (11, 7, 64, 40), (24, 24), (3, 5, 16, 16)),
    ((64, 300), (2, 9, 60, 290), (32, 48), (0, 0, 32, 48)),
    ((1, 1), (0, 0, 1, 1), (8, 8), (0, 0, 8, 8)),
]
CENTER_CASES = (7, 8, 9)                                        # the three .center records above
SEED = 5100                                                     # case i's source is emulated_resize.image(SEED + i, h, w)


def source(i):
    return ER.image(SEED + i, *CASES[i][0])


def rcrop(img, box, size, window):
    """uint8 [h, w, 3] -> uint8 [H, W, 3]: resize(img[box], vh, vw)[window]."""
    by0, bx0, bh, bw = box
    wy0, wx0, H, W = window
    assert 0 <= by0 and 0 <= bx0 and bh >= 1 and bw >= 1 and by0 + bh <= img.shape[0] and bx0 + bw <= img.shape[1]
    assert 0 <= wy0 and 0 <= wx0 and wy0 + H <= size[0] and wx0 + W <= size[1]
    full = ER.resize(np.ascontiguousarray(img[by0:by0 + bh, bx0:bx0 + bw]), size[0], size[1])
    return np.ascontiguousarray(full[wy0:wy0 + H, wx0:wx0 + W])


def rcrop_batch(imgs, records, H, W):
    """records: (image index, box, size, (wy0, wx0)) -> uint8 [B, 3, H, W], the layout of out_kind 0."""
    return np.ascontiguousarray(np.stack([rcrop(imgs[i], box, size, (wy0, wx0, H, W)).transpose(2, 0, 1)
                                          for i, box, size, (wy0, wx0) in records]))


def normalise(u8, mean=MEAN, std=STD):
    """uint8 [B, 3, H, W] -> float64 [B, 3, H, W], n(v) = (v / 255 - mean[c]) / std[c] (out_kind 1)."""
    m, s = (np.asarray(v, dtype=np.float64).reshape(1, 3, 1, 1) for v in (mean, std))
    return (u8.astype(np.float64) / 255.0 - m) / s


def normalise_f32(u8, mean=MEAN, std=STD):
    """uint8 [B, 3, H, W] -> float32 [B, 3, H, W]: the header's fp32 evaluation, fma(v, 1 / 255, -mean) * (1 / std) with mean,
    std and 1 / 255 rounded to float32.  v * (1 / 255) - mean is exact in float64 (8 x 24 bits, then a sum within 2^-31 .. 1),
    so rounding it to float32 once is the fused multiply-add."""
    m, s = (np.asarray(v, dtype=np.float32).reshape(1, 3, 1, 1) for v in (mean, std))
    c = np.float32(1.0) / np.float32(255.0)
    fma = (u8.astype(np.float64) * np.float64(c) - m.astype(np.float64)).astype(np.float32)
    return fma * (np.float32(1.0) / s)


def tokens(image):
    """[B, 3, H, W] -> [B, H, 3W], out[b, i, 3j + c] = image[b, c, i, j] (out_kind 2)."""
    B, _, H, W = image.shape
    return np.ascontiguousarray(image.transpose(0, 2, 3, 1)).reshape(B, H, 3 * W)
