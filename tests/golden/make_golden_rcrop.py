"""Mints tests/golden/golden_rcrop_pil.npz: what PIL's Image.crop(box).resize(size, BILINEAR) returns, sliced to the output
window, recorded, so that the emulation of calm_resized_crop is held to PIL's bytes wherever the suite runs.  Needs numpy
and PIL only.

  python tests/golden/make_golden_rcrop.py

Contents, for case i of emulated_rcrop.CASES (source emulated_resize.image(SEED + i, h, w), regenerated from the seed):
  out_i  uint8 [H, W, 3]   the window of PIL's output; of a window above 4096 pixels (150 KB each is too large to keep)
                           its top-left and bottom-right 32 x 32 corners, [2, 32, 32, 3] (kept())
  src_i  uint8 [h, w, 3]   the seeded input, kept for the sources of at most 4096 pixels
  pil_version."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import emulated_rcrop as EC  # noqa: E402

PATH = os.path.join(HERE, "golden_rcrop_pil.npz")
SRC_KEPT_PIXELS = 4096


def pil_rcrop(a, box, size, window):
    """crop((bx0, by0, bx0 + bw, by0 + bh)).resize((vw, vh), BILINEAR), sliced to the window."""
    by0, bx0, bh, bw = box
    wy0, wx0, H, W = window
    out = np.asarray(Image.fromarray(a).crop((bx0, by0, bx0 + bw, by0 + bh)).resize((size[1], size[0]), Image.BILINEAR))
    return np.ascontiguousarray(out[wy0:wy0 + H, wx0:wx0 + W])


def pil_resize_box(a, box, size, window):
    """Image.resize(size, BILINEAR, box=box): NOT the contract — it reads pixels around the box."""
    by0, bx0, bh, bw = box
    wy0, wx0, H, W = window
    out = np.asarray(Image.fromarray(a).resize((size[1], size[0]), Image.BILINEAR, box=(bx0, by0, bx0 + bw, by0 + bh)))
    return np.ascontiguousarray(out[wy0:wy0 + H, wx0:wx0 + W])


def kept(out):
    """What the golden holds of a window: all of it, or its two 32 x 32 corners when it has more than 4096 pixels."""
    if out.shape[0] * out.shape[1] <= SRC_KEPT_PIXELS:
        return out
    return np.stack([out[:32, :32], out[-32:, -32:]])


def main():
    data = {"pil_version": np.array(PIL.__version__)}
    for i, ((h, w), box, size, window) in enumerate(EC.CASES):
        src = EC.source(i)
        if h * w <= SRC_KEPT_PIXELS:
            data[f"src_{i}"] = src
        data[f"out_{i}"] = kept(pil_rcrop(src, box, size, window))
    np.savez_compressed(PATH, **data)
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
