"""Mints tests/golden/golden_resize_pil.npz: what PIL's Image.resize(size, BILINEAR) returns, recorded, so that the kernel
and the emulation are held to PIL's bytes wherever the suite runs.  Needs numpy and PIL only.

  python tests/golden/make_golden_resize.py

Contents, for case i of the first nine cases of emulated_resize.CASES (1x1 -> 8x8 ... 100x75 -> 16x24):
  src_i  uint8 [h, w, 3]   the seeded input (emulated_resize.image(SEED + i, h, w))
  out_i  uint8 [oh, ow, 3] PIL's output
and for the two 500x375 -> 256x256 inputs of seeds BIG_SEEDS (regenerated from the seed: 562 KB each is too large to keep)
  big_0  uint8 [32, 32, 3] the top-left corner of PIL's output,  big_1  the bottom-right corner.
  pil_version."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import emulated_resize as ER  # noqa: E402

SEED = 4100
N_SMALL = 9
BIG_SEEDS = (4200, 4201)
BIG_SRC, BIG_OUT = (500, 375), (256, 256)
PATH = os.path.join(HERE, "golden_resize_pil.npz")


def pil_resize(a, oh, ow):
    return np.asarray(Image.fromarray(a, "RGB").resize((ow, oh), Image.BILINEAR))


def big_corner(i, out):
    return out[:32, :32] if i == 0 else out[-32:, -32:]


def main():
    data = {"pil_version": np.array(PIL.__version__)}
    for i, ((h, w), (oh, ow)) in enumerate(ER.CASES[:N_SMALL]):
        src = ER.image(SEED + i, h, w)
        data[f"src_{i}"] = src
        data[f"out_{i}"] = pil_resize(src, oh, ow)
    for i, seed in enumerate(BIG_SEEDS):
        data[f"big_{i}"] = big_corner(i, pil_resize(ER.image(seed, *BIG_SRC), *BIG_OUT))
    np.savez_compressed(PATH, **data)
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
