#!/usr/bin/env python3
"""Time the device resized crop (calm_resized_crop) on ab_resize.py's batch: B=256 decoded images in the seeded
ImageNet-like mix of sizes (500x375, 375x500, 500x333, 333x500 and `--big` images of 2048x1536), packed by
trainer.RaggedU8Collate.  Three uses, each held to the 0.6 ms yardstick of the augment and resize passes (1 % of the 61 ms
Base-224 autocast step):
  center_tokens        DeviceResizedCrop.center(256, (224, 224)), out="tokens": the validation input in one launch
  random_resized_u8    DeviceResizedCrop.random_resized((224, 224)), uint8 for the collate
  window_u8            DeviceResizedCrop.window((256, 256), (224, 224)), uint8 for the collate
and, beside them, what the windowed form replaces and becomes:
  resize_u8_256                 calm_resize_u8 to 256x256, every pixel
  resize_then_collate           calm_resize_u8 to 256x256 + calm_collate_crop_mix (mode 0, the same corners, tokens)
  window_tokens                 the window as tokens in one launch (no uint8 round trip)
  window_u8_then_collate        the window as uint8 + calm_collate_crop_mix (mode 0, no crop, tokens): train()'s form
--parent-lib FILE runs the two calm_resize_u8 / calm_collate_crop_mix arms through another build of the library (the
parent commit's), loaded into the same process, so that the comparison is against the code the feature replaces.
Every candidate is measured in `--rounds` alternating rounds in one process (HIP events around `--iters` calls); the table
holds the median and the spread (min .. max) over the rounds.  Three images of the batch are compared with the numpy
emulation of tests/emulated_rcrop.py for each of the three uses first, and window_tokens with resize_then_collate: a time
for wrong bytes is not reported.  --out FILE writes the result as JSON (profiles/rcrop_ab.json)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import calm_vit_dte_amd as calm  # noqa: E402
import emulated_rcrop as EC  # noqa: E402
from ab_resize import BIG, SIZES, STEP_BUDGET_US, alternate, batch, summary  # noqa: E402


def two_launch_arm(lib_path):
    """(resize_u8, collate_crop_mix) as plain calls into the library at lib_path — this build's when it is empty."""
    binding = __import__("importlib").import_module("calm_vit_dte_amd._lib")
    lib = binding.load() if not lib_path else C.CDLL(lib_path)
    if lib_path:
        for name in ("calm_resize_u8", "calm_collate_crop_mix"):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = binding.SIGNATURES[name]
    mean, std = (C.c_float * 3)(*EC.MEAN), (C.c_float * 3)(*EC.STD)

    def resize(dev, records, out):
        B, _, oh, ow = out.shape
        rc = lib.calm_resize_u8(dev.data_ptr(), dev.numel(), records.data_ptr(), out.data_ptr(), B, oh, ow,
                                torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def collate(img, corners, out):
        B, _, Hs, Ws = img.shape
        H, W = out.shape[1], out.shape[2] // 3
        rc = lib.calm_collate_crop_mix(img.data_ptr(), Hs, Ws, corners.data_ptr() if corners is not None else None, None,
                                       out.data_ptr(), B, H, W, 1, 0, 1.0, None, mean, std,
                                       torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    return resize, collate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--big", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_rcrop.py times kernels: it needs the GPU")
    trainer = __import__("importlib").import_module("calm_vit_dte_amd.trainer")
    DRC = trainer.DeviceResizedCrop
    be = calm.backend.get_backend()
    B, S, Hc = args.batch, 256, 224
    samples = batch(B, args.big, args.seed)
    packed, meta, _ = trainer.RaggedU8Collate()(samples)
    dev = packed.cuda()
    shapes = [tuple(m[1:]) for m in meta.tolist()]
    checked = sorted({shapes.index(s) for s in (SIZES[0], SIZES[2], BIG) if s in shapes})
    rng = np.random.default_rng(args.seed + 1)
    corners_host = np.stack([rng.integers(0, S - Hc + 1, B), rng.integers(0, S - Hc + 1, B)], axis=1).astype(np.int32)
    corners = torch.from_numpy(corners_host).cuda()

    uses = {"center": DRC.center(S, (Hc, Hc)), "random_resized": DRC.random_resized((Hc, Hc), seed=args.seed),
            "window": DRC.window((S, S), (Hc, Hc))}
    rec = {k: u.pack(meta, dev.numel(), corners_host if k == "window" else None, device="cuda") for k, u in uses.items()}
    u8 = torch.empty(B, 3, Hc, Hc, dtype=torch.uint8, device="cuda")
    tok, tok2 = (torch.empty(B, Hc, 3 * Hc, dtype=torch.float32, device="cuda") for _ in range(2))
    whole = torch.empty(B, 3, S, S, dtype=torch.uint8, device="cuda")
    records_whole = trainer.DeviceResize.pack(meta, dev.numel(), device="cuda")
    resize, collate = two_launch_arm(args.parent_lib)

    # the bytes first: three images per use against the emulation, and the one-launch tokens against the two launches
    for k, u in uses.items():
        be.resized_crop(dev, rec[k], u8)
        got = u8.cpu().numpy()
        t = u.last_records
        for i in checked:
            box = tuple(int(t[i][f]) for f in ("by0", "bx0", "bh", "bw"))
            want = EC.rcrop(samples[i][0], box, (int(t[i]["vh"]), int(t[i]["vw"])), (int(t[i]["wy0"]), int(t[i]["wx0"]), Hc, Hc))
            differing = int((got[i] != want.transpose(2, 0, 1)).sum())
            assert differing == 0, (k, i, shapes[i], differing)
    be.resized_crop(dev, rec["window"], tok, EC.MEAN, EC.STD, tokens=True)
    resize(dev, records_whole, whole)
    collate(whole, corners, tok2)
    torch.cuda.synchronize()
    window_vs_two = float((tok - tok2).abs().max())

    def window_then_collate():
        be.resized_crop(dev, rec["window"], u8)
        collate(u8, None, tok2)

    def resize_then_collate():
        resize(dev, records_whole, whole)
        collate(whole, corners, tok2)

    fns = {
        "center_tokens": lambda: be.resized_crop(dev, rec["center"], tok, EC.MEAN, EC.STD, tokens=True),
        "random_resized_u8": lambda: be.resized_crop(dev, rec["random_resized"], u8),
        "window_u8": lambda: be.resized_crop(dev, rec["window"], u8),
        "resize_u8_256": lambda: resize(dev, records_whole, whole),
        "resize_then_collate": resize_then_collate,
        "window_tokens": lambda: be.resized_crop(dev, rec["window"], tok, EC.MEAN, EC.STD, tokens=True),
        "window_u8_then_collate": window_then_collate,
    }
    t = alternate(fns, args.rounds, args.iters, args.warmup)
    result = {"B": B, "resize": S, "crop": Hc, "big": args.big, "seed": args.seed, "iters": args.iters, "rounds": args.rounds,
              "step_budget_us": STEP_BUDGET_US, "packed_bytes": packed.numel(),
              "two_launch_arm_library": "the build given as --parent-lib" if args.parent_lib else "this build",
              "images_compared_with_the_emulation": [list(shapes[i]) for i in checked],
              "window_tokens_vs_resize_then_collate_max_abs": window_vs_two,
              "random_resized_fallbacks": int(uses["random_resized"].last_fallback.sum()),
              **{n: summary(us) for n, us in t.items()}}
    for n in ("center_tokens", "random_resized_u8", "window_u8"):
        result[n]["fraction_of_step_budget"] = result[n]["median_us"] / STEP_BUDGET_US
    result["window_tokens_over_resize_then_collate"] = result["window_tokens"]["median_us"] / result["resize_then_collate"]["median_us"]
    result["window_u8_then_collate_over_resize_then_collate"] = (result["window_u8_then_collate"]["median_us"]
                                                                 / result["resize_then_collate"]["median_us"])
    result["window_u8_over_resize_u8_256"] = result["window_u8"]["median_us"] / result["resize_u8_256"]["median_us"]
    for n in t:
        print(f"{n:24s} {result[n]['median_us']:9.1f} us ({result[n]['min_us']:.1f} .. {result[n]['max_us']:.1f})", flush=True)
    print(f"one-launch window tokens against resize + collate: max |difference| {window_vs_two:.3g}; "
          f"time ratio {result['window_tokens_over_resize_then_collate']:.3f}", flush=True)
    inside = all(result[n]["median_us"] <= STEP_BUDGET_US for n in ("center_tokens", "random_resized_u8", "window_u8"))
    print(f"the three uses are {'inside' if inside else 'OUTSIDE'} the {STEP_BUDGET_US:.0f} us yardstick", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    if not inside:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
