#!/usr/bin/env python3
"""Time the device resize (calm_resize_u8) on a batch a loader would hand it: B=256 decoded images in a fixed, seeded
ImageNet-like mix of sizes — 500x375, 375x500, 500x333, 333x500 (width x height) and `--big` images of 2048x1536 — packed
by trainer.RaggedU8Collate and resized to 256x256.  Beside it, the host-to-device copy of the same packed batch from
pinned memory and, for scale, the copy of the resized [B,3,256,256] batch the loader would send without the feature: the
packed originals are several times its bytes, and that cost is part of the decision to use this.
Every candidate is measured in `--rounds` alternating rounds in one process (HIP events around `--iters` calls); the table
holds the median and the spread (min .. max) over the rounds.  Compulsory traffic: every source byte read once and every
output byte written once; `fraction_of_hbm_peak` is that traffic over the median time, over 8 TB/s.  Three images of the
batch (a 500x375, a 333x500, a 2048x1536) are compared with the numpy emulation of tests/emulated_resize.py first:
a time for wrong bytes is not reported.  --out FILE writes the result as JSON (profiles/resize_ab.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import calm_vit_dte_amd as calm  # noqa: E402
import emulated_resize as ER  # noqa: E402

HBM_PEAK = 8.0e12               # bytes/s, MI355X
STEP_BUDGET_US = 600.0          # 1 % of the Base-224 autocast step (61 ms at 256 images): the augment pass's yardstick
SIZES = ((375, 500), (500, 375), (333, 500), (500, 333))        # h x w
BIG = (1536, 2048)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters              # us per iteration


def alternate(fns, rounds, iters, warmup):
    out = {k: [] for k in fns}
    for r in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, iters, warmup if r == 0 else 1))
    return out


def summary(us):
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def batch(B, n_big, seed):
    rng = np.random.default_rng(seed)
    shapes = [SIZES[i] for i in rng.integers(0, len(SIZES), B)]
    for i in rng.choice(B, n_big, replace=False):
        shapes[i] = BIG
    return [(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), 0) for h, w in shapes]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--big", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_resize.py times a kernel and copies: it needs the GPU")
    trainer = __import__("importlib").import_module("calm_vit_dte_amd.trainer")
    be = calm.backend.get_backend()
    B, S = args.batch, args.size
    samples = batch(B, args.big, args.seed)
    packed, meta, _ = trainer.RaggedU8Collate()(samples)
    packed = packed.pin_memory()
    dev = packed.cuda()
    records = trainer.DeviceResize.pack(meta, dev.numel(), device="cuda")
    out = torch.empty(B, 3, S, S, dtype=torch.uint8, device="cuda")
    resized_host = torch.empty(B, 3, S, S, dtype=torch.uint8).pin_memory()
    dev2, out2 = torch.empty_like(dev), torch.empty_like(out)

    be.resize_u8(dev, records, out)
    torch.cuda.synchronize()
    shapes = [tuple(m[1:]) for m in meta.tolist()]
    checked = sorted({shapes.index(s) for s in (SIZES[0], SIZES[2], BIG) if s in shapes})
    for i in checked:
        want = ER.resize(samples[i][0], S, S).transpose(2, 0, 1)
        differing = int((out[i].cpu().numpy() != want).sum())
        assert differing == 0, (i, shapes[i], differing)

    fns = {
        "resize_u8": lambda: be.resize_u8(dev, records, out),
        "h2d_packed_originals": lambda: dev2.copy_(packed, non_blocking=True),
        "h2d_resized_batch": lambda: out2.copy_(resized_host, non_blocking=True),
    }
    t = alternate(fns, args.rounds, args.iters, args.warmup)
    read = int(sum(3 * h * w for h, w in shapes))
    written = out.numel()
    result = {"B": B, "size": S, "big": args.big, "seed": args.seed, "iters": args.iters, "rounds": args.rounds,
              "step_budget_us": STEP_BUDGET_US, "source_bytes": read, "packed_bytes": packed.numel(), "output_bytes": written,
              "packed_over_resized_bytes": packed.numel() / written, "images_compared_with_the_emulation": [list(shapes[i]) for i in checked],
              **{n: summary(us) for n, us in t.items()}}
    result["resize_u8"]["fraction_of_hbm_peak"] = (read + written) / (result["resize_u8"]["median_us"] * 1e-6) / HBM_PEAK
    result["resize_u8"]["fraction_of_step_budget"] = result["resize_u8"]["median_us"] / STEP_BUDGET_US
    for n, nbytes in (("h2d_packed_originals", packed.numel()), ("h2d_resized_batch", written)):
        result[n]["gbytes_per_s"] = nbytes / (result[n]["median_us"] * 1e-6) / 1e9
    for n in t:
        print(f"{n:22s} {result[n]['median_us']:9.1f} us ({result[n]['min_us']:.1f} .. {result[n]['max_us']:.1f})", flush=True)
    print(f"resize_u8: {read + written} compulsory bytes, {100 * result['resize_u8']['fraction_of_hbm_peak']:.1f} % of HBM peak, "
          f"{100 * result['resize_u8']['fraction_of_step_budget']:.0f} % of the {STEP_BUDGET_US:.0f} us yardstick; packed / resized "
          f"bytes {result['packed_over_resized_bytes']:.2f}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
