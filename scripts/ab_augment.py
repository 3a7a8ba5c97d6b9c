#!/usr/bin/env python3
"""Time the augmenting collate (calm_augment_collate: a stats launch and the fused launch) next to the plain collate it
extends (calm_collate_crop_mix) at the reference's shapes: B=256, 256x256 source, 224x224 crop, row-token output, MixUp
(mode 1) and CutMix (mode 2).  The augment table is drawn by trainer.DeviceAugment with the reference's ranges (all four
jitter operations, solarize p=0.5, grayscale p=0.1, blur on); `identity` is the same kernel with an empty table.
Every candidate is measured in `--rounds` alternating rounds in one process (HIP events around `--iters` launches); the
table holds the median and the spread (min .. max) over the rounds.  Compulsory traffic: the uint8 windows read once per
use (own and, where the mix needs it, partner) and the fp32 batch written once; `fraction_of_hbm_peak` is that traffic
over the median time, over 8 TB/s.  --out FILE writes the result as JSON (profiles/augment_ab.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import calm_vit_dte_amd as calm  # noqa: E402

HBM_PEAK = 8.0e12               # bytes/s, MI355X
STEP_BUDGET_US = 600.0          # 1 % of the Base-224 autocast step (61 ms at 256 images)


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


def compulsory_bytes(B, H, W, mode, box):
    """uint8 window pixels read (own + the partner's where the mix uses it) and fp32 output written."""
    partner = {0: 0, 1: H * W, 2: 0 if box is None else (box[1] - box[0]) * (box[3] - box[2])}[mode]
    read = 3 * B * (H * W + partner)
    return read, 4 * 3 * B * H * W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--source", type=int, default=256)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_augment.py times kernels: it needs the GPU")
    trainer = __import__("importlib").import_module("calm_vit_dte_amd.trainer")
    be = calm.backend.get_backend()
    B, Hs, S = args.batch, args.source, args.crop
    rng = np.random.default_rng(0)
    u8 = torch.from_numpy(rng.integers(0, 256, (B, 3, Hs, Hs), dtype=np.uint8)).cuda()
    corners = np.stack([rng.integers(0, Hs - S + 1, B), rng.integers(0, Hs - S + 1, B)], axis=1).astype(np.int32)
    flips = torch.from_numpy((rng.random(B) < 0.5).astype(np.uint8))
    corners_dev, flips_dev = torch.from_numpy(corners).cuda(), flips.cuda()
    table = trainer.DeviceAugment(seed=0).draw(B)
    full = trainer.DeviceAugment.pack(table, corners, flips, device="cuda")
    ident = trainer.DeviceAugment.pack(trainer.DeviceAugment.identity(B), corners, flips, device="cuda")
    out_p, out_a = (torch.empty(B, S, 3 * S, device="cuda") for _ in range(2))
    gm = torch.empty(B, device="cuda")
    mean, std = trainer.DeviceCollate.MEAN, trainer.DeviceCollate.STD
    box_full = trainer.SoftMixCollate.cutmix_box(0.5, S // 2, S // 2, S, S)[0]       # lam 0.5: half the area, centred
    result = {"B": B, "source": Hs, "crop": S, "iters": args.iters, "rounds": args.rounds, "step_budget_us": STEP_BUDGET_US,
              "cases": []}
    for mode, lam, box in ((1, 0.3, None), (2, 0.5, box_full)):
        fns = {
            "collate_crop_mix": lambda: be.collate_crop_mix(u8, corners_dev, flips_dev, out_p, mode, lam, box, mean, std, tokens=True),
            "augment_collate": lambda: be.augment_collate(u8, full, gm, out_a, mode, lam, box, mean, std, tokens=True),
            "augment_collate_identity": lambda: be.augment_collate(u8, ident, gm, out_a, mode, lam, box, mean, std, tokens=True),
        }
        t = alternate(fns, args.rounds, args.iters, args.warmup)
        fns["collate_crop_mix"]()
        fns["augment_collate_identity"]()
        torch.cuda.synchronize()
        same = (out_a - out_p).abs().max().item()
        assert same <= 1e-6, same                              # the identity table computes the plain collate
        read, written = compulsory_bytes(B, S, S, mode, box)
        row = {"mode": mode, "lam": lam, "box": box, "bytes_read": read, "bytes_written": written,
               "identity_vs_plain_max_abs": same, **{n: summary(us) for n, us in t.items()}}
        for n in t:
            row[n]["fraction_of_hbm_peak"] = (read + written) / (row[n]["median_us"] * 1e-6) / HBM_PEAK
        row["augment_over_plain"] = row["augment_collate"]["median_us"] / row["collate_crop_mix"]["median_us"]
        row["augment_fraction_of_step_budget"] = row["augment_collate"]["median_us"] / STEP_BUDGET_US
        result["cases"].append(row)
        print(f"mode {mode}: " + "   ".join(
            f"{n} {row[n]['median_us']:8.1f} us ({row[n]['min_us']:.1f} .. {row[n]['max_us']:.1f}, "
            f"{100 * row[n]['fraction_of_hbm_peak']:.1f} % of HBM peak)" for n in t) +
            f"   augment/plain {row['augment_over_plain']:.2f}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
