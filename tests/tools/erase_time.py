#!/usr/bin/env python3
"""What does RandomErasing inside the collate kernel cost on the MI355X?

B = 256 uint8 images of 256 x 256, a 224 x 224 window, row tokens out, a DeviceAugment table with the reference's ranges
(every jitter operation, blur on) and MixUp (--mode 1: the partner is needed in every tile) or CutMix (--mode 2):
  augment / augment_again   calm_augment_collate of this tree, timed twice as two variants of its own: their difference
                            and their min .. max over the repeats are the spread every other difference is read against
  parent / parent_again     with --parent-lib PATH (another build of libcalmvit_hip.so, the parent commit's, built from a
                            checkout of it and loaded beside this tree's): its calm_augment_collate on the same tensors —
                            the entry point's ABI is the same — whose output must also equal this tree's bit for bit
  erase_p0 / erase_p25 / erase_p100   calm_augment_collate_erase with the boxes of DeviceErase(p = 0 / 0.25 / 1), noise
                            fill, with the share of output pixels inside a box beside each

Every figure is device time between two events around `--iters` calls, after a warm-up, as the median of `--repeats`
windows with min .. max beside it; the variants alternate inside every repeat, in one process.  The bytes a call has to
move (the uint8 window of the own and the partner sample read, the fp32 batch written) over the median give the achieved
rate.  One JSON line per figure; --out also writes them to a file.  The run stops itself after --limit seconds.  Needs a
GPU."""
import argparse
import ctypes
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests", "tools")):
    sys.path.insert(0, p)
from importlib import import_module  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import calm_vit_dte_amd as calm  # noqa: E402
from optim_groups_time import LINES, emit, windows  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
backend = import_module("calm_vit_dte_amd.backend")
B, HS, H = 256, 256, 224


def measure(args):
    dev = torch.device("cuda", 0)
    be = calm.backend.get_backend()
    gen = torch.Generator(device=dev).manual_seed(0)
    img = torch.randint(0, 256, (B, 3, HS, HS), dtype=torch.uint8, device=dev, generator=gen)
    col, aug = trainer.DeviceCollate(seed=2006), trainer.DeviceAugment(seed=2006)
    corners = col.draw_corners(B, HS, HS, H, H)
    flips = (np.random.default_rng(1).random(B) < 0.5).astype("uint8")
    samples = trainer.DeviceAugment.pack(aug.draw(B), corners, flips, device=dev)
    MEAN, STD = col.MEAN, col.STD
    mode, lam = args.mode, 0.3 if args.mode == 1 else 1.0
    box = (40, 150, 30, 170) if mode == 2 else None
    out = {k: torch.empty(B, H, 3 * H, device=dev) for k in ("augment", "parent", "erase")}
    gm = torch.empty(B, device=dev)
    tables, share = {}, {}
    for name, p in (("erase_p0", 0.0), ("erase_p25", 0.25), ("erase_p100", 1.0)):
        t, key = trainer.DeviceErase(p=p, seed=2006).draw(B, H, H)
        tables[name] = (trainer.DeviceErase.pack(t, device=dev), key)
        share[name] = round(float((t["h"].astype(np.int64) * t["w"]).sum()) / (B * H * H), 4)

    def this_tree():
        be.augment_collate(img, samples, gm, out["augment"], mode, lam, box, MEAN, STD, tokens=True)

    fns = {"augment": this_tree, "parent": None, "augment_again": this_tree, "parent_again": None}      # alternating
    if not args.parent_lib:
        del fns["parent"], fns["parent_again"]
    else:
        other = ctypes.CDLL(os.path.abspath(args.parent_lib))
        other.calm_augment_collate.restype, other.calm_augment_collate.argtypes = binding.SIGNATURES["calm_augment_collate"]
        cbox = (ctypes.c_int32 * 4)(*box) if box is not None else None
        cm, cs = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)

        def parent():
            rc = other.calm_augment_collate(img.data_ptr(), HS, HS, samples.data_ptr(), gm.data_ptr(), out["parent"].data_ptr(),
                                            B, H, H, 1, mode, lam, cbox, cm, cs, backend._stream())
            assert rc == 0, rc
        fns["parent"] = fns["parent_again"] = parent
    for name, (boxes, key) in tables.items():
        fns[name] = (lambda boxes=boxes, key=key: be.augment_collate_erase(img, samples, gm, out["erase"], mode, lam, box, MEAN,
                                                                           STD, boxes, None, key, tokens=True))
    r = windows(fns, args.iters, args.repeats, 20)
    same = None
    if args.parent_lib:
        fns["augment"]()
        fns["parent"]()
        torch.cuda.synchronize()
        same = bool(torch.equal(out["augment"].view(torch.int32), out["parent"].view(torch.int32)))
    fns["erase_p0"]()
    torch.cuda.synchronize()
    p0_same = bool(torch.equal(out["erase"].view(torch.int32), out["augment"].view(torch.int32)))
    us = {k: [round(x, 2) for x in v] for k, v in r.items()}
    base = ("augment", "augment_again") + (("parent", "parent_again") if args.parent_lib else ())
    spread = max([abs(r["augment"][0] - r["augment_again"][0])] + [r[k][2] - r[k][1] for k in base])
    moved = B * 3 * H * H * ((2 if mode == 1 else 1) + 4)          # uint8 windows read (CutMix: the own one), fp32 written
    rec = dict(what="collate with RandomErasing, 256 x 3 x 256 x 256 uint8 -> 256 x 224 x 672 fp32 tokens", mode=mode,
               iters=args.iters, repeats=args.repeats, median_min_max_us=us, spread_us=round(spread, 2), erased_share=share,
               erase_minus_augment_us={k: round(r[k][0] - r["augment"][0], 2) for k in tables}, bytes_moved=moved,
               gb_per_s={k: round(moved / (v[0] * 1e-6) / 1e9, 1) for k, v in r.items()}, erase_p0_equals_augment_bits=p0_same)
    if args.parent_lib:
        rec.update(this_tree_minus_parent_us=round(r["augment"][0] - r["parent"][0], 2),
                   within_spread=bool(abs(r["augment"][0] - r["parent"][0]) <= spread), equals_parent_bits=same)
    emit(**rec)
    assert p0_same and same is not False


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the run stops itself")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--mode", type=int, default=1, choices=(1, 2), help="1 MixUp (lam 0.3), 2 CutMix")
    ap.add_argument("--parent-lib", default=None, metavar="PATH",
                    help="another build of libcalmvit_hip.so whose calm_augment_collate is timed against this tree's")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("erase_time: no GPU — nothing measured")

    def expired(*_):
        print(f"erase_time: stopped after {args.limit} s", flush=True)
        os._exit(3)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(args.limit)
    try:
        emit(what="box", device=torch.cuda.get_device_name(0), torch=torch.__version__)
        measure(args)
    finally:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.writelines(json.dumps(r) + "\n" for r in LINES)


if __name__ == "__main__":
    main()
