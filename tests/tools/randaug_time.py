#!/usr/bin/env python3
"""What does the device RandAugment stage cost on the MI355X, and what does the same chain cost in PIL on the host?

B = 256 uint8 images of 256 x 256, a 224 x 224 window with random corners and flips, two operations per sample at
magnitude 9 of 31 (DeviceRandAugment's defaults), the table drawn once:
  stage        calm_randaugment_u8 on that table: device time between two events around `--iters` calls after a warm-up,
               the median of `--repeats` windows with min .. max beside it (the launches: an apply pass per slot and, in
               front of a slot in which some sample needs statistics, a memset and a statistics pass);
  stage_geometric / stage_statistics   the same with the operations restricted to the five warps / to Contrast,
               AutoContrast and Equalize: the cheapest and the dearest mix;
  crop_flip    num_ops = 0: the one copy pass, the floor of the stage;
  pil_host     the same table through PIL on `--threads` host threads (crop, transpose, the chain, np.asarray): wall time
               per batch, best of 3; the output must equal the stage's byte for byte.
One JSON line per figure; --out also writes them to a file.  The run stops itself after --limit seconds.  Needs a GPU.  No
threshold is set: the figures are reported."""
import argparse
import json
import os
import signal
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests", "tools")):
    sys.path.insert(0, p)
from importlib import import_module  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import calm_vit_dte_amd as calm  # noqa: E402
from optim_groups_time import LINES, emit, windows  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
DRA = trainer.DeviceRandAugment
B, HS, H = 256, 256, 224
GEOMETRIC = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
STATISTICS = ("Contrast", "AutoContrast", "Equalize")


def pil_chain(src, table, names, values, fill, threads):
    """The table's chains through PIL, one image per task on `threads` threads: [B,3,H,H] uint8."""
    from PIL import Image
    from test_randaug_cpu import pil_op

    def one(b):
        y0, x0 = int(table["y0"][b]), int(table["x0"][b])
        im = Image.fromarray(src[b]).crop((x0, y0, x0 + H, y0 + H))
        if table["flip"][b]:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        for name, v in zip(names[b], values[b]):
            im = pil_op(im, name, v, fill)
        return np.asarray(im).transpose(2, 0, 1)

    with ThreadPoolExecutor(threads) as pool:
        return np.stack(list(pool.map(one, range(len(table)))))


def named_draw(ra, n, Hh, Ww):
    """DeviceRandAugment.draw's table together with the operation names and signed magnitudes behind it (the same draws,
    made on a copy of the generator)."""
    rng = np.random.default_rng()
    rng.bit_generator.state = ra.rng.bit_generator.state
    which = rng.integers(0, len(ra.ops), (n, ra.num_ops))
    negate = rng.random((n, ra.num_ops)) < 0.5
    table = ra.draw(n, Hh, Ww)
    names = [[ra.ops[j] for j in row] for row in which]
    values = []
    for b in range(n):
        row = []
        for k, name in enumerate(names[b]):
            m = ra.magnitudes(name, Hh, Ww)
            v = 0.0 if m is None else float(m[ra.magnitude])
            row.append(-v if name in ra.SIGNED and negate[b, k] else v)
        values.append(row)
    return table, names, values


def measure(args):
    dev = torch.device("cuda", 0)
    be = calm.backend.get_backend()
    src = np.random.default_rng(0).integers(0, 256, (B, HS, HS, 3), dtype=np.uint8)          # HWC, as a decoder gives it
    # smooth the noise a little so that the histograms are not flat (Equalize and AutoContrast then move the image)
    src = (src.astype(np.float32) * np.linspace(0.3, 0.9, HS, dtype=np.float32)[None, None, :, None] + 20).astype(np.uint8)
    img = torch.from_numpy(np.ascontiguousarray(src.transpose(0, 3, 1, 2))).to(dev)
    col = trainer.DeviceCollate(seed=2006)
    flips = col.draw(B, H, H)[3].numpy()
    corners = col.draw_corners(B, HS, HS, H, H)
    out = torch.empty(B, 3, H, H, dtype=torch.uint8, device=dev)
    scratch = torch.empty(be.randaugment_scratch_bytes(B, H, H), dtype=torch.uint8, device=dev)

    variants = {"stage": DRA(seed=2006), "stage_geometric": DRA(ops=GEOMETRIC, seed=2006),
                "stage_statistics": DRA(ops=STATISTICS, seed=2006), "crop_flip": DRA(num_ops=0, seed=2006)}
    fns, plans, named = {}, {}, {}
    for name, ra in variants.items():
        table, names, values = named_draw(ra, B, H, H)
        table["y0"], table["x0"], table["flip"] = corners[:, 0], corners[:, 1], flips
        DRA.check(table, H, H)
        plan = DRA.launch_plan(table)
        packed = DRA.pack(table, device=dev)
        fns[name] = (lambda packed=packed, plan=plan, ra=ra: be.randaugment_u8(img, packed, out, *plan, fill=ra.fill, scratch=scratch))
        plans[name], named[name] = plan, (table, names, values, ra.fill)
    r = windows(fns, args.iters, args.repeats, 10)

    table, names, values, fill = named["stage"]
    fns["stage"]()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref = pil_chain(src, table, names, values, fill, args.threads)
        walls.append(time.perf_counter() - t0)
    same = bool(got.tobytes() == ref.tobytes())
    emit(what="RandAugment stage, 256 x 3 x 256 x 256 uint8 -> 256 x 3 x 224 x 224 uint8, two operations, magnitude 9 of 31",
         iters=args.iters, repeats=args.repeats,
         median_min_max_ms={k: [round(x / 1e3, 4) for x in v] for k, v in r.items()},
         n_slots_stats_mask={k: list(v) for k, v in plans.items()},
         images_per_s={k: round(B / (v[0] * 1e-6)) for k, v in r.items()},
         pil_host_ms=round(1e3 * min(walls), 1), pil_host_threads=args.threads, pil_host_images_per_s=round(B / min(walls)),
         pil_over_stage=round(1e3 * min(walls) / (r["stage"][0] / 1e3), 1), stage_equals_pil_bytes=same)
    assert same


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the run stops itself")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the PIL chain")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("randaug_time: no GPU — nothing measured")

    def expired(*_):
        print(f"randaug_time: stopped after {args.limit} s", flush=True)
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
