#!/usr/bin/env python3
"""What does stochastic depth cost on the MI355X?

1. Kernel level, at the 48 residual joins of the Small-224 model (their [B, L] shapes are recorded from one training
   forward at the workload's batch): calm_drop_path in its forward form (x, residual -> y: three streams of fp32) and in its
   backward form (dy -> dx: two streams), each as ONE pass over all 48 sites, next to calm_dropout in the same two forms on
   the same tensors — same bytes, one Philox call per four elements instead of one per (sample, chunk).  Achieved bytes / s
   = streams x 4 bytes x elements / device time.
2. Step level: one Small-224 training step (TrainStep over FusedClipAdamW, the workload's batch, fp32 as `python bench.py`)
   with set_drop_path(model, 0.1, "linear") against the same step with it off.

Device time is between two events around `--iters` calls (part 1) or `--steps` steps (part 2), after a warm-up, as the
median of `--repeats` windows with min .. max beside it; the variants alternate inside every repeat, in one process.  One
JSON line per figure, each with the sha256 of the kernel sources it was measured with; --out also writes them to a file
(default profiles/drop_path_timing.jsonl).  The run stops itself after --limit seconds.  Needs a GPU."""
import argparse
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"),
          os.path.join(ROOT, "tests", "tools")):
    sys.path.insert(0, p)
from importlib import import_module  # noqa: E402

import torch  # noqa: E402

import bench  # noqa: E402
import calm_vit_dte_amd as calm  # noqa: E402
from optim_groups_time import LINES, emit, windows  # noqa: E402
from sam_timing import source_stamp  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
vt = calm.Vi_Tools_CNN_less_V2


def site_shapes(batch, dev):
    """[(B, L)] of the drop-path calls of one Small-224 training forward, in call order."""
    wl = bench.WORKLOADS["small224"]
    x, _ = bench.synthetic_batch(batch, wl["kw"]["seq_length"], wl["kw"]["out_features"], seed=0, device=dev)
    m = bench.build_model(calm, wl["kw"], dev).train()
    vt.set_drop_path(m, 0.1, "uniform")
    be = calm.backend.get_backend()
    shapes, real = [], be.drop_path

    def recording(x, residual, y, B, L, p, key, sample0=0):
        shapes.append((int(B), int(L)))
        return real(x, residual, y, B, L, p, key, sample0)
    be.drop_path = recording
    try:
        with torch.no_grad():
            m(x)
    finally:
        del be.drop_path
    del m, x
    torch.cuda.empty_cache()
    return shapes


def kernels(args, stamp):
    dev = torch.device("cuda", 0)
    be = calm.backend.get_backend()
    batch = args.batch or bench.WORKLOADS["small224"]["batch"]
    shapes = site_shapes(batch, dev)
    distinct = sorted(set(shapes))
    key = calm.ops.draw_dropout_key(dev)
    # one (x, residual, y) triple per distinct shape; the pass over the 48 sites walks them in call order
    bufs = {s: tuple(torch.randn(s, device=dev) for _ in range(3)) for s in distinct}
    p = 0.1

    def path(residual):
        for s in shapes:
            x, r, y = bufs[s]
            be.drop_path(x, r if residual else None, y, s[0], s[1], p, key)

    def drop(residual):
        for s in shapes:
            x, r, y = bufs[s]
            be.dropout(x, r if residual else None, y, s[0] * s[1], p, key)
    fns = {"drop_path_fwd": lambda: path(True), "dropout_fwd": lambda: drop(True),
           "drop_path_bwd": lambda: path(False), "dropout_bwd": lambda: drop(False)}
    w = windows(fns, args.iters, args.repeats, 3)
    elements = sum(b * l for b, l in shapes)
    moved = {k: 4 * elements * (3 if k.endswith("fwd") else 2) for k in fns}
    emit(what="calm_drop_path next to calm_dropout, one pass over the residual joins of Small-224, fp32", source_sha256=stamp,
         batch=batch, sites=len(shapes), distinct_shapes=[list(s) for s in distinct], elements=elements, iters=args.iters,
         repeats=args.repeats, median_min_max_us={k: [round(x, 1) for x in v] for k, v in w.items()}, moved_bytes=moved,
         moved_gb_per_s={k: round(moved[k] / (w[k][0] * 1e-6) / 1e9, 1) for k in fns},
         drop_path_over_dropout={"fwd": round(w["drop_path_fwd"][0] / w["dropout_fwd"][0], 3),
                                 "bwd": round(w["drop_path_bwd"][0] / w["dropout_bwd"][0], 3)},
         fwd_plus_bwd_ms=round((w["drop_path_fwd"][0] + w["drop_path_bwd"][0]) / 1e3, 3))


def steps(args, stamp):
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS["small224"]
    batch = args.batch or wl["batch"]
    x, y = bench.synthetic_batch(batch, wl["kw"]["seq_length"], wl["kw"]["out_features"], seed=0, device=dev)
    runs = {}
    try:
        for kind in ("off", "drop_path"):
            torch.manual_seed(bench.NOISE_SEED)
            m = bench.build_model(calm, wl["kw"], dev).train()
            if kind == "drop_path":
                vt.set_drop_path(m, 0.1, "linear")
            opt = trainer.FusedClipAdamW(m)
            runs[kind] = (trainer.TrainStep(m, opt), opt)
        for step, _ in runs.values():
            for _ in range(args.warmup):
                step(x, y)
        torch.cuda.synchronize()
        ms = {k: [] for k in runs}
        for _ in range(args.repeats):
            for kind, (step, _) in runs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.steps):
                    step(x, y)
                t1.record()
                t1.synchronize()
                ms[kind].append(t0.elapsed_time(t1) / args.steps)
    finally:
        for _, opt in runs.values():
            opt.close()
    mmm = {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}
    emit(what="TrainStep with set_drop_path(0.1, linear) against the same step with it off, Small-224", source_sha256=stamp,
         batch=batch, steps=args.steps, warmup=args.warmup, repeats=args.repeats,
         median_min_max_ms={k: [round(x, 2) for x in v] for k, v in mmm.items()},
         added_ms=round(mmm["drop_path"][0] - mmm["off"][0], 2), drop_path_over_off=round(mmm["drop_path"][0] / mmm["off"][0], 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--limit", type=int, default=420, help="seconds after which the run stops itself")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=0, help="batch of both parts (default: the workload's)")
    ap.add_argument("--no-steps", action="store_true", help="the kernels only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drop_path_timing.jsonl"), help="the JSON lines' file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("drop_path_timing: no GPU — nothing measured")

    def expired(*_):
        print(f"drop_path_timing: stopped after {args.limit} s", flush=True)
        os._exit(3)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(args.limit)
    stamp = source_stamp()
    try:
        emit(what="box", device=torch.cuda.get_device_name(0), torch=torch.__version__)
        kernels(args, stamp)
        if not args.no_steps:
            steps(args, stamp)
    finally:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.writelines(json.dumps(r) + "\n" for r in LINES)


if __name__ == "__main__":
    main()
