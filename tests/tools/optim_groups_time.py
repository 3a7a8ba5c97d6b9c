#!/usr/bin/env python3
"""What do parameter groups cost the optimizer-side step on the MI355X?

On the parameter set of the Small-224 model (its tensors, shapes and deferred spectral-norm layers; random gradients),
calm_optim_step against calm_optim_step_groups with 1 group, 2 groups (the "no_decay" preset's assignment) and 16 groups
(tensor k in group k % 16).  calm_optim_step is timed twice, as two variants of its own: their difference and their
min .. max over the repeats are the spread every other difference is read against.

--parent-lib PATH: another build of libcalmvit_hip.so (the parent commit's, built from a checkout of it) is loaded beside
this tree's and its calm_optim_step is timed on the same plans' tensors, alternating with this tree's in the same windows
— the entry point's ABI is the same — as a record of its own.

Every figure is device time between two events around `--iters` calls, after a warm-up, as the median of `--repeats`
windows with min .. max beside it; the variants alternate inside every repeat, in one process.  One JSON line per
figure; --out also writes them to a file.  The run stops itself after --limit seconds.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
from importlib import import_module  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import calm_vit_dte_amd as calm  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
LINES = []


def emit(**rec):
    LINES.append(rec)
    print(json.dumps(rec), flush=True)


def windows(fns, iters, repeats, warmup):
    """Median / min / max microseconds of device time per call of each fn; the fns alternate inside every repeat."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                fn()
            t1.record()
            t1.synchronize()
            times[k].append(1e3 * t0.elapsed_time(t1) / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def against_parent(args, be, recs, grads, hp, stats):
    """calm_optim_step of the library at args.parent_lib against this tree's: raw calls of both, each on two plans."""
    binding = import_module("calm_vit_dte_amd._lib")
    backend = import_module("calm_vit_dte_amd.backend")
    other = ctypes.CDLL(os.path.abspath(args.parent_lib))
    other.calm_optim_step.restype, other.calm_optim_step.argtypes = binding.SIGNATURES["calm_optim_step"]
    ptrs = np.asarray([g.data_ptr() for g in grads], dtype=np.uint64)

    def call(lib, plan):
        plan.upload(ptrs)
        h = binding.OptimHparams(*hp)
        rc = lib.calm_optim_step(plan.table_dev.data_ptr(), plan.n, plan.chunk_dev.data_ptr(), plan.n_chunks,
                                 plan.scratch.data_ptr(), ctypes.byref(h), None, stats.data_ptr(), plan.step_dev.data_ptr(),
                                 None, backend._stream())
        assert rc == 0, rc

    plans = {k: be.optim_plan(recs) for k in ("this_tree", "parent", "this_tree_again", "parent_again")}
    fns = {k: (lambda k=k: call(other if k.startswith("parent") else be.lib, plans[k])) for k in plans}
    r = windows(fns, args.iters, args.repeats, 20)
    emit(what="calm_optim_step, the library of --parent-lib against this tree, Small-224 parameter set",
         iters=args.iters, repeats=args.repeats, median_min_max_us={k: [round(x, 2) for x in v] for k, v in r.items()})


def measure(args):
    dev = torch.device("cuda", 0)
    be = calm.backend.get_backend()
    m = bench.build_model(calm, bench.WORKLOADS["small224"]["kw"], dev).train()
    opt = trainer.FusedClipAdamW(m, lr=1e-6)            # (its records: the tensors, the moments, the deferred layers)
    try:
        recs = opt._records
        gen = torch.Generator(device=dev).manual_seed(0)
        grads = [torch.randn(r["param"].shape, device=dev, generator=gen) * 0.02 for r in recs]
        small = [int(r["param"].dim() <= 1) for r in recs]
        stats = torch.zeros(2, device=dev)
        hp = (1e-6, 0.9, 0.98, 1e-8, 0.02, 1.0, 0)
        assign = {"groups_1": [0] * len(recs), "groups_2_no_decay": small, "groups_16": [k % 16 for k in range(len(recs))]}
        plans = {k: be.optim_plan([dict(r, group=g) for r, g in zip(recs, a)], n_groups=max(a) + 1) for k, a in assign.items()}
        rates = {k: [(1e-6, 0.02 if g != 1 else 0.0) for g in range(max(a) + 1)] for k, a in assign.items()}
        plain = {k: be.optim_plan(recs) for k in ("step", "step_again")}
        fns = {k: (lambda p=p: be.optim_step(p, grads, hp, None, stats)) for k, p in plain.items()}
        fns.update({k: (lambda p=p, r=rates[k]: be.optim_step_groups(p, grads, hp, r, None, stats)) for k, p in plans.items()})
        r = windows(fns, args.iters, args.repeats, 20)
        assert float(stats[1]) == 0.0
        if args.parent_lib:
            against_parent(args, be, recs, grads, hp, stats)
    finally:
        opt.close()
    us = {k: [round(x, 2) for x in v] for k, v in r.items()}
    spread = max(abs(r["step"][0] - r["step_again"][0]), r["step"][2] - r["step"][1], r["step_again"][2] - r["step_again"][1])
    emit(what="optimizer-side step, Small-224 parameter set", tensors=len(recs), elements=sum(x["param"].numel() for x in recs),
         deferred=sum(x["sn"] is not None for x in recs), iters=args.iters, repeats=args.repeats, median_min_max_us=us,
         spread_us=round(spread, 2),
         grouped_minus_step_us={k: round(r[k][0] - r["step"][0], 2) for k in plans},
         within_spread={k: bool(abs(r[k][0] - r["step"][0]) <= spread) for k in plans})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the run stops itself")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--parent-lib", default=None, metavar="PATH",
                    help="another build of libcalmvit_hip.so whose calm_optim_step is timed against this tree's")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_groups_time: no GPU — nothing measured")

    def expired(*_):
        print(f"optim_groups_time: stopped after {args.limit} s", flush=True)
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
