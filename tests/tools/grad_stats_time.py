#!/usr/bin/env python3
"""What does the gradient monitor cost on the MI355X?

On the parameter set of the Small-224 model (its tensors, shapes and deferred spectral-norm layers; random gradients, the
step count at 1000 so that the Adam direction is evaluated): calm_grad_stats against calm_optim_step, and
FusedClipAdamW.step() with and without a GradMonitor attached.  calm_optim_step is timed twice, as two variants of its
own: their difference and their min .. max over the repeats are the spread every other difference is read against.  The
bar of the feature is relative: the median of calm_grad_stats at or below the median of calm_optim_step, beyond that
spread.  The bytes calm_grad_stats reads (G twice for the deferred tensors, G, p, m, v once for all) over its median give
the achieved bandwidth.

Every figure is device time between two events around `--iters` calls, after a warm-up, as the median of `--repeats`
windows with min .. max beside it; the variants alternate inside every repeat, in one process.  One JSON line per
figure; --out also writes them to a file (default profiles/grad_stats_time.jsonl).  The run stops itself after --limit
seconds.  Needs a GPU."""
import argparse
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests", "tools")):
    sys.path.insert(0, p)
from importlib import import_module  # noqa: E402

import torch  # noqa: E402

import bench  # noqa: E402
import calm_vit_dte_amd as calm  # noqa: E402
from optim_groups_time import LINES, emit, windows  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")


def measure(args):
    dev = torch.device("cuda", 0)
    be = calm.backend.get_backend()
    m = bench.build_model(calm, bench.WORKLOADS["small224"]["kw"], dev).train()
    opt = trainer.FusedClipAdamW(m, lr=1e-6)            # (its records: the tensors, the moments, the deferred layers)
    try:
        recs = opt._records
        gen = torch.Generator(device=dev).manual_seed(0)
        grads = [torch.randn(r["param"].shape, device=dev, generator=gen) * 0.02 for r in recs]
        stats = torch.zeros(2, device=dev)
        hp = (1e-6, 0.9, 0.98, 1e-8, 0.02, 1.0, 0)
        mon = trainer.GradMonitor(m, opt)
        plans = {k: be.optim_plan(recs) for k in ("grad_stats", "step", "step_again")}
        for p in list(plans.values()) + [opt._plan]:
            p.step_dev.fill_(1000)
        scratch = torch.empty(be.grad_stats_scratch_floats(plans["grad_stats"]), dtype=torch.float32, device=dev)

        def optimizer_step(monitor):
            opt.monitor = monitor
            for p, g in zip(opt.params, grads):
                p.grad = g
            opt.step()

        fns = {"grad_stats": lambda: be.grad_stats(plans["grad_stats"], grads, hp, None, mon._out, mon._summary, scratch),
               "step": lambda: be.optim_step(plans["step"], grads, hp, None, stats),
               "step_again": lambda: be.optim_step(plans["step_again"], grads, hp, None, stats),
               "optimizer_step": lambda: optimizer_step(None),
               "optimizer_step_monitored": lambda: optimizer_step(mon)}
        r = windows(fns, args.iters, args.repeats, 20)
        assert float(stats[1]) == 0.0
        rep = mon.read()
        assert rep["skipped"] == 0 and rep["norm"] > 0
    finally:
        opt.monitor = None
        opt.close()
    us = {k: [round(x, 2) for x in v] for k, v in r.items()}
    spread = max(abs(r["step"][0] - r["step_again"][0]), r["step"][2] - r["step"][1], r["step_again"][2] - r["step_again"][1])
    elements = sum(x["param"].numel() for x in recs)
    deferred = sum(x["param"].numel() for x in recs if x["sn"] is not None)
    read_bytes = 4 * (4 * elements + 2 * deferred)
    emit(what="gradient monitor, Small-224 parameter set", tensors=len(recs), elements=elements,
         deferred_tensors=sum(x["sn"] is not None for x in recs), deferred_elements=deferred, iters=args.iters,
         repeats=args.repeats, median_min_max_us=us, spread_us=round(spread, 2),
         grad_stats_minus_step_us=round(r["grad_stats"][0] - r["step"][0], 2),
         grad_stats_at_or_below_step=bool(r["grad_stats"][0] <= r["step"][0] + spread),
         grad_stats_read_bytes=read_bytes, grad_stats_gb_per_s=round(read_bytes / (r["grad_stats"][0] * 1e-6) / 1e9, 1),
         monitored_minus_plain_optimizer_step_us=round(r["optimizer_step_monitored"][0] - r["optimizer_step"][0], 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--limit", type=int, default=240, help="seconds after which the run stops itself")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_stats_time.jsonl"), help="the JSON lines' file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("grad_stats_time: no GPU — nothing measured")

    def expired(*_):
        print(f"grad_stats_time: stopped after {args.limit} s", flush=True)
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
