#!/usr/bin/env python3
"""What do the two SAM kernels, and a SAM step, cost on the MI355X?

1. On the parameter set of the Small-224 model (its tensors, shapes and deferred spectral-norm layers; random gradients):
   calm_sam_perturb + calm_sam_restore as a pair (a run of perturbations without the way back would walk the weights off),
   calm_sam_restore alone, and calm_optim_step twice, as two variants of its own — their difference and their min .. max
   over the repeats are the spread every other difference is read against.  perturb = pair - restore.
   The byte model (model_bytes): the perturbation reads G and W and writes the backup and W (16 bytes per element) and
   reads G and W once more for c on the deferred tensors (8 bytes more); the restore reads the backup and writes W (8
   bytes).  What the launches request (moved_bytes) is more: the norm pass reads G (adaptive: and W) a further time, so
   the perturbation asks for 20 (24) bytes per element and 8 more on the deferred tensors; calm_optim_step for 32 (G in
   its first pass; G, p, m, v read and p, m, v written in its third) and 4 more on the deferred tensors.
2. At the bench shape (Small-224, the workload's batch, fp32): SamTrainStep against TrainStep, wall time per step between
   synchronisations.  A SAM step is expected to cost about two plain steps.

Device time of part 1 is between two events around `--iters` calls, after a warm-up, as the median of `--repeats` windows
with min .. max beside it; the variants alternate inside every repeat, in one process.  One JSON line per figure, each with
the sha256 of the kernel sources it was measured with; --out also writes them to a file (default
profiles/sam_timing.jsonl).  The run stops itself after --limit seconds.  Needs a GPU."""
import argparse
import glob
import hashlib
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests", "tools")):
    sys.path.insert(0, p)
from importlib import import_module  # noqa: E402

import torch  # noqa: E402

import bench  # noqa: E402
import calm_vit_dte_amd as calm  # noqa: E402
from optim_groups_time import LINES, emit, windows  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")


def source_stamp():
    """sha256 over the kernel sources (name and content, in name order), as scripts/pmc_summary.py stamps its summaries"""
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "calm-vit-dte_amd", "csrc", "*"))):
        if os.path.isfile(f):
            h.update(os.path.basename(f).encode())
            h.update(hashlib.sha256(open(f, "rb").read()).digest())
    return h.hexdigest()


def kernels(args, stamp):
    dev = torch.device("cuda", 0)
    be = calm.backend.get_backend()
    m = bench.build_model(calm, bench.WORKLOADS["small224"]["kw"], dev).train()
    opt = trainer.FusedClipAdamW(m, lr=1e-6)            # (its records: the tensors, the moments, the deferred layers)
    try:
        recs = opt._records
        gen = torch.Generator(device=dev).manual_seed(0)
        grads = [torch.randn(r["param"].shape, device=dev, generator=gen) * 0.02 for r in recs]
        stats, sam_stats = torch.zeros(2, device=dev), torch.zeros(3, device=dev)
        hp = (1e-6, 0.9, 0.98, 1e-8, 0.02, 1.0, 0)
        plans = {k: be.optim_plan(recs) for k in ("sam", "step", "step_again")}
        for p in plans.values():
            p.step_dev.fill_(1000)
        backups = [torch.empty_like(r["param"]) for r in recs]
        ptrs = torch.tensor([b.data_ptr() for b in backups], dtype=torch.int64, device=dev)
        scratch = torch.empty(be.sam_scratch_floats(plans["sam"]), dtype=torch.float32, device=dev)
        r = {}
        for adaptive in (0, 1):
            sam_hp = (0.05, 1e-12, 0.01, adaptive)

            def pair():
                be.sam_perturb(plans["sam"], grads, sam_hp, None, ptrs, scratch, sam_stats)
                be.sam_restore(plans["sam"], ptrs)

            pair()                                          # (the backups hold the weights before `restore` is timed alone)
            fns = {"perturb_restore": pair, "restore": lambda: be.sam_restore(plans["sam"], ptrs),
                   "step": lambda: be.optim_step(plans["step"], grads, hp, None, stats),
                   "step_again": lambda: be.optim_step(plans["step_again"], grads, hp, None, stats)}
            r[adaptive] = windows(fns, args.iters, args.repeats, 20)
            assert float(stats[1]) == 0.0 and float(sam_stats[1]) == 0.0 and float(sam_stats[2]) > 0.0
    finally:
        opt.close()
    elements = sum(x["param"].numel() for x in recs)
    deferred = sum(x["param"].numel() for x in recs if x["sn"] is not None)
    for adaptive, w in r.items():
        spread = max(abs(w["step"][0] - w["step_again"][0]), w["step"][2] - w["step"][1], w["step_again"][2] - w["step_again"][1])
        perturb = w["perturb_restore"][0] - w["restore"][0]
        model = {"perturb": 4 * (4 * elements + 2 * deferred), "restore": 4 * 2 * elements}
        moved = {"perturb": 4 * ((6 if adaptive else 5) * elements + 2 * deferred), "restore": 4 * 2 * elements,
                 "step": 4 * (8 * elements + deferred)}
        emit(what="SAM kernels, Small-224 parameter set", source_sha256=stamp, adaptive=bool(adaptive), tensors=len(recs),
             elements=elements, deferred_tensors=sum(x["sn"] is not None for x in recs), deferred_elements=deferred,
             iters=args.iters, repeats=args.repeats, median_min_max_us={k: [round(x, 2) for x in v] for k, v in w.items()},
             spread_us=round(spread, 2), perturb_us=round(perturb, 2), restore_us=round(w["restore"][0], 2),
             step_us=round(w["step"][0], 2), model_bytes=model, moved_bytes=moved,
             moved_gb_per_s={"perturb": round(moved["perturb"] / (perturb * 1e-6) / 1e9, 1),
                             "restore": round(moved["restore"] / (w["restore"][0] * 1e-6) / 1e9, 1),
                             "step": round(moved["step"] / (w["step"][0] * 1e-6) / 1e9, 1)},
             perturb_at_or_below_step=bool(perturb <= w["step"][0] + spread),
             restore_at_or_below_step=bool(w["restore"][0] <= w["step"][0] + spread))


def steps(args, stamp):
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS["small224"]
    batch = args.batch or wl["batch"]
    x, y = bench.synthetic_batch(batch, wl["kw"]["seq_length"], wl["kw"]["out_features"], seed=0, device=dev)
    ms = {}
    for kind in ("plain", "sam"):
        torch.manual_seed(bench.NOISE_SEED)
        m = bench.build_model(calm, wl["kw"], dev).train()
        opt = trainer.FusedClipAdamWindow(m) if kind == "sam" else trainer.FusedClipAdamW(m)
        try:
            step = trainer.SamTrainStep(m, opt, sam=trainer.SharpnessAware(m, opt)) if kind == "sam" else trainer.TrainStep(m, opt)
            for _ in range(args.warmup):
                step(x, y)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(x, y)
            torch.cuda.synchronize()
            ms[kind] = 1e3 * (time.perf_counter() - t0) / args.steps
        finally:
            opt.close()
        del step, opt, m
        torch.cuda.empty_cache()
    emit(what="SamTrainStep against TrainStep, Small-224, fp32", source_sha256=stamp, batch=batch, steps=args.steps,
         warmup=args.warmup, ms_per_step={k: round(v, 2) for k, v in ms.items()}, sam_over_plain=round(ms["sam"] / ms["plain"], 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--limit", type=int, default=420, help="seconds after which the run stops itself")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=0, help="batch of the step comparison (default: the workload's)")
    ap.add_argument("--no-steps", action="store_true", help="the kernels only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_timing.jsonl"), help="the JSON lines' file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sam_timing: no GPU — nothing measured")

    def expired(*_):
        print(f"sam_timing: stopped after {args.limit} s", flush=True)
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
