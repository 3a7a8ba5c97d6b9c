#!/usr/bin/env python3
"""What does knowledge distillation cost on the MI355X?

  (a) the loss alone, forward + backward through autograd, at [256, 1000] and [484, 1000]: the fused kernel pair
      (calm_distill_fwd / _bwd, loss kernels on) against the stock-torch chain (trainer.distill_loss_torch, kernels off);
  (b) a Small-224 student step with a Base-224 teacher (batch 256, autocast bf16 + GradScaler, FusedClipAdamW), teacher
      eager and captured (teacher_graph=True), against the SUM of a student-only TrainStep and a stand-alone lean teacher
      forward (Predictor), all four in one process and alternating.

Every figure is wall time around work that ends in a device synchronise, after a warm-up of every shape, as the median of
`--repeats` windows with the spread (min .. max) beside it.  One JSON line per figure; --out also writes them to a file.
The whole run stops itself after --limit seconds.  Needs a GPU: there is nothing to time without one."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
from importlib import import_module  # noqa: E402

import torch  # noqa: E402

import bench  # noqa: E402
import calm_vit_dte_amd as calm  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
LINES = []


def emit(**rec):
    LINES.append(rec)
    print(json.dumps(rec), flush=True)


def windows(fns, iters, repeats, warmup):
    """Median / min / max microseconds per call of each fn: warm-up first, then `repeats` rounds that alternate the fns."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            times[k].append(1e6 * (time.perf_counter() - t0) / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def loss_alone(args):
    import distill_f64 as D
    for B, C in ((256, 1000), (484, 1000)):
        z, t, y = (v.cuda() for v in D.inputs(B, C, 2.0))
        z.requires_grad_(True)
        for mode in ("soft", "hard"):
            def run(on, mode=mode):
                calm.backend.set_loss_kernels(on)
                z.grad = None
                trainer.distillation_loss(z, t, y, 0.5, 2.0, mode).backward()
            # the same numbers before the same time (float64 is the tests' business: here the two paths against each other)
            run(False)
            g_off = z.grad.clone()
            run(True)
            diff = float((z.grad - g_off).abs().max() / g_off.abs().max())
            r = windows({"kernels": lambda: run(True), "torch": lambda: run(False)}, args.loss_iters, args.repeats, 20)
            emit(what="loss fwd+bwd", B=B, C=C, mode=mode, kernels_us=round(r["kernels"][0], 1),
                 kernels_spread_us=[round(v, 1) for v in r["kernels"][1:]], torch_us=round(r["torch"][0], 1),
                 torch_spread_us=[round(v, 1) for v in r["torch"][1:]], grad_rel_diff=diff)
    calm.backend.set_loss_kernels(False)


def step_with_teacher(args):
    dev = torch.device("cuda", 0)
    ws, wt = bench.WORKLOADS["small224"], bench.WORKLOADS["base224"]
    bs = args.batch
    x, y = bench.synthetic_batch(bs, 224, 1000, 0, dev)
    teacher = bench.build_model(calm, wt["kw"], dev).eval()
    with torch.no_grad():
        for p in teacher.parameters():
            p.mul_(1.01)
    calm.backend.set_loss_kernels(True)
    amp = dict(autocast_dtype=torch.bfloat16)
    made = {}

    def student(kind):
        m = bench.build_model(calm, ws["kw"], dev).train()
        opt = trainer.FusedClipAdamW(m)
        kw = dict(scaler=torch.amp.GradScaler("cuda"), **amp)
        if kind == "plain":
            step = trainer.TrainStep(m, opt, None, **kw)
        else:
            step = trainer.DistillTrainStep(m, opt, teacher, alpha=0.5, temperature=2.0, teacher_graph=kind == "graph", **kw)
        made[kind] = (m, opt, step)
        return step

    steps = {k: student(k) for k in ("plain", "eager", "graph")}
    lean = trainer.Predictor(teacher, **amp)
    fns = {"student_only_step": lambda: steps["plain"](x, y), "teacher_forward_lean": lambda: lean(x),
           "distill_step_eager_teacher": lambda: steps["eager"](x, y), "distill_step_graphed_teacher": lambda: steps["graph"](x, y)}
    try:
        r = windows(fns, args.step_iters, args.repeats, 3)
    finally:
        for _, opt, step in made.values():
            if isinstance(getattr(step, "teacher", None), trainer.Predictor):
                step.teacher.close()
            opt.close()
    ms = {k: [round(v / 1e3, 2) for v in r[k]] for k in r}
    emit(what="step", student="small224", teacher="base224", batch=bs, precision="autocast bf16 + GradScaler",
         median_min_max_ms=ms, sum_student_plus_teacher_ms=round(ms["student_only_step"][0] + ms["teacher_forward_lean"][0], 2),
         peak_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))
    calm.backend.set_loss_kernels(False)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--limit", type=int, default=540, help="seconds after which the run stops itself")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loss-iters", type=int, default=200)
    ap.add_argument("--step-iters", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--skip-step", action="store_true", help="part (a) only")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("distill_step_time: no GPU — nothing measured")

    def expired(*_):
        print(f"distill_step_time: stopped after {args.limit} s", flush=True)
        os._exit(3)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(args.limit)
    try:
        emit(what="box", device=torch.cuda.get_device_name(0), torch=torch.__version__)
        loss_alone(args)
        if not args.skip_step:
            step_with_teacher(args)
    finally:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.writelines(json.dumps(r) + "\n" for r in LINES)


if __name__ == "__main__":
    main()
