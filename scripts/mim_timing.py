#!/usr/bin/env python3
"""What does masked image modelling cost on the MI355X?

1. Kernel level, at the row tokens of the Small-224 batch (B = 256, S = 224: n = 3 B S^2 fp32 elements per tensor), for the
   patch sides 16 and 32 at ratio 0.6: calm_mim_draw, calm_mim_apply (out of place and in place), calm_mim_huber_fwd and
   calm_mim_huber_bwd, next to calm_recon_huber_rows_fwd / _bwd — the unmasked loss of the same job — on the same n.  The
   unmasked pair is timed twice, as two variants of its own: min .. max of its windows is the spread every masked figure is
   read against.
2. Step level: one Small-224 `generate=True` RegTrainStep over FusedClipAdamW (fp32, loss kernels on, image batch) with
   mim={"patch": 32, "ratio": 0.6} against the same step without it.

Device time is between two events around `--iters` calls (part 1) or `--steps` steps (part 2), after a warm-up, as the
median of `--repeats` windows with min .. max beside it; the variants alternate inside every repeat, in one process.  One
JSON line per figure, each with the sha256 of the kernel sources it was measured with; --out also writes them to a file
(default profiles/mim_timing.jsonl).  The run stops itself after --limit seconds.  Needs a GPU."""
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
RATIO = 0.6


def kernels(args, stamp):
    dev = torch.device("cuda", 0)
    be = calm.backend.get_backend()
    B, S = args.batch or bench.WORKLOADS["small224"]["batch"], bench.WORKLOADS["small224"]["kw"]["seq_length"]
    n = 3 * B * S * S
    gen = torch.Generator(device=dev).manual_seed(0)
    tokens, target = (torch.randn(B, S, 3 * S, device=dev, generator=gen) for _ in range(2))
    out, work = torch.empty_like(tokens), tokens.clone()
    loss, dloss = torch.empty((), device=dev), torch.ones(1, device=dev)
    key = calm.ops.draw_dropout_key(dev)

    def unmasked_fwd():
        be.huber_rows_fwd(tokens, target, 1.0, loss, n)

    def unmasked_bwd():
        be.huber_rows_bwd(tokens, target, 1.0, dloss, out, n)
    for p in (16, 32):
        mim = trainer.MaskedImageModelling(p, RATIO)
        G, P, k = mim.grid(S)
        mask = torch.empty(B, P, dtype=torch.uint8, device=dev)
        be.mim_draw(mask, B, G, k, key)
        assert int(mask.sum()) == B * k
        fns = {"huber_rows_fwd": unmasked_fwd, "huber_rows_bwd": unmasked_bwd,
               "mim_draw": lambda: be.mim_draw(mask, B, G, k, key),
               "mim_apply": lambda: be.mim_apply(tokens, out, mask, mim.fill, B, S, p),
               "mim_apply_in_place": lambda: be.mim_apply(work, work, mask, mim.fill, B, S, p),
               "mim_huber_fwd": lambda: be.mim_huber_fwd(tokens, target, mask, 1.0, loss, B, S, p, B * k),
               "mim_huber_bwd": lambda: be.mim_huber_bwd(tokens, target, mask, 1.0, dloss, out, B, S, p, B * k),
               "huber_rows_fwd_again": unmasked_fwd, "huber_rows_bwd_again": unmasked_bwd}
        w = windows(fns, args.iters, args.repeats, 3)
        share = k / P
        # bytes the algorithm needs: the unmasked pair reads two tensors (and writes one); the masked pair reads the
        # masked share of two (and writes one in full); apply reads the unmasked share and writes everything — in place
        # it writes the masked share only
        moved = {"huber_rows_fwd": 8 * n, "huber_rows_bwd": 12 * n, "mim_apply": int(4 * n * (2 - share)),
                 "mim_apply_in_place": int(4 * n * share), "mim_huber_fwd": int(8 * n * share),
                 "mim_huber_bwd": int(4 * n * (1 + 2 * share))}
        spread = {d: [min(w[f"huber_rows_{d}"][1], w[f"huber_rows_{d}_again"][1]),
                      max(w[f"huber_rows_{d}"][2], w[f"huber_rows_{d}_again"][2])] for d in ("fwd", "bwd")}
        emit(what="the calm_mim entry points next to calm_recon_huber_rows on the row tokens of the Small-224 batch, fp32",
             source_sha256=stamp, batch=B, S=S, patch=p, ratio=RATIO, k=k, P=P, elements=n, iters=args.iters,
             repeats=args.repeats, median_min_max_us={name: [round(x, 1) for x in v] for name, v in w.items()},
             moved_bytes=moved, moved_gb_per_s={name: round(moved[name] / (w[name][0] * 1e-6) / 1e9, 1) for name in moved},
             unmasked_min_max_us={d: [round(x, 1) for x in v] for d, v in spread.items()},
             masked_over_unmasked={d: round(w[f"mim_huber_{d}"][0] / w[f"huber_rows_{d}"][0], 3) for d in ("fwd", "bwd")},
             masked_median_within_unmasked_max={d: bool(w[f"mim_huber_{d}"][0] <= spread[d][1]) for d in ("fwd", "bwd")})


def gen_model(dev):
    kw = bench.WORKLOADS["small224"]["kw"]
    m = calm.ViT(torch.device("cpu"), type=8, force_reduce=False, generate=True, **kw)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in calm.synthetic_weights.make_params(shapes, bench.WEIGHT_SEED).items()})
    return m.to(dev).train()


def steps(args, stamp):
    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS["small224"]
    batch = args.batch or wl["batch"]
    x, _ = bench.synthetic_batch(batch, wl["kw"]["seq_length"], wl["kw"]["out_features"], seed=0, device=dev)
    runs = {}
    was = calm.backend.get_loss_kernels()
    calm.backend.set_loss_kernels(True)
    try:
        for kind in ("off", "mim"):
            torch.manual_seed(bench.NOISE_SEED)
            m = gen_model(dev)
            opt = trainer.FusedClipAdamW(m)
            runs[kind] = (trainer.RegTrainStep(m, opt, mim={"patch": 32, "ratio": RATIO} if kind == "mim" else None), opt)
        for step, _ in runs.values():
            for _ in range(args.warmup):
                step(x)
        torch.cuda.synchronize()
        ms = {k: [] for k in runs}
        for _ in range(args.repeats):
            for kind, (step, _) in runs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.steps):
                    step(x)
                t1.record()
                t1.synchronize()
                ms[kind].append(t0.elapsed_time(t1) / args.steps)
    finally:
        calm.backend.set_loss_kernels(was)
        for _, opt in runs.values():
            opt.close()
    mmm = {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}
    emit(what="RegTrainStep(mim={patch 32, ratio 0.6}) against the same step without mim, Small-224 generate=True, image batch",
         source_sha256=stamp, batch=batch, steps=args.steps, warmup=args.warmup, repeats=args.repeats,
         median_min_max_ms={k: [round(x, 2) for x in v] for k, v in mmm.items()},
         added_ms=round(mmm["mim"][0] - mmm["off"][0], 2), mim_over_off=round(mmm["mim"][0] / mmm["off"][0], 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--limit", type=int, default=420, help="seconds after which the run stops itself")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=0, help="batch of both parts (default: the workload's)")
    ap.add_argument("--no-steps", action="store_true", help="the kernels only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mim_timing.jsonl"), help="the JSON lines' file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mim_timing: no GPU — nothing measured")

    def expired(*_):
        print(f"mim_timing: stopped after {args.limit} s", flush=True)
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
