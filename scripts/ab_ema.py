#!/usr/bin/env python3
"""Time calm_ema_update next to the update pass of calm_optim_step (the yardstick: the existing multi-tensor pass over the
same parameters) on the Base-224 parameter set, and a Base-224 autocast(bfloat16) training step with and without `ema=`,
eager and captured.

Kernel figures — achieved bytes/s over the algorithmic bytes, HIP events around `--iters` calls after `--warmup`:
  calm_ema_update   parameter read, average read and written: 12 bytes per element (both of its launches are inside)
  optim_update      gradient read, parameter and both moments read and written: 28 bytes per element.  The pass is one of
                    calm_optim_step's three launches and cannot be bracketed by events on its own; its time is the call on
                    finite gradients minus the same call with one infinite gradient, in which the pass returns at once
                    while the statistics and finalize launches do the same work.  Plain tensors (defer_sn=False): the
                    pass without the spectral-norm correction, its fastest form.
Acceptance: the EMA's median rate is not below optim_update's by more than the run's own spread (the larger max - min of
the two over the rounds).
Step figures — TrainStep and GraphedTrainStep with FusedClipAdamW under autocast(bfloat16) + GradScaler at `--batch`.
Every set of candidates is measured in `--rounds` alternating rounds in one process; the table holds the median and the
spread (min .. max) over the rounds.  --out FILE writes it as JSON (profiles/ema_ab.json)."""
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
from calm_vit_dte_amd import _lib, trainer  # noqa: E402

HBM_PEAK = 8e12
BASE224 = dict(heads=12, seq_length=224, in_features=672, dim_step=48, mean_var_hidden=240, seq_len_step=16,
               seq_len_reduce=80, out_features=1000)
WEIGHT_SEED = 1234


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
    """{name: [us per iteration, one figure per round]}, the candidates taking turns within every round."""
    out = {k: [] for k in fns}
    for r in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, iters, warmup if r == 0 else 1))
    return out


def summary(us, nbytes=None):
    s = {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "rounds_us": list(us)}
    if nbytes is not None:
        rates = [nbytes / (u * 1e-6) for u in us]
        s.update(algorithmic_bytes=nbytes, median_bytes_per_s=statistics.median(rates), min_bytes_per_s=min(rates),
                 max_bytes_per_s=max(rates))
    return s


def build_cpu_model():
    m = calm.ViT(torch.device("cpu"), type=8, force_reduce=False, generate=False, **BASE224)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in calm.synthetic_weights.make_params(shapes, WEIGHT_SEED).items()})
    return m


def kernels(model, args):
    be = calm.backend.get_backend()
    opt = trainer.FusedClipAdamW(model, defer_sn=False)
    ema = trainer.ModelEMA(model, decay=0.9999, warmup=True)
    n = sum(p.numel() for p in opt.params)
    gen = torch.Generator(device="cuda").manual_seed(0)
    grads = [torch.randn(p.shape, device="cuda", generator=gen) * 1e-3 for p in opt.params]
    grads_inf = list(grads)
    grads_inf[0] = grads[0].clone()
    grads_inf[0].view(-1)[0] = float("inf")
    hp = (1e-4, 0.9, 0.98, 1e-8, 0.02, 1.0, 0)
    t = alternate({"ema": lambda: be.ema_update(ema._plan, ema.decay, ema.schedule),
                   "optim_step": lambda: be.optim_step(opt._plan, grads, hp, None, opt.stats),
                   "optim_step_skipped": lambda: be.optim_step(opt._plan, grads_inf, hp, None, opt.stats)},
                  args.rounds, args.iters, args.warmup)
    opt.close()
    upd = [a - b for a, b in zip(t["optim_step"], t["optim_step_skipped"])]
    row = {"parameters": n, "tensors": len(opt.params), "calm_ema_update": summary(t["ema"], 12 * n),
           "optim_update": summary(upd, 28 * n), "calm_optim_step": summary(t["optim_step"]),
           "calm_optim_step_skipped": summary(t["optim_step_skipped"])}
    e, o = row["calm_ema_update"], row["optim_update"]
    spread = max(e["max_bytes_per_s"] - e["min_bytes_per_s"], o["max_bytes_per_s"] - o["min_bytes_per_s"])
    row["spread_bytes_per_s"] = spread
    row["accepted"] = bool(e["median_bytes_per_s"] >= o["median_bytes_per_s"] - spread)
    print(f"{n} parameters in {len(opt.params)} tensors")
    for label, s in (("calm_ema_update", e), ("optim_update", o)):
        print(f"{label:16s} {s['median_us']:7.1f} us ({s['min_us']:.1f} .. {s['max_us']:.1f})  {s['median_bytes_per_s'] / 1e12:5.2f} TB/s "
              f"({s['min_bytes_per_s'] / 1e12:.2f} .. {s['max_bytes_per_s'] / 1e12:.2f})")
    print(f"spread {spread / 1e12:.2f} TB/s, accepted: {row['accepted']}")
    return row


def steps(cpu_model, args):
    import copy
    g = np.random.default_rng(0)
    x = torch.from_numpy(g.standard_normal((args.batch, 3, 224, 224)).astype(np.float32)).cuda()
    y = torch.zeros(args.batch, 1000, device="cuda")
    y[torch.arange(args.batch), torch.from_numpy(g.integers(0, 1000, args.batch)).cuda()] = 1.0
    fns, keep = {}, []
    for graphed in (False, True):
        for with_ema in (False, True):
            m = copy.deepcopy(cpu_model).cuda().train()
            opt = trainer.FusedClipAdamW(m)
            ema = trainer.ModelEMA(m) if with_ema else None
            scaler = torch.amp.GradScaler("cuda")
            if graphed:
                step = trainer.GraphedTrainStep(m, opt, x, y, scaler=scaler, autocast_dtype=torch.bfloat16, ema=ema)
            else:
                step = trainer.TrainStep(m, opt, scaler=scaler, autocast_dtype=torch.bfloat16, ema=ema)
            keep.append((m, opt, ema, step))
            fns[("graphed" if graphed else "eager") + ("_ema" if with_ema else "")] = (lambda s=step: s(x, y))
    rows = {}
    for mode in ("eager", "graphed"):
        t = alternate({k: fns[k] for k in (mode, mode + "_ema")}, args.rounds, args.step_iters, 3)
        rows[mode] = {"without_ema": summary(t[mode]), "with_ema": summary(t[mode + "_ema"])}
        a, b = rows[mode]["without_ema"], rows[mode]["with_ema"]
        print(f"base224 autocast {mode:8s}: {a['median_us'] / 1e3:7.2f} ms/step ({a['min_us'] / 1e3:.2f} .. {a['max_us'] / 1e3:.2f})   "
              f"with ema= {b['median_us'] / 1e3:7.2f} ms/step ({b['min_us'] / 1e3:.2f} .. {b['max_us'] / 1e3:.2f})")
    for _, opt, _, _ in keep:
        opt.close()
    return {"batch": args.batch, **rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-iters", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-steps", action="store_true", help="kernel figures only")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_ema.py times kernels: it needs the GPU")
    assert _lib.load().calm_ema_chunk_elems() > 0
    cpu_model = build_cpu_model()
    import copy
    result = {"iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "step_iters": args.step_iters,
              "hbm_peak_bytes_per_s": HBM_PEAK, "kernels": kernels(copy.deepcopy(cpu_model).cuda(), args)}
    torch.cuda.empty_cache()
    if not args.no_steps:
        result["base224_autocast_step"] = steps(cpu_model, args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
