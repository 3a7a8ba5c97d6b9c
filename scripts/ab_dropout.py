#!/usr/bin/env python3
"""Time calm_dropout next to calm_add (the yardstick: an existing streaming kernel) at the two Base-224 stage-0 sizes, and
one stage-0 Base-224 self-attention block forward + backward with dropout off and on.

Kernel figures — achieved bytes/s over the algorithmic bytes, HIP events around `--iters` launches after `--warmup`:
  fp32 with residual   256*224*672 elements   x, residual read, y written: 12 bytes per element (what DropoutAddFn runs)
  bf16 in place        256*224*1344 elements  read and written once: 4 bytes per element (the MLP hidden state)
  calm_add             the same element counts, fp32: 12 bytes per element
Block figures — VMLA_Block(heads 12, 672 -> 672, sequence 224, MLP 1344) at batch 256, forward + backward, p = 0 and
p = 0.1, in fp32 and under autocast(bfloat16).
Every pair is measured in `--rounds` alternating rounds in one process; the table holds the median and the spread
(min .. max) over the rounds.  --out FILE writes it as JSON (profiles/dropout_ab.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import calm_vit_dte_amd as calm  # noqa: E402

HBM_PEAK = 8e12
ROWS = 256 * 224


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
    s = {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}
    if nbytes is not None:
        s["algorithmic_bytes"] = nbytes
        s["median_bytes_per_s"] = nbytes / (s["median_us"] * 1e-6)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block-iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_dropout.py times kernels: it needs the GPU")
    be = calm.backend.get_backend()
    gen = torch.Generator(device="cuda").manual_seed(0)
    key = calm.ops.draw_dropout_key(torch.device("cuda"))
    kernels = []
    for label, n, dtype, with_res in (("fp32 with residual", ROWS * 672, torch.float32, True),
                                      ("bf16 in place", ROWS * 1344, torch.bfloat16, False)):
        x = torch.randn(n, device="cuda", generator=gen).to(dtype)
        res = torch.randn(n, device="cuda", generator=gen) if with_res else None
        y = torch.empty_like(x) if with_res else x
        a, b, c = (torch.randn(n, device="cuda", generator=gen) for _ in range(3))
        t = alternate({"dropout": lambda: be.dropout(x, res, y, n, 0.1, key), "add": lambda: be.add(a, b, c, n)},
                      args.rounds, args.iters, args.warmup)
        drop_bytes = n * (12 if with_res else 4)
        row = {"case": label, "elements": n, "calm_dropout": summary(t["dropout"], drop_bytes),
               "calm_add": summary(t["add"], 12 * n)}
        kernels.append(row)
        d, ad = row["calm_dropout"], row["calm_add"]
        print(f"{label:19s} n {n:9d}: calm_dropout {d['median_us']:7.1f} us ({d['min_us']:.1f} .. {d['max_us']:.1f}) "
              f"{d['median_bytes_per_s'] / 1e12:5.2f} TB/s   calm_add {ad['median_us']:7.1f} us ({ad['min_us']:.1f} .. "
              f"{ad['max_us']:.1f}) {ad['median_bytes_per_s'] / 1e12:5.2f} TB/s")
    vt = calm.Vi_Tools_CNN_less_V2
    torch.manual_seed(0)
    blk = vt.VMLA_Block(12, 672, 672, 240, 224, 80, 224, 1344, force_reduce=False).cuda().train()
    xq = torch.randn(args.batch, 224, 672, device="cuda", generator=gen).requires_grad_(True)
    gy = torch.randn(args.batch, 224, 672, device="cuda", generator=gen)
    blocks = []
    for precision, autocast in (("fp32", False), ("autocast(bfloat16)", True)):
        def step(p):
            blk.dropout.p = blk.mlp[2].p = p
            xq.grad = None
            for prm in blk.parameters():
                prm.grad = None
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                y = blk(xq, state_manager=vt.ResidualStateManager(mode="sum"), mask=True)
            (y.float() * gy).sum().backward()
        t = alternate({"p0": lambda: step(0.0), "p01": lambda: step(0.1)}, args.rounds, args.block_iters, 2)
        row = {"precision": precision, "batch": args.batch, "p_0": summary(t["p0"]), "p_0.1": summary(t["p01"])}
        blocks.append(row)
        a, b = row["p_0"], row["p_0.1"]
        print(f"block fwd+bwd {precision:19s}: p=0 {a['median_us'] / 1e3:7.2f} ms ({a['min_us'] / 1e3:.2f} .. "
              f"{a['max_us'] / 1e3:.2f})   p=0.1 {b['median_us'] / 1e3:7.2f} ms ({b['min_us'] / 1e3:.2f} .. {b['max_us'] / 1e3:.2f})")
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "block_iters": args.block_iters,
                       "hbm_peak_bytes_per_s": HBM_PEAK, "kernels": kernels, "block": blocks}, f, indent=1)


if __name__ == "__main__":
    main()
