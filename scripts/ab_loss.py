#!/usr/bin/env python3
"""Time the loss kernels (calm_soft_ce_*, calm_huber_tokens_*) against the stock-torch chains they replace: forward +
backward of the loss end, cross-entropy at (256, 1000) and (484, 1000), Huber at (256, 224) and (256, 48).

HIP events around `--iters` iterations after `--warmup` warm-up iterations; three figures per shape:
  torch   F.cross_entropy(z, y) / F.huber_loss(tokens.reshape(-1,S,S,3).permute(0,3,1,2), x), then .backward()
  fn      ops.SoftTargetCrossEntropyFn / ops.HuberTokensFn through autograd (what the trainer runs with the switch on)
  abi     the two entry points on preallocated tensors (no autograd, no allocation)
The time between the events includes the gaps the host leaves between launches: for the microsecond-sized cross-entropy
kernels the torch and fn columns are host-bound; the abi column is closest to kernel time.  Huber also reports achieved
bytes/s over the algorithmic bytes (tokens and x read forward; tokens, x read and dtokens written backward: 5 tensors of
4*B*3*S*S bytes) against the 8 TB/s HBM peak.  --out FILE writes the table as JSON."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import calm_vit_dte_amd as calm  # noqa: E402

HBM_PEAK = 8e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_loss.py times kernels: it needs the GPU")
    be = calm.backend.get_backend()
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for B, C in ((256, 1000), (484, 1000)):
        z = torch.randn(B, C, device="cuda", generator=gen).requires_grad_(True)
        y = torch.softmax(torch.randn(B, C, device="cuda", generator=gen), 1)
        one = torch.ones(1, device="cuda")
        row_stats, loss, dz = torch.empty(B, 2, device="cuda"), torch.empty((), device="cuda"), torch.empty(B, C, device="cuda")

        def run(fn):
            z.grad = None
            fn().backward()

        def abi():
            be.soft_ce_fwd(z.detach(), y, row_stats, loss, None, B, C)
            be.soft_ce_bwd(z.detach(), y, row_stats, one, dz, B, C)
        r = {"loss": "soft_ce", "B": B, "C": C,
             "torch_us": timed(lambda: run(lambda: F.cross_entropy(z, y)), args.iters, args.warmup),
             "fn_us": timed(lambda: run(lambda: calm.ops.SoftTargetCrossEntropyFn.apply(z, y)), args.iters, args.warmup),
             "abi_us": timed(abi, args.iters, args.warmup)}
        rows.append(r)
        print(f"soft CE  B {B} C {C}: torch {r['torch_us']:8.1f} us  fn {r['fn_us']:8.1f} us  abi {r['abi_us']:8.1f} us")
    for B, S in ((256, 224), (256, 48)):
        x = torch.randn(B, 3, S, S, device="cuda", generator=gen)
        tok = torch.randn(B, S, 3 * S, device="cuda", generator=gen).requires_grad_(True)
        one = torch.ones(1, device="cuda")
        loss, dt = torch.empty((), device="cuda"), torch.empty(B, S, 3 * S, device="cuda")

        def run(fn):
            tok.grad = None
            fn().backward()

        def abi():
            be.huber_tokens_fwd(tok.detach(), x, 1.0, loss, B, S)
            be.huber_tokens_bwd(tok.detach(), x, 1.0, one, dt, B, S)
        nbytes = 5 * 4 * B * 3 * S * S
        r = {"loss": "huber_tokens", "B": B, "S": S, "algorithmic_bytes": nbytes,
             "torch_us": timed(lambda: run(lambda: F.huber_loss(tok.reshape(-1, S, S, 3).permute(0, 3, 1, 2), x)),
                               args.iters, args.warmup),
             "fn_us": timed(lambda: run(lambda: calm.ops.HuberTokensFn.apply(tok, x)), args.iters, args.warmup),
             "abi_us": timed(abi, args.iters, args.warmup)}
        for k in ("torch", "fn", "abi"):
            r[k + "_bytes_per_s"] = nbytes / (r[k + "_us"] * 1e-6)
        rows.append(r)
        print(f"Huber    B {B} S {S}: torch {r['torch_us']:8.1f} us ({r['torch_bytes_per_s'] / 1e12:5.2f} TB/s)  "
              f"fn {r['fn_us']:8.1f} us ({r['fn_bytes_per_s'] / 1e12:5.2f} TB/s)  "
              f"abi {r['abi_us']:8.1f} us ({r['abi_bytes_per_s'] / 1e12:5.2f} TB/s, {100 * r['abi_bytes_per_s'] / HBM_PEAK:4.1f} % of 8 TB/s)")
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"iters": args.iters, "warmup": args.warmup, "hbm_peak_bytes_per_s": HBM_PEAK, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
