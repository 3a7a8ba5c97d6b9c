#!/usr/bin/env python3
"""Time the kernels of the generative job (csrc/recon.hip) against the torch compositions they stand in for, at (256, 224)
and (256, 48):

  calm_recon_metrics     one call (two launches) on fp32 and on bf16 tokens, rows and NCHW target, with and without SSIM,
                         against trainer.recon_metrics_torch (the fp32 conv2d / elementwise composition) on the same tensors
  the rows Huber pair    forward + backward: F.huber_loss(tokens, target).backward(), ops.HuberRowsFn through autograd, and
                         the two entry points on preallocated tensors

HIP events around `--iters` iterations after `--warmup` warm-up iterations (the time between the events includes the gaps
the host leaves between launches; the abi columns are closest to kernel time).  Achieved bytes/s are over the ALGORITHMIC
bytes — metrics: both tensors read once (4 or 2 bytes per token element, 4 per target element; the halo rows the SSIM bands
read again are not counted); Huber: tokens and target read forward, both read and dtokens written backward, 5 tensors of
4 * B * 3 * S * S bytes — against the 8 TB/s HBM peak.  --out FILE writes the table as JSON."""
import argparse
import json
import os
import sys
from importlib import import_module

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
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_recon.py times kernels: it needs the GPU")
    trainer = import_module("calm_vit_dte_amd.trainer")
    lib = import_module("calm_vit_dte_amd._lib")
    be = calm.backend.get_backend()
    mean, std = trainer.DeviceCollate.MEAN, trainer.DeviceCollate.STD
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for B, S in ((256, 224), (256, 48)):
        target = torch.randn(B, S, 3 * S, device="cuda", generator=gen)
        tok32 = target + 0.2 * torch.randn(B, S, 3 * S, device="cuda", generator=gen)
        image = target.reshape(B, S, S, 3).permute(0, 3, 1, 2).contiguous()
        sums = torch.zeros(8, dtype=torch.float64, device="cuda")
        rec = torch.empty(be.recon_scratch_floats(B, S), dtype=torch.float32, device="cuda")
        for dtype in (torch.float32, torch.bfloat16):
            tok = tok32.to(dtype)
            for layout, tgt in (("rows", target), ("nchw", image)):
                for ssim in (True, False):
                    nbytes = B * 3 * S * S * (tok.element_size() + 4)
                    code = lib.RECON_NCHW if layout == "nchw" else lib.RECON_ROWS
                    r = {"what": "recon_metrics", "B": B, "S": S, "tokens": str(dtype)[6:], "target": layout, "ssim": ssim,
                         "algorithmic_bytes": nbytes,
                         "abi_us": timed(lambda: be.recon_metrics(tok, tgt, code, mean, std, 1.0, ssim, sums, B, S, rec),
                                         args.iters, args.warmup),
                         "torch_us": timed(lambda: trainer.recon_metrics_torch(tok, tgt, mean, std, 1.0, ssim, sums),
                                           max(args.iters // 10, 3), 2)}
                    for k in ("abi", "torch"):
                        r[k + "_bytes_per_s"] = nbytes / (r[k + "_us"] * 1e-6)
                    rows.append(r)
                    print(f"metrics B {B} S {S} {r['tokens']:8s} {layout:4s} ssim {int(ssim)}: torch {r['torch_us']:9.1f} us  "
                          f"abi {r['abi_us']:8.1f} us ({r['abi_bytes_per_s'] / 1e12:5.2f} TB/s, "
                          f"{100 * r['abi_bytes_per_s'] / HBM_PEAK:4.1f} % of 8 TB/s)")
        tok = tok32.clone().requires_grad_(True)
        one = torch.ones(1, device="cuda")
        loss, dt = torch.empty((), device="cuda"), torch.empty(B, S, 3 * S, device="cuda")
        n = tok.numel()

        def run(fn):
            tok.grad = None
            fn().backward()

        def abi():
            be.huber_rows_fwd(tok.detach(), target, 1.0, loss, n)
            be.huber_rows_bwd(tok.detach(), target, 1.0, one, dt, n)
        nbytes = 5 * 4 * n
        r = {"what": "huber_rows", "B": B, "S": S, "algorithmic_bytes": nbytes,
             "torch_us": timed(lambda: run(lambda: F.huber_loss(tok, target)), args.iters, args.warmup),
             "fn_us": timed(lambda: run(lambda: calm.ops.HuberRowsFn.apply(tok, target)), args.iters, args.warmup),
             "abi_us": timed(abi, args.iters, args.warmup)}
        for k in ("torch", "fn", "abi"):
            r[k + "_bytes_per_s"] = nbytes / (r[k + "_us"] * 1e-6)
        rows.append(r)
        print(f"Huber rows B {B} S {S}: torch {r['torch_us']:8.1f} us ({r['torch_bytes_per_s'] / 1e12:5.2f} TB/s)  "
              f"fn {r['fn_us']:8.1f} us ({r['fn_bytes_per_s'] / 1e12:5.2f} TB/s)  "
              f"abi {r['abi_us']:8.1f} us ({r['abi_bytes_per_s'] / 1e12:5.2f} TB/s, {100 * r['abi_bytes_per_s'] / HBM_PEAK:4.1f} % of 8 TB/s)")
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"iters": args.iters, "warmup": args.warmup, "hbm_peak_bytes_per_s": HBM_PEAK, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
