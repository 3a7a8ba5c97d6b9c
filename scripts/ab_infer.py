#!/usr/bin/env python3
"""Time the lean inference forward next to the stored (training) forward it is cut from.

Kernel pairs — stored (calm_attention_fwd / calm_attention16_fwd) against lean (calm_attention_infer /
calm_attention16_infer) at batch 256: fp32 S=224 H=6 hd=112 and S=80 H=6 hd=40, bf16 S=224 H=12 hd=56 and S=80 H=12 hd=20.
With --parent-lib FILE (another build of the library, e.g. the parent commit's) its stored entry points are timed in the
same rounds through a second ctypes handle, to show whether the training path moved.
Whole-model eval forward in images/s — Small-224 fp32 and Base-224 under autocast(bfloat16), batch --model-batch: stored
eager (the model under no_grad, switch off), lean eager (trainer.Predictor), lean graph (Predictor(graph=True)); with
--parent-lib also the stored eager forward of a child process that loads that library through CALM_VIT_LIB.
Every set is measured in `--rounds` alternating rounds in one process (HIP events around `--iters` launches); the table
holds the median and the spread (min .. max) over the rounds.  --out FILE writes it as JSON (profiles/infer_ab.json)."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import calm_vit_dte_amd as calm  # noqa: E402
import bench  # noqa: E402

INFER_SYMBOLS = ("calm_attention_infer", "calm_attention16_infer")
KERNEL_CASES = [("fp32", 224, 6, 112), ("fp32", 80, 6, 40), ("bf16", 224, 12, 56), ("bf16", 80, 12, 20)]
MODEL_CASES = [("small224", None), ("base224", torch.bfloat16)]


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


def summary(us):
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def show(s):
    return f"{s['median_us']:9.1f} us ({s['min_us']:.1f} .. {s['max_us']:.1f})"


def parent_entry_points(path):
    """calm_attention_fwd / calm_attention16_fwd of another build, typed like the package's own binding."""
    lib = ctypes.CDLL(path)
    for n in ("calm_attention_fwd", "calm_attention16_fwd"):
        res, argtypes = calm._lib.SIGNATURES[n]
        getattr(lib, n).restype, getattr(lib, n).argtypes = res, argtypes
    return lib


def kernel_pairs(args, parent):
    be = calm.backend.get_backend()
    stream = calm.backend._stream
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for prec, S, H, hd in KERNEL_CASES:
        B, D = args.batch, H * hd
        dt = torch.float32 if prec == "fp32" else torch.bfloat16
        rn = lambda *s, sc=1.0: (torch.randn(*s, device="cuda", generator=gen) * sc)   # noqa: E731
        q, k, v = rn(B, S, D, sc=0.5).to(dt), rn(B, S, D, sc=0.5).to(dt), rn(B, S, D).to(dt)
        w1, w2 = rn(2 * S, S, sc=S ** -0.5).to(dt), rn(S, 2 * S, sc=(2 * S) ** -0.5).to(dt)
        b1, b2 = rn(2 * S, sc=0.1), rn(S, sc=0.1)
        s1, s2 = torch.tensor([1.3], device="cuda"), torch.tensor([0.8], device="cuda")
        e = lambda *s, d=dt: torch.empty(*s, dtype=d, device="cuda")   # noqa: E731
        out, R, hp, hg, Mk = e(B, S, D), e(B, S, S), e(B, S, 2 * S), e(B, S, 2 * S), e(B, S, S)
        out2, Mk2 = e(B, S, D), e(B, S, S)
        ins = (q, k, v, w1, b1, s1, w2, b2, s2)
        if prec == "fp32":
            P = e(B, H, S, S)
            fns = {"stored": lambda: be.attn_fwd(*ins, out, R, hp, hg, Mk, P, B, S, S, H, hd),
                   "lean": lambda: be.attn_infer(*ins, out2, Mk2, B, S, S, H, hd)}
            saved = 4 * (5 + H) * S * S * B
            if parent is not None:
                ptrs = [t.data_ptr() for t in ins + (out, R, hp, hg, Mk, P)]
                fns["parent_stored"] = lambda: calm._lib.check(
                    parent.calm_attention_fwd(*ptrs, B, S, S, H, hd, stream()), "parent calm_attention_fwd")
        else:
            MkT, lse = e(B, S, S), e(B, H, S, d=torch.float32)
            fns = {"stored": lambda: be.attn16_fwd(*ins, out, R, hp, hg, Mk, MkT, lse, B, S, H, hd),
                   "lean": lambda: be.attn16_infer(*ins, out2, Mk2, B, S, H, hd)}
            saved = (2 * 6 * S * S + 4 * H * S) * B                       # R, hp, hg (2 S^2 each), MkT: bf16; lse
            if parent is not None:
                ptrs = [t.data_ptr() for t in ins + (out, R, hp, hg, Mk, MkT, lse)]
                fns["parent_stored"] = lambda: calm._lib.check(
                    parent.calm_attention16_fwd(*ptrs, B, S, H, hd, stream()), "parent calm_attention16_fwd")
        t = alternate(fns, args.rounds, args.iters, args.warmup)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), out2.view(torch.int16)) and torch.equal(Mk.view(torch.int16), Mk2.view(torch.int16))
        row = {"precision": prec, "B": B, "S": S, "H": H, "hd": hd, "bytes_not_written_by_lean": saved,
               **{n: summary(us) for n, us in t.items()}}
        row["lean_over_stored"] = row["lean"]["median_us"] / row["stored"]["median_us"]
        rows.append(row)
        print(f"{prec} B={B} S={S} H={H} hd={hd}: " + "   ".join(f"{n} {show(row[n])}" for n in t) +
              f"   lean/stored {row['lean_over_stored']:.3f}", flush=True)
    return rows


def model_forms(name, autocast, batch, forms, args):
    """{form: summary, images_per_s} of the eval forward of workload `name` at `batch`."""
    wl = bench.WORKLOADS[name]
    calm.backend.set_matmul_precision("fp32")
    model = bench.build_model(calm, wl["kw"], torch.device("cuda")).eval()
    S = wl["kw"]["seq_length"]
    x = torch.randn(batch, 3, S, S, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    trainer = sys.modules.get("calm_vit_dte_amd.trainer") or __import__("importlib").import_module("calm_vit_dte_amd.trainer")

    def stored():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast is not None):
            return model(x)
    fns = {}
    keep = []
    if "stored_eager" in forms:
        fns["stored_eager"] = stored
    if "lean_eager" in forms:
        eager = trainer.Predictor(model, autocast_dtype=autocast)
        fns["lean_eager"] = lambda: eager(x)
    if "lean_graph" in forms:
        graphed = trainer.Predictor(model, example_x=x, autocast_dtype=autocast, graph=True)
        keep.append(graphed)
        fns["lean_graph"] = lambda: graphed(x)
    t = alternate(fns, args.rounds, args.model_iters, 2)
    for g in keep:
        g.close()
    out = {}
    for n, us in t.items():
        out[n] = summary(us)
        out[n]["images_per_s"] = batch / (out[n]["median_us"] * 1e-6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--model-iters", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="batch of the kernel pairs")
    ap.add_argument("--model-batch", type=int, default=256)
    ap.add_argument("--parent-lib", default="", help="another build of libcalmvit_hip.so to time in the same rounds")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-models", action="store_true")
    ap.add_argument("--child-model", default="", help=argparse.SUPPRESS)       # internal: the parent-library child
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_infer.py times kernels: it needs the GPU")
    if args.child_model:
        # this process loaded --parent-lib through CALM_VIT_LIB: time its stored eager forward and print one JSON line
        name = args.child_model
        autocast = dict(MODEL_CASES)[name]
        print("CHILD " + json.dumps(model_forms(name, autocast, args.model_batch, ("stored_eager",), args)))
        return
    parent = parent_entry_points(args.parent_lib) if args.parent_lib else None
    result = {"iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "model_iters": args.model_iters,
              "parent_lib": bool(args.parent_lib)}
    if not args.skip_kernels:
        result["kernels"] = kernel_pairs(args, parent)
    if not args.skip_models:
        result["models"] = []
        for name, autocast in MODEL_CASES:
            row = {"workload": name, "precision": "fp32" if autocast is None else "autocast(bfloat16)",
                   "batch": args.model_batch}
            row.update(model_forms(name, autocast, args.model_batch, ("stored_eager", "lean_eager", "lean_graph"), args))
            torch.cuda.empty_cache()
            if args.parent_lib:
                cmd = [sys.executable, os.path.abspath(__file__), "--child-model", name, "--model-batch", str(args.model_batch),
                       "--rounds", str(args.rounds), "--model-iters", str(args.model_iters)]
                r = subprocess.run(cmd, env=dict(os.environ, CALM_VIT_LIB=os.path.abspath(args.parent_lib)),
                                   capture_output=True, text=True, timeout=900)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
                if r.returncode != 0 or not line:
                    raise SystemExit("parent-library child failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
                row["parent_stored_eager"] = json.loads(line[0][6:])["stored_eager"]
            result["models"].append(row)
            print(f"{name} {row['precision']} batch {args.model_batch}: " + "   ".join(
                f"{n} {row[n]['images_per_s']:8.0f} img/s ({row[n]['min_us'] / 1e3:.1f} .. {row[n]['max_us'] / 1e3:.1f} ms)"
                for n in ("stored_eager", "lean_eager", "lean_graph", "parent_stored_eager") if n in row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    if os.environ.get("CALM_VIT_LIB"):
        for n in INFER_SYMBOLS:                      # an older build has no lean entry points: bind what it does have
            calm._lib.SIGNATURES.pop(n, None)
    main()
