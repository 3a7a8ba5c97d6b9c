#!/usr/bin/env python3
"""What a snapshot of the training state costs the training thread on Base-224 with FusedClipAdamW and a weight EMA:

  parent    torch.save of model.state_dict(), FusedClipAdamW.state_dict() and ModelEMA.state_dict() — the way to keep that
            state before trainer.TrainState existed: one blocking device-to-host copy per tensor, then the write, all on
            the training thread.  Stall = wall time of the call (device idle before and after).
  new       TrainState.save_async: one calm_snapshot_pack launch; the copy runs on a side stream, the write on a thread.
            Stall = wall time of save_async + (time of the step that runs while the copy is in flight - time of a step
            with nothing in flight).  The steps behind it, while the writer thread is busy, are timed as well, and
            so is a step behind a pack alone (no copy): what of the difference is the pack kernel itself.
            The same three — nothing, a pack alone, save_async — in front of a WINDOW of `--after` steps issued back to
            back with one synchronise at its end: the stream never runs dry there, as in a training loop.

The step is the captured one (GraphedTrainStep, autocast(bfloat16) + GradScaler) at `--batch`; a step's time is a host
clock around the replay and a device synchronise.  Candidates alternate within each of `--rounds` rounds; the table holds
median and spread (min .. max).  Also: the achieved bytes/s of calm_snapshot_pack and calm_snapshot_unpack alone (HIP
events around `--iters` calls; bytes = payload read + payload written) beside the device-copy rate of the architecture
notes (6.29 TB/s, float4 copy).  Acceptance, a relation: the new stall is below the parent's by more than the spread of
both, and the step with a copy in flight is within the spread of the step without.  --out FILE writes JSON
(profiles/snapshot_ab.json)."""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import calm_vit_dte_amd as calm  # noqa: E402
from calm_vit_dte_amd import trainer  # noqa: E402

DEVICE_COPY_BYTES_PER_S = 6.29e12
BASE224 = dict(heads=12, seq_length=224, in_features=672, dim_step=48, mean_var_hidden=240, seq_len_step=16,
               seq_len_reduce=80, out_features=1000)
WEIGHT_SEED = 1234


def build_cpu_model():
    m = calm.ViT(torch.device("cpu"), type=8, force_reduce=False, generate=False, **BASE224)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in calm.synthetic_weights.make_params(shapes, WEIGHT_SEED).items()})
    return m


def summary(values, unit="ms"):
    return {f"median_{unit}": statistics.median(values), f"min_{unit}": min(values), f"max_{unit}": max(values),
            "rounds": list(values)}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--after", type=int, default=4, help="steps timed behind every save_async")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_snapshot.py times the GPU path: it needs the GPU")
    g = np.random.default_rng(0)
    x = torch.from_numpy(g.standard_normal((args.batch, 3, 224, 224)).astype(np.float32)).cuda()
    y = torch.zeros(args.batch, 1000, device="cuda")
    y[torch.arange(args.batch), torch.from_numpy(g.integers(0, 1000, args.batch)).cuda()] = 1.0
    m = copy.deepcopy(build_cpu_model()).cuda().train()
    opt = trainer.FusedClipAdamW(m)
    ema = trainer.ModelEMA(m)
    scaler = torch.amp.GradScaler("cuda")
    step = trainer.GraphedTrainStep(m, opt, x, y, scaler=scaler, autocast_dtype=torch.bfloat16, ema=ema)
    st = trainer.TrainState(m, opt, scaler=scaler, ema=ema, step=step)
    be = calm.backend.get_backend()
    tmp = tempfile.mkdtemp(prefix="snapshot_ab_")
    new_path, old_path = os.path.join(tmp, "new.snap"), os.path.join(tmp, "old.pt")

    def parent_save():
        torch.save({"model": m.state_dict(), "optim": opt.state_dict(), "ema": ema.state_dict()}, old_path)

    for _ in range(3):
        step(x, y)
    st.save_async(new_path, {"epoch": 0, "batch": 0, "step": 0})       # builds the plan and the pinned buffer
    st.wait()
    parent_save()
    plan = st._plan
    def window_ms(before):
        """`--after` steps back to back behind `before()`, one synchronise at the end: the stream never runs dry, as in a
        training loop (a step timed alone starts on an idle stream)."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        before()
        for _ in range(args.after):
            step(x, y)
            st.poll()
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        st.wait()
        return ms

    rows = {"window_plain": [], "window_behind_pack_only": [], "window_behind_save_async": [], "parent_stall": [], "save_async": [], "step_plain": [], "step_behind_pack_only": [], "step_copy_in_flight": [],
            "step_writer_busy": [], "file_in_place": []}
    for _ in range(args.rounds):
        rows["window_plain"].append(window_ms(lambda: None))
        rows["window_behind_pack_only"].append(window_ms(lambda: be.snapshot_pack(plan)))
        rows["window_behind_save_async"].append(window_ms(lambda: st.save_async(new_path, {"epoch": 0, "batch": 0, "step": 0})))
        rows["step_plain"].append(statistics.median(wall_ms(lambda: step(x, y)) for _ in range(args.after)))
        rows["parent_stall"].append(wall_ms(parent_save))
        torch.cuda.synchronize()                                   # the pack alone in front of a step: no copy, no writer
        t0 = time.perf_counter()
        be.snapshot_pack(plan)
        step(x, y)
        torch.cuda.synchronize()
        rows["step_behind_pack_only"].append(1e3 * (time.perf_counter() - t0))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.save_async(new_path, {"epoch": 0, "batch": 0, "step": 0})
        t1 = time.perf_counter()
        rows["save_async"].append(1e3 * (t1 - t0))
        behind = []
        for _ in range(args.after):
            t = time.perf_counter()
            step(x, y)
            torch.cuda.synchronize()
            behind.append(1e3 * (time.perf_counter() - t))
            st.poll()
        st.wait()
        rows["file_in_place"].append(1e3 * (time.perf_counter() - t0))
        rows["step_copy_in_flight"].append(behind[0])
        rows["step_writer_busy"].append(statistics.median(behind[1:]) if len(behind) > 1 else behind[0])
    res = {k: summary(v) for k, v in rows.items()}
    new_stall = [a + (b - c) for a, b, c in zip(rows["save_async"], rows["step_copy_in_flight"], rows["step_plain"])]
    res["new_stall"] = summary(new_stall)
    res["new_stall_in_a_window"] = summary([a - b for a, b in zip(rows["window_behind_save_async"], rows["window_plain"])])
    spread = lambda s: s["max_ms"] - s["min_ms"]  # noqa: E731
    res["accepted_stall"] = bool(res["parent_stall"]["median_ms"] - res["new_stall"]["median_ms"]
                                 > spread(res["parent_stall"]) + spread(res["new_stall"]))
    step_spread = max(spread(res["step_plain"]), spread(res["step_copy_in_flight"]))
    res["accepted_step"] = bool(abs(res["step_copy_in_flight"]["median_ms"] - res["step_plain"]["median_ms"]) <= step_spread)
    # the kernels alone
    payload = int(sum(plan.sizes))
    rates = {}
    for name, fn in (("calm_snapshot_pack", lambda: be.snapshot_pack(plan)), ("calm_snapshot_unpack", lambda: be.snapshot_unpack(plan))):
        us = []
        for r in range(args.rounds):
            for _ in range(3 if r == 0 else 1):
                fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            us.append(1e3 * a.elapsed_time(b) / args.iters)
        s = summary(us, "us")
        s.update(algorithmic_bytes=2 * payload, median_bytes_per_s=2 * payload / (s["median_us"] * 1e-6),
                 min_bytes_per_s=2 * payload / (s["max_us"] * 1e-6), max_bytes_per_s=2 * payload / (s["min_us"] * 1e-6))
        rates[name] = s
    opt.close()
    st.close()
    out = {"config": "base224, FusedClipAdamW, ModelEMA, captured autocast(bf16) step", "batch": args.batch,
           "rounds": args.rounds, "iters": args.iters, "tensors": plan.n, "chunks": plan.n_chunks, "payload_bytes": payload,
           "packed_bytes": plan.packed_bytes, "old_file_bytes": os.path.getsize(old_path),
           "new_file_bytes": os.path.getsize(new_path), "device_copy_bytes_per_s": DEVICE_COPY_BYTES_PER_S,
           "timings_ms": res, "kernels": rates}
    print(f"{plan.n} tensors, {payload / 1e6:.1f} MB payload in {plan.n_chunks} chunks")
    for k in ("parent_stall", "new_stall", "new_stall_in_a_window", "window_plain", "window_behind_pack_only",
              "window_behind_save_async", "save_async", "step_plain", "step_behind_pack_only", "step_copy_in_flight", "step_writer_busy", "file_in_place"):
        s = res[k]
        print(f"{k:22s} {s['median_ms']:9.2f} ms ({s['min_ms']:.2f} .. {s['max_ms']:.2f})")
    for k, s in rates.items():
        print(f"{k:22s} {s['median_us']:9.1f} us  {s['median_bytes_per_s'] / 1e12:.2f} TB/s "
              f"({s['min_bytes_per_s'] / 1e12:.2f} .. {s['max_bytes_per_s'] / 1e12:.2f}) of {DEVICE_COPY_BYTES_PER_S / 1e12:.2f} TB/s")
    print(f"accepted: stall {res['accepted_stall']}, step {res['accepted_step']}")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
