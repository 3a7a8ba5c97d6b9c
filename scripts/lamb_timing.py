#!/usr/bin/env python3
"""What does calm_optim_step_lamb cost on the MI355X, next to calm_optim_step?

On the parameter set of the Small-224 model (its tensors, shapes and deferred spectral-norm layers; random gradients, a
learning rate of 1e-6 so that a few thousand steps leave the weights where they are): calm_optim_step_lamb ungrouped, with
always_adapt, and with the two "no_decay" groups, against calm_optim_step twice, as two variants of its own — their
difference and their min .. max over the repeats are the spread every other difference is read against.

The word model (words of 4 bytes per element that the launches request): calm_optim_step reads G in its first pass and
reads G, w, m, v and writes w, m, v in its third: 8.  LAMB reads G in the first pass, reads G, w, m, v and writes m, v in
the third (6) and reads w, m, v and writes w in the fourth (4): 11.  A deferred tensor adds one word (w for <G, W_orig>) to
either.  By words LAMB is expected at about 11 / 8 of calm_optim_step.

Device time is between two events around `--iters` calls, after a warm-up, as the median of `--repeats` windows with
min .. max beside it; the variants alternate inside every repeat, in one process.  One JSON line per figure, each with the
sha256 of the kernel sources it was measured with; --out also writes them to a file (default profiles/lamb_timing.jsonl).
The run stops itself after --limit seconds.  Needs a GPU."""
import argparse
import json
import os
import signal
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


def kernels(args, stamp):
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
        small = [int(r["param"].dim() <= 1) for r in recs]
        plans = {k: be.optim_plan(recs) for k in ("step", "step_again", "lamb", "lamb_always")}
        plans["lamb_no_decay_groups"] = be.optim_plan([dict(r, group=g) for r, g in zip(recs, small)], n_groups=2)
        for p in plans.values():
            p.step_dev.fill_(1000)
        rates = [(1e-6, 0.02), (1e-6, 0.0)]
        fns = {"step": lambda: be.optim_step(plans["step"], grads, hp, None, stats),
               "lamb": lambda: be.optim_step_lamb(plans["lamb"], grads, hp, (None, False), None, stats),
               "step_again": lambda: be.optim_step(plans["step_again"], grads, hp, None, stats),
               "lamb_always": lambda: be.optim_step_lamb(plans["lamb_always"], grads, hp, (10.0, True), None, stats),
               "lamb_no_decay_groups": lambda: be.optim_step_lamb(plans["lamb_no_decay_groups"], grads, hp, (None, False), None,
                                                                  stats, group_hp=rates)}
        w = windows(fns, args.iters, args.repeats, 20)
        assert float(stats[1]) == 0.0
        trust = plans["lamb"].lamb_trust[:, 2]
        assert bool(torch.isfinite(trust).all()) and bool((trust > 0).all())
    finally:
        opt.close()
    elements = sum(x["param"].numel() for x in recs)
    deferred = sum(x["param"].numel() for x in recs if x["sn"] is not None)
    step = 0.5 * (w["step"][0] + w["step_again"][0])
    spread = max(abs(w["step"][0] - w["step_again"][0]), w["step"][2] - w["step"][1], w["step_again"][2] - w["step_again"][1])
    moved = {"step": 4 * (8 * elements + deferred), "lamb": 4 * (11 * elements + deferred)}
    emit(what="calm_optim_step_lamb against calm_optim_step, Small-224 parameter set", source_sha256=stamp, tensors=len(recs),
         chunks=plans["lamb"].n_chunks, elements=elements, deferred_tensors=sum(x["sn"] is not None for x in recs),
         deferred_elements=deferred, iters=args.iters, repeats=args.repeats,
         median_min_max_us={k: [round(x, 2) for x in v] for k, v in w.items()}, step_us=round(step, 2), spread_us=round(spread, 2),
         lamb_over_step={k: round(w[k][0] / step, 3) for k in ("lamb", "lamb_always", "lamb_no_decay_groups")},
         expected_by_words=round(moved["lamb"] / moved["step"], 3), spread_over_step=round(spread / step, 3), moved_bytes=moved,
         moved_gb_per_s={"step": round(moved["step"] / (step * 1e-6) / 1e9, 1),
                         "lamb": round(moved["lamb"] / (w["lamb"][0] * 1e-6) / 1e9, 1)},
         lamb_within_words_plus_spread=bool(w["lamb"][0] <= step * moved["lamb"] / moved["step"] + spread))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--limit", type=int, default=300, help="seconds after which the run stops itself")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lamb_timing.jsonl"), help="the JSON lines' file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lamb_timing: no GPU — nothing measured")

    def expired(*_):
        print(f"lamb_timing: stopped after {args.limit} s", flush=True)
        os._exit(3)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(args.limit)
    stamp = source_stamp()
    try:
        emit(what="box", device=torch.cuda.get_device_name(0), torch=torch.__version__)
        kernels(args, stamp)
    finally:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.writelines(json.dumps(r) + "\n" for r in LINES)


if __name__ == "__main__":
    main()
