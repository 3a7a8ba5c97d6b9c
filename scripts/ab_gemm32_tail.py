#!/usr/bin/env python3
"""Compare per-shape GEMM tables (`bench.py --gemm-report`) of two or more builds of the library, e.g. the 128-row-only
build (-DCALM_GEMM_F32_TILE64=0, or the parent commit), the default planner and the always-64-row calibration build
(-DCALM_GEMM_F32_TILE64=2), each run through CALM_VIT_LIB on the same box.

    python scripts/ab_gemm32_tail.py base.csv new.csv [more.csv ...] [--min-ms 0.2]

Prints the rows of the first table with the time of every other table and its ratio, then totals: all shapes, shapes
below 90 TFLOP/s in the first table, and the rows of >= --min-ms that got more than 3 % slower."""
import csv
import sys


def load(path):
    rows = {}
    for r in csv.DictReader(open(path)):
        key = tuple(int(r[k]) for k in ("M", "N", "K", "batch", "a_kc", "b_kc", "reduce"))
        rows[key] = (float(r["ms_per_step"]), float(r["tflops"]), int(r["launches_per_step"]))
    return rows


def main(argv):
    min_ms = 0.2
    if "--min-ms" in argv:
        i = argv.index("--min-ms")
        min_ms = float(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    tabs = [load(p) for p in argv]
    base = tabs[0]
    print("M,N,K,batch,a_kc,b_kc,reduce,launches," + ",".join(f"ms[{i}],tf[{i}]" for i in range(len(tabs))) +
          "," + ",".join(f"ratio[{i}]" for i in range(1, len(tabs))))
    tot = [0.0] * len(tabs)
    tail = [0.0] * len(tabs)
    slower = [[] for _ in tabs]
    for key, (ms0, tf0, n) in sorted(base.items(), key=lambda kv: -kv[1][0]):
        vals = [t.get(key, (float("nan"), float("nan"), 0)) for t in tabs]
        for i, v in enumerate(vals):
            tot[i] += v[0]
            if tf0 < 90:
                tail[i] += v[0]
            if i and ms0 >= min_ms and v[0] > 1.03 * ms0:
                slower[i].append((key, ms0, v[0]))
        print(",".join(map(str, key)) + f",{n}," + ",".join(f"{v[0]:.3f},{v[1]:.1f}" for v in vals) + "," +
              ",".join(f"{v[0] / ms0:.3f}" for v in vals[1:]))
    for i, p in enumerate(argv):
        print(f"# [{i}] {p}: GEMM {tot[i]:.2f} ms/step, shapes below 90 TFLOP/s in [0]: {tail[i]:.2f} ms/step, "
              f"rows >= {min_ms} ms more than 3 % slower than [0]: {len(slower[i])}")
        for key, a, b in slower[i]:
            print(f"#     {key}: {a:.3f} -> {b:.3f} ms")


if __name__ == "__main__":
    main(sys.argv[1:])
