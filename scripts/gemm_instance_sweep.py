"""Smallest calm_gemm arguments per compiled kernel instance, found by asking calm_gemm_describe (host code: no GPU).

Writes tests/golden/gemm_f64_cases.json, the per-instance case table of tests/gemm_f64.py: for every entry of
gemm_f64.CENSUS the cheapest (fewest multiply-adds) ragged argument set of the sweep that plans it with more than one
tile in M and in N (a full tile, then a tail), a never-split launch (split_k = 1) where one exists.  Shapes are ragged by construction: M ends 5 past a multiple of 16 (8 where a
row-contiguous operand has to stay 16-byte stageable), N ends 8 past a multiple of 16, K has a tail shorter than the
k-tile and K % 8 == 4 wherever no bf16 / fp8 operand forbids it.  Re-run after any change to the cost models of
plan_gemm():

    python scripts/gemm_instance_sweep.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gemm_f64 as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gemm_f64_cases.json")
BATCHES = (1, 4, 16, 64, 256)
GRID = list(range(0, 2049, 64))
CAP = 2.2e9


def sizes(tail, smallest):
    return [s for s in sorted({g + tail for g in GRID} | {g + tail for g in (16, 32, 96, 144, 176, 208)}) if s >= smallest]


def classes():
    """(label, case fields, K candidates, layouts)"""
    out = []
    for lay in G.LAYOUTS:
        out.append(("f32", dict(dtype=G.F32), (36, 100), lay))
        out.append(("f32 one-element", dict(dtype=G.F32, scalar=1), (37,), lay))
        for sa, sb in ((0, 0), (1, 1), (1, 0), (0, 1)):
            for sk in (1, 2):
                out.append(("bf16 operands", dict(dtype=G.BF16, a_st=sa, b_st=sb, split_k=sk), (36, 40, 100, 104), lay))
        for sk in (1, 2):
            out.append(("bf16x3", dict(dtype=G.BF16X3, split_k=sk), (36, 100), lay))
    for lay in G.PIPE_LAYOUTS:
        out.append(("bf16 pipelined", dict(dtype=G.BF16, a_st=1, b_st=1, c_st=1), (164, 168, 196, 200), lay))
        out.append(("f32 pipelined", dict(dtype=G.F32, pipe32=1), (36, 100), lay))
    for sa in (G.ST_E4M3, G.ST_E5M2):
        out.append(("fp8", dict(dtype=G.BF16, a_st=sa, b_st=G.ST_E4M3), (80,), (1, 1)))
    return out


def main():
    lib = G.binding().load()
    best = {}
    n = 0
    for label, fields, Ks, (akc, bkc) in classes():
        case0 = G.full_case(dict(fields, akc=akc, bkc=bkc, M=1, N=1, K=1))
        with G.options(lib, case0):
            for M in sizes(5 if akc else 8, 8):
                for N in sizes(8, 8):
                    for K in Ks:
                        for b0 in BATCHES:
                            c = dict(case0, M=M, N=N, K=K, b0=b0)
                            if G.macs(c) > CAP:
                                continue
                            g = G.fake_args(c)
                            rc, plan = G.describe(lib, g)
                            n += 1
                            if rc:
                                continue
                            key = G.instance_key(g, plan)
                            # a full tile followed by a tail in M and in N (an interior tile boundary, the last of
                            # several tiles) wherever the plan allows it, then the fewest multiply-adds
                            single = M <= key.tile_m or N <= key.tile_n
                            rank = (c["split_k"] != 1, single, G.macs(c))
                            k = G.kernel_of(key)
                            if k not in best or rank < best[k][0]:
                                best[k] = (rank, dict(c, key=list(key), k_slices=plan["k_slices"]))
    missing = sorted(G.CENSUS - set(best))
    extra = sorted(set(best) - G.CENSUS)
    table = [best[k][1] for k in sorted(best) if k in G.CENSUS]
    for c in table:
        for f, v in G.CASE_DEFAULTS.items():        # keep the file short: defaults are implied
            if c.get(f) == v:
                del c[f]
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c, sort_keys=True) for c in table) + "\n]\n")
    print(f"{n} describes, {len(table)} of {len(G.CENSUS)} instances, largest {max(G.macs(c) for c in table):.3g} multiply-adds, "
          f"sum {sum(G.macs(c) for c in table):.3g}")
    print("missing:", missing)
    print("outside the census:", extra)


if __name__ == "__main__":
    main()
