"""Where the weight-gradient lane's kernels run: `python scripts/lane_overlap.py PARENT_kernel_trace.csv NEW_kernel_trace.csv
[steps]` on the kernel traces of two `rocprofv3 --kernel-trace --stats -f csv -- python bench.py ...` runs (a run of its
own per build).  Prints, in ms of kernel time per step: the lane's kernels (every stream but the busiest one of the new
trace), how much of them lies beside a main-stream kernel and beside which family, every family's time in both builds,
and the time with any kernel running.  DESIGN.md section 7, "weight-gradient lane"."""
import bisect
import collections
import csv
import sys

FAMILIES = ("gemm_f32", "splitk_reduce", "cnn_bwd", "cnn_fwd", "ln_bwd", "ln_fwd", "rope_bwd", "rope_fwd", "attn_bwd_kv_ring",
            "attn_bwd_dq_ring", "attn_bwd_q", "attn_bwd", "attn_fwd", "colsum", "grid_transpose")


def load(path):
    return [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], (r["Queue_Id"], r["Stream_Id"]))
            for r in csv.DictReader(open(path))]


def family(name):
    return next((f for f in FAMILIES if f in name), "other")


def union(rows):
    total, (cs, ce) = 0, (rows[0][0], rows[0][1])
    for s, e, *_ in rows[1:]:
        if s > ce:
            total, cs, ce = total + ce - cs, s, e
        else:
            ce = max(ce, e)
    return total + ce - cs


def main(parent_csv, new_csv, steps=7):
    ms = lambda ns: ns / 1e6 / steps
    par, new = sorted(load(parent_csv)), sorted(load(new_csv))
    main_stream = collections.Counter(r[3] for r in new).most_common(1)[0][0]
    on_main, lane = [r for r in new if r[3] == main_stream], [r for r in new if r[3] != main_stream]
    print(f"lane: {len(lane) / steps:g} kernels, {ms(sum(e - s for s, e, *_ in lane)):.2f} ms per step")
    starts, longest = [r[0] for r in on_main], max(e - s for s, e, *_ in on_main)
    beside = collections.Counter()
    for s, e, *_ in lane:
        j = bisect.bisect_left(starts, s - longest)
        while j < len(on_main) and on_main[j][0] < e:
            o = min(e, on_main[j][1]) - max(s, on_main[j][0])
            if o > 0:
                beside[family(on_main[j][2])] += o
            j += 1
    print(f"beside a main-stream kernel: {ms(sum(beside.values())):.2f} ms per step")
    for k, v in beside.most_common():
        print(f"    {k:20s} {ms(v):7.2f}")
    tot = lambda rows: collections.Counter({f: sum(e - s for s, e, n, _ in rows if family(n) == f) for f in FAMILIES + ("other",)})
    tp, tm, tl = tot(par), tot(on_main), tot(lane)
    print(f"{'family':20s} {'parent':>8s} {'new main':>8s} {'new lane':>8s}")
    for f in sorted(tp, key=lambda f: -tp[f]):
        print(f"{f:20s} {ms(tp[f]):8.2f} {ms(tm[f]):8.2f} {ms(tl[f]):8.2f}")
    print(f"any kernel running: parent {ms(union(par)):.2f}, new {ms(union(new)):.2f}, new main stream alone {ms(union(on_main)):.2f}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 7)
