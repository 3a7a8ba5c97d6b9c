#!/usr/bin/env python3
"""Time the k-NN probe's retrieval (trainer.KnnProbe.neighbours: calm_gemm on the fp32 pipe + calm_knn_merge per bank chunk)
against the torch composition it stands in for — a matmul per chunk, torch.topk over the chunk's rows, cat, torch.topk again —
at Nq 4096, Nb 262 144, D 384, k 20, chunk 16 384, in the same run:

  probe        KnnProbe.neighbours as it is called (normalisation of the queries included)
  gemm         the 16 similarity GEMMs alone, into the probe's scratch
  merge cold   calm_knn_merge on the first chunk from an empty state (every element is a candidate: radix select + sort)
  merge warm   calm_knn_merge of the other 15 chunks into the state of the chunks before them (the compare pass, few survivors)
  torch        matmul + topk per chunk, cat, topk; and the same without the matmuls (topk / cat / topk alone)

HIP events around `--iters` iterations after `--warmup` warm-up iterations.  The merge reads the [Nq, chunk] fp32 scratch
once when the state is warm: its bytes/s are over those 4 * Nq * chunk bytes against the 8 TB/s HBM peak.  The torch
composition leaves ties unspecified; the probe's state is also compared with it (values equal, indices where there is no tie).
--out FILE writes the rows as JSON lines."""
import argparse
import json
import os
import sys
from importlib import import_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

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
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--nb", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ab_knn.py times kernels: it needs the GPU")
    trainer = import_module("calm_vit_dte_amd.trainer")
    be = calm.backend.get_backend()
    Nq, Nb, D, k, chunk = args.nq, args.nb, args.dim, args.k, args.chunk
    gen = torch.Generator(device="cuda").manual_seed(0)
    cent = torch.randn(1000, D, device="cuda", generator=gen)
    bank = cent[torch.arange(Nb, device="cuda") % 1000] + 0.7 * torch.randn(Nb, D, device="cuda", generator=gen)
    q = cent[torch.arange(Nq, device="cuda") % 1000] + 0.7 * torch.randn(Nq, D, device="cuda", generator=gen)
    probe = trainer.KnnProbe(1000, k=k, chunk=chunk, device="cuda")
    probe.add_bank(bank, torch.arange(Nb, device="cuda") % 1000)
    bn, _ = probe.bank()
    qn = torch.empty_like(q)                            # the probe's own normalisation: the comparison below is on bits
    be.knn_normalize(q, qn, torch.zeros(1, dtype=torch.int64, device="cuda"), Nq, D)
    spans = [(b, min(chunk, Nb - b)) for b in range(0, Nb, chunk)]
    scratch = torch.empty(Nq, chunk, device="cuda")

    def gemm(b, n):
        with calm.backend.fp32_matmul():
            be.gemm(qn, bn[b:b + n], scratch, Nq, n, D, (D, 1, 0, 0), (D, 1, 0, 0), (chunk, 0, 0))

    def empty():
        return (torch.full((Nq, k), float("-inf"), device="cuda"), torch.full((Nq, k), -1, dtype=torch.int64, device="cuda"))

    # the similarity chunks are kept (Nb * Nq * 4 bytes: 4 GiB at the default sizes) so that the merges can be timed alone
    sims = []
    for b, n in spans:
        gemm(b, n)
        sims.append(scratch[:, :n].clone())
    warm_s, warm_i = empty()
    be.knn_merge(sims[0], 0, warm_s, warm_i, Nq, spans[0][1], k)
    cold_s, cold_i = empty()

    def merge_cold():
        cold_s.fill_(float("-inf"))
        cold_i.fill_(-1)
        be.knn_merge(sims[0], 0, cold_s, cold_i, Nq, spans[0][1], k)
    rest_s, rest_i = warm_s.clone(), warm_i.clone()

    def merge_warm():
        rest_s.copy_(warm_s)
        rest_i.copy_(warm_i)
        for (b, n), s in zip(spans[1:], sims[1:]):
            be.knn_merge(s, b, rest_s, rest_i, Nq, n, k)

    def torch_topk(with_matmul):
        vals, idxs = [], []
        for (b, n), s in zip(spans, sims):
            if with_matmul:
                s = qn @ bn[b:b + n].t()
            v, i = s.topk(min(k, n), dim=1)
            vals.append(v)
            idxs.append(i + b)
        v, i = torch.cat(vals, dim=1), torch.cat(idxs, dim=1)
        top, at = v.topk(k, dim=1)
        return top, i.gather(1, at)

    it, wu = args.iters, args.warmup
    rows = [{"what": "shape", "Nq": Nq, "Nb": Nb, "D": D, "k": k, "chunk": chunk, "chunks": len(spans), "iters": it}]
    t_probe = timed(lambda: probe.neighbours(q), it, wu)
    t_gemm = timed(lambda: [gemm(b, n) for b, n in spans], it, wu)
    t_cold = timed(merge_cold, it, wu)
    t_warm = timed(merge_warm, it, wu) if len(spans) > 1 else 0.0
    t_torch = timed(lambda: torch_topk(True), it, wu)
    t_topk = timed(lambda: torch_topk(False), it, wu)
    per_gemm = t_gemm / len(spans)
    per_warm = t_warm / max(len(spans) - 1, 1)
    warm_bytes = 4.0 * Nq * chunk
    rows.append({"what": "probe", "neighbours_us": t_probe, "gemm_us": t_gemm, "merge_us": t_cold + t_warm,
                 "gemm_per_chunk_us": per_gemm, "merge_cold_chunk_us": t_cold, "merge_warm_chunk_us": per_warm,
                 "merge_warm_bytes_per_s": warm_bytes / (per_warm * 1e-6) if per_warm else 0.0})
    rows.append({"what": "torch", "matmul_topk_cat_topk_us": t_torch, "topk_cat_topk_us": t_topk})
    ps, pi = probe.neighbours(q)
    ts, ti = torch_topk(False)
    same = bool(torch.equal(ps, ts))
    untied = (ps[:, 1:] != ps[:, :-1]).all(dim=1)
    rows.append({"what": "agreement", "values_equal": same, "rows_without_ties": int(untied.sum()),
                 "indices_equal_on_those": bool(torch.equal(pi[untied], ti[untied]))})
    print(f"Nq {Nq} Nb {Nb} D {D} k {k} chunk {chunk} ({len(spans)} chunks)")
    print(f"probe.neighbours {t_probe:10.1f} us   = gemm {t_gemm:10.1f} us + merge {t_cold + t_warm:9.1f} us (+ normalise, fills)")
    print(f"per chunk: gemm {per_gemm:9.1f} us   merge cold {t_cold:9.1f} us   merge warm {per_warm:8.1f} us "
          f"({warm_bytes / max(per_warm, 1e-9) / 1e6:5.2f} TB/s, {100 * warm_bytes / max(per_warm, 1e-9) * 1e6 / HBM_PEAK:4.1f} % of 8 TB/s)")
    print(f"torch: matmul + topk + cat + topk {t_torch:10.1f} us   topk + cat + topk alone {t_topk:10.1f} us")
    print(f"agreement: values equal {same}, {int(untied.sum())} rows without ties, indices equal on those "
          f"{rows[-1]['indices_equal_on_those']}")
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
