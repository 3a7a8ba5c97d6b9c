"""TEST INFRASTRUCTURE: numpy emulation of calm_ema_update / calm_ema_swap (include/calm_vit.h, csrc/ema.hip) on CPU
tensors — the same two launches, the same walk over chunks of calm_ema_chunk_elems() elements of one entry and the same
split of a chunk into 16-byte vectors with a scalar tail (both addresses 16-byte aligned) or single words (any other
4-byte aligned pair).  `EmaMixin` adds ema_plan / ema_update / ema_swap to tests/emulated_backend.py's EmulatedBackend
(`EmulatedEmaBackend`) without editing it.  `fault=` plants one defect, for the checker's own test (tests/ema_f64.py):
  "count+1"   the weight is taken from n + 1 instead of n
  "tail"      the last chunk's scalar tail is left untouched
  "skip"      the update is applied although skip != 0
  "boundary"  the vector part ends 4 elements early and the tail starts where it should: 4 elements untouched
  "one-way"   the swap copies the average into the parameter and leaves the average as it was"""
import numpy as np
import torch

from emulated_backend import EmulatedBackend

CHUNK = 16384
EMA_CONSTANT, EMA_WARMUP = 0, 1
_f = np.float32


def emu_weight(decay, schedule, count, skip, weight_out, fault=None):
    """First launch (one thread): count int32[1], skip None or float32[1], weight_out float32[2] — numpy arrays."""
    n = int(count[0])
    if skip is not None and skip[0] != 0 and fault != "skip":
        weight_out[0], weight_out[1] = 0.0, 1.0
        return
    if fault == "count+1":
        n += 1
    d = _f(decay)
    if schedule == EMA_WARMUP:
        d = min(d, (_f(1.0) + _f(n)) / (_f(10.0) + _f(n)))            # numpy's fp32 division is correctly rounded
    weight_out[0], weight_out[1] = _f(1.0) - d, 0.0
    count[0] = int(count[0]) + 1


def _fma(w, d, e):
    """fmaf(w, d, e): the fp32 product is exact in float64; one rounding of the float64 sum stands in for the fused one."""
    return (np.float64(w) * d.astype(np.float64) + e.astype(np.float64)).astype(np.float32)


def _segments(src_addr, ema_addr, numel, fault=None):
    """[(begin, end, "vector" | "scalar")] in the order the workgroups of one entry walk it."""
    out = []
    n_chunks = (numel + CHUNK - 1) // CHUNK
    for k in range(n_chunks):
        i0, i1 = k * CHUNK, min((k + 1) * CHUNK, numel)
        if (src_addr + 4 * i0) % 16 == 0 and (ema_addr + 4 * i0) % 16 == 0:
            v1 = i0 + ((i1 - i0) & ~3)
            v_end = max(i0, v1 - 4) if fault == "boundary" else v1
            if v_end > i0:
                out.append((i0, v_end, "vector"))
            if i1 > v1 and not (fault == "tail" and k == n_chunks - 1):
                out.append((v1, i1, "scalar"))
        elif not (fault == "tail" and k == n_chunks - 1):
            out.append((i0, i1, "scalar"))
        else:                                                         # a scalar chunk's "tail": its last (i1 - i0) % 4 words
            out.append((i0, i0 + ((i1 - i0) & ~3), "scalar"))
    return out


def emu_update(pairs, weight_out, fault=None):
    """Second launch: pairs of (src, ema) contiguous fp32 CPU tensors, updated in place."""
    if weight_out[1] != 0:
        return
    w = _f(weight_out[0])
    for src, ema in pairs:
        x, e = src.detach().reshape(-1).numpy(), ema.detach().reshape(-1).numpy()
        for b, t, _ in _segments(src.data_ptr(), ema.data_ptr(), x.size, fault):
            e[b:t] = _fma(w, x[b:t] - e[b:t], e[b:t])


def emu_swap(pairs, fault=None):
    for src, ema in pairs:
        x, e = src.detach().reshape(-1).numpy().view(np.int32), ema.detach().reshape(-1).numpy().view(np.int32)
        for b, t, _ in _segments(src.data_ptr(), ema.data_ptr(), x.size):
            keep = x[b:t].copy()
            x[b:t] = e[b:t]
            if fault != "one-way":
                e[b:t] = keep


class EmuEmaPlan:
    def __init__(self, pairs):
        for src, ema in pairs:
            if src.dtype != torch.float32 or ema.dtype != torch.float32:
                raise TypeError(f"fp32 tensor expected, got {src.dtype} / {ema.dtype}")
            if not (src.is_contiguous() and ema.is_contiguous()):
                raise TypeError("weight EMA expects contiguous parameters and averages")
            if src.shape != ema.shape:
                raise ValueError("weight EMA shape mismatch")
        self.pairs = [(s, a) for s, a in pairs if s.numel() > 0]
        spans = sorted((t.data_ptr(), t.data_ptr() + 4 * t.numel()) for pr in self.pairs for t in pr)
        if any(b[0] < a[1] for a, b in zip(spans, spans[1:])):
            raise ValueError("weight EMA expects parameters and averages that do not overlap in memory")
        self.n = len(self.pairs)
        self.n_chunks = sum((s.numel() + CHUNK - 1) // CHUNK for s, _ in self.pairs)
        self.count_dev = torch.zeros(1, dtype=torch.int32)
        self.weight_out = torch.zeros(2, dtype=torch.float32)
        self.src_ptrs = np.asarray([s.data_ptr() for s, _ in self.pairs], dtype=np.uint64)
        self.ema_ptrs = np.asarray([a.data_ptr() for _, a in self.pairs], dtype=np.uint64)


class EmaMixin:
    """ema_plan / ema_update / ema_swap with HipBackend's signatures; `ema_fault` plants a defect (module docstring)."""
    ema_fault = None

    def ema_plan(self, pairs):
        return EmuEmaPlan(pairs)

    def ema_update(self, plan, decay, schedule, skip=None):
        if not (0.0 <= decay < 1.0) or schedule not in (EMA_CONSTANT, EMA_WARMUP):
            raise RuntimeError("calm_ema_update failed: code -1 (invalid argument/unsupported shape)")
        emu_weight(decay, schedule, plan.count_dev.numpy(), None if skip is None else skip.detach().numpy(),
                   plan.weight_out.numpy(), self.ema_fault)
        emu_update(plan.pairs, plan.weight_out.numpy(), self.ema_fault)

    def ema_swap(self, plan):
        emu_swap(plan.pairs, self.ema_fault)


class EmulatedEmaBackend(EmaMixin, EmulatedBackend):
    name = "emulated+ema"
