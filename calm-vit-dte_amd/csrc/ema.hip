// Exponential moving average of ALL parameters, and its in-place exchange with the live weights (the weight EMA every
// ImageNet ViT recipe evaluates with: timm's ModelEmaV2, torch's AveragedModel) — a launch of its own behind
// calm_optim_step, which stays as it is:
//   pass 1  ema_weight   one thread: n = count; skipped (skip != 0): weight_out = {0, 1}, count untouched; otherwise
//                        d = decay | min(decay, (1 + n) / (10 + n)), weight_out = {1 - d, 0}, count = n + 1
//   pass 2  ema_update   per chunk: nothing if weight_out[1] != 0, otherwise ema += w * (src - ema)
//   swap    ema_swap     per chunk: src <-> ema, bits moved through integer registers (NaN payloads survive)
// Work item = chunk of CHUNK consecutive elements of one entry (the walk of chunk_table.h).  A chunk whose src + i0 and ema + i0 are both 16-byte aligned moves 16-byte vectors with a scalar tail;
// any other 4-byte aligned pair moves single words.  Every element belongs to one thread of one workgroup: no workgroup
// reads a word another one of the same launch writes, no atomics, and the result per element does not depend on the grid.
#include "chunk_table.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = CHUNK_ELEMS;           // elements per work item (64 per thread)
constexpr int U = 4;                         // 16-byte vectors a thread has in flight per tensor

__global__ void ema_weight(float decay, int schedule, int* __restrict__ count, const float* __restrict__ skip,
                           float* __restrict__ weight_out) {
    const int n = count[0];
    if (skip && skip[0] != 0.f) {
        weight_out[0] = 0.f;
        weight_out[1] = 1.f;
        return;
    }
    float d = decay;
    if (schedule == CALM_EMA_WARMUP) {
        const float nf = (float)n;
        d = fminf(decay, __fdiv_rn(1.0f + nf, 10.0f + nf));     // correctly rounded: the host evaluates the same fp32 formula
    }
    weight_out[0] = 1.0f - d;
    weight_out[1] = 0.f;
    count[0] = n + 1;
}

// src and ema are not __restrict__ for the compiler (they come out of a table), so the loads of U vectors are issued
// ahead of the first store (loads_ahead_of_stores): U x 2 x 16 bytes in flight per thread
__global__ __launch_bounds__(NT) void ema_update(const calm_ema_entry* __restrict__ E, const int* __restrict__ chunk_entry,
                                                 const float* __restrict__ weight) {
    if (weight[1] != 0.f) return;             // skipped step (inf/NaN gradients): the average keeps every bit
    const float w = weight[0];
    const calm_ema_entry e = E[chunk_entry[blockIdx.x]];
    const auto [i0, i1] = chunk_span(blockIdx.x, CHUNK, e.chunk0, e.numel);
    const gf32* src = (const gf32*)e.src;
    gf32* ema = (gf32*)e.ema;
    if (dev_aligned16(src + i0) && dev_aligned16(ema + i0)) {
        const long v1 = i0 + ((i1 - i0) & ~3L);
        struct Pair { f32x4 x, a; };
        const auto load = [&](long i) __attribute__((always_inline)) {
            return Pair{*(const gf32x4*)(src + i), *(const gf32x4*)(ema + i)};
        };
        const auto store = [&](long i, const Pair& v) __attribute__((always_inline)) {
            f32x4 r;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = fmaf(w, v.x[k] - v.a[k], v.a[k]);
            *(gf32x4*)(ema + i) = r;
        };
        loads_ahead_of_stores<U, 4, NT>(i0, v1, load, store);
        for (long i = v1 + threadIdx.x; i < i1; i += NT) ema[i] = fmaf(w, src[i] - ema[i], ema[i]);
    } else {
        for (long i = i0 + threadIdx.x; i < i1; i += NT) ema[i] = fmaf(w, src[i] - ema[i], ema[i]);
    }
}

__global__ __launch_bounds__(NT) void ema_swap(const calm_ema_entry* __restrict__ E, const int* __restrict__ chunk_entry) {
    const calm_ema_entry e = E[chunk_entry[blockIdx.x]];
    const auto [i0, i1] = chunk_span(blockIdx.x, CHUNK, e.chunk0, e.numel);
    gu32* s = (gu32*)e.src;
    gu32* a = (gu32*)e.ema;
    if (dev_aligned16(s + i0) && dev_aligned16(a + i0)) {
        const long v1 = i0 + ((i1 - i0) & ~3L);
        struct Pair { u32x4 x, y; };
        const auto load = [&](long i) __attribute__((always_inline)) {
            return Pair{*(const gu32x4*)(s + i), *(const gu32x4*)(a + i)};
        };
        const auto store = [&](long i, const Pair& v) __attribute__((always_inline)) {
            *(gu32x4*)(s + i) = v.y;
            *(gu32x4*)(a + i) = v.x;
        };
        loads_ahead_of_stores<U, 4, NT>(i0, v1, load, store);
        for (long i = v1 + threadIdx.x; i < i1; i += NT) { const uint32_t x = s[i]; s[i] = a[i]; a[i] = x; }
    } else {
        for (long i = i0 + threadIdx.x; i < i1; i += NT) { const uint32_t x = s[i]; s[i] = a[i]; a[i] = x; }
    }
}

}  // namespace

extern "C" {

int32_t calm_ema_chunk_elems(void) { return CHUNK; }

int calm_ema_update(const calm_ema_entry* entries_dev, int32_t n_entries, const int32_t* chunk_entry_dev,
                    int32_t n_chunks, float decay, int32_t schedule, int32_t* count_dev, const float* skip_dev,
                    float* weight_out, void* stream) {
    if (!entries_dev || !chunk_entry_dev || !count_dev || !weight_out || n_entries <= 0 || n_chunks <= 0)
        return CALM_E_INVAL;
    if (!(decay >= 0.f && decay < 1.f) || (schedule != CALM_EMA_CONSTANT && schedule != CALM_EMA_WARMUP))   // NaN fails both
        return CALM_E_INVAL;
    if (int e = calm_launch(ema_weight, 1, 1, 0, stream, decay, schedule, count_dev, skip_dev, weight_out)) return e;
    return calm_launch(ema_update, n_chunks, NT, 0, stream, entries_dev, chunk_entry_dev, weight_out);
}

int calm_ema_swap(const calm_ema_entry* entries_dev, int32_t n_entries, const int32_t* chunk_entry_dev,
                  int32_t n_chunks, void* stream) {
    if (!entries_dev || !chunk_entry_dev || n_entries <= 0 || n_chunks <= 0) return CALM_E_INVAL;
    return calm_launch(ema_swap, n_chunks, NT, 0, stream, entries_dev, chunk_entry_dev);
}

}  // extern "C"
