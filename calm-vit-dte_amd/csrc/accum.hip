// Gradient accumulation over micro-batches, between the backward and calm_optim_step: the gradients of one micro-batch
// are added to fp32 accumulators, and the spectral-norm weight-gradient correction of every deferred layer
//     dW_orig = (G - <G, W_orig/sigma> u v^T) / sigma          G = gradient w.r.t. the normalised weight
// is applied HERE, with the u, v, sigma of that micro-batch's forward (the power iteration advances them in place at
// every training forward, so raw G's summed over a window cannot be corrected once at its end).  The table is
// calm_optim_step's, walked the same way (chunk_table.h), in two launches:
//   pass 1  accum_gw      chunks of spectral-norm tensors: the per-chunk partial of <G, W_orig>, in the thread / block order
//                         of optim_stats (optim.hip: thread t adds elements i0 + t, i0 + t + 256, ... serially, then
//                         block_sum_256); chunks of plain tensors write nothing
//   pass 2  accum_apply   spectral-norm tensors: every workgroup sums its tensor's partials in chunk order (one thread,
//                         broadcast through LDS), c = gw / sigma, g' = (G[i] - c u[r] v[col]) * (1 / sigma);
//                         plain tensors: g' = G[i];   acc[i] = first ? g' : acc[i] + g'
// With first = 1 the accumulator is not read (it may hold NaN from a window that was skipped).  No unscale, no clip, no
// inf flag: a non-finite value stays one in the accumulator and calm_optim_step finds it at the window's end.
// A chunk whose grad + i0 and acc + i0 are both 16-byte aligned moves 16-byte vectors with a scalar tail, any other
// 4-byte aligned pair single words.  Every element belongs to one thread of one workgroup and c to its tensor alone: no
// atomics, and the result per element does not depend on the grid.
#include "chunk_table.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = CHUNK_ELEMS;           // elements per work item (64 per thread)
constexpr int U = 4;                         // 16-byte vectors a thread has in flight per tensor

__global__ __launch_bounds__(NT) void accum_gw(const calm_optim_tensor* __restrict__ T, const int* __restrict__ chunk_tensor,
                                               float* __restrict__ chunk_part) {
    __shared__ float red[4];
    const calm_optim_tensor e = T[chunk_tensor[blockIdx.x]];
    if (!e.sn_sigma) return;
    const auto [i0, i1] = chunk_span(blockIdx.x, CHUNK, e.chunk0, e.numel);
    const float gw = chunk_gw_partial(e, i0, i1, red);
    if (threadIdx.x == 0) chunk_part[blockIdx.x] = gw;
}

// one chunk [i0, i1) of tensor e: g (gradient) -> a (accumulator); c and inv_sg only for SN
template <bool FIRST, bool SN>
__device__ __forceinline__ void accum_span(const calm_optim_tensor& e, const gf32* g, gf32* a, long i0, long i1, float c,
                                           float inv_sg) {
    const gf32* u = (const gf32*)e.sn_u;
    const gf32* v = (const gf32*)e.sn_v;
    const unsigned cols = (unsigned)e.cols;
    // the 32-bit row / column split of optim_update (rows * cols < 2^31, checked by the host)
    const auto corrected = [&](float gi, unsigned r, unsigned cc) __attribute__((always_inline)) {
        return SN ? (gi - c * u[r] * v[cc]) * inv_sg : gi;
    };
    const auto scalar = [&](long b, long end) __attribute__((always_inline)) {
        for (long i = b + threadIdx.x; i < end; i += NT) {
            unsigned r = 0, cc = 0;
            if (SN) { r = (unsigned)i / cols; cc = (unsigned)i - r * cols; }
            const float x = corrected(g[i], r, cc);
            a[i] = FIRST ? x : a[i] + x;
        }
    };
    if (dev_aligned16(g + i0) && dev_aligned16(a + i0)) {
        const long v1 = i0 + ((i1 - i0) & ~3L);
        struct Pair { f32x4 g, a; };
        const auto load = [&](long i) __attribute__((always_inline)) {
            Pair p;
            p.g = *(const gf32x4*)(g + i);
            p.a = FIRST ? p.g : *(const gf32x4*)(a + i);        // first = 1: the old accumulator is never read
            return p;
        };
        const auto store = [&](long i, const Pair& p) __attribute__((always_inline)) {
            unsigned r = 0, cc = 0;
            if (SN) { r = (unsigned)i / cols; cc = (unsigned)i - r * cols; }
            f32x4 out;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float x = corrected(p.g[k], r, cc);
                out[k] = FIRST ? x : p.a[k] + x;
                if (SN && ++cc == cols) { cc = 0; ++r; }         // (cols = 1: every element starts a row)
            }
            *(gf32x4*)(a + i) = out;
        };
        loads_ahead_of_stores<U, 4, NT>(i0, v1, load, store);
        scalar(v1, i1);
    } else {
        scalar(i0, i1);
    }
}

template <bool FIRST>
__global__ __launch_bounds__(NT) void accum_apply(const calm_optim_tensor* __restrict__ T, const int* __restrict__ chunk_tensor,
                                                  float* const* __restrict__ acc, const float* __restrict__ chunk_part) {
    __shared__ float c_lds;
    const int t = chunk_tensor[blockIdx.x];
    const calm_optim_tensor e = T[t];
    const auto [i0, i1] = chunk_span(blockIdx.x, CHUNK, e.chunk0, e.numel);
    const gf32* g = (const gf32*)e.grad;
    gf32* a = (gf32*)acc[t];
    if (e.sn_sigma) {                                            // (uniform over the workgroup)
        const float sg = e.sn_sigma[0];
        const float c = tensor_sn_c(e, chunk_part, sg, &c_lds);
        accum_span<FIRST, true>(e, g, a, i0, i1, c, 1.0f / sg);
    } else {
        accum_span<FIRST, false>(e, g, a, i0, i1, 0.f, 1.f);
    }
}

}  // namespace

extern "C" {

int calm_grad_accum(const calm_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev,
                    int32_t n_chunks, float* const* acc_dev, float* scratch, int32_t first, void* stream) {
    if (!tensors_dev || !chunk_tensor_dev || !acc_dev || !scratch || n_tensors <= 0 || n_chunks <= 0) return CALM_E_INVAL;
    if (first != 0 && first != 1) return CALM_E_INVAL;
    if (int e = calm_launch(accum_gw, n_chunks, NT, 0, stream, tensors_dev, chunk_tensor_dev, scratch)) return e;
    return calm_launch(first ? accum_apply<true> : accum_apply<false>, n_chunks, NT, 0, stream, tensors_dev,
                       chunk_tensor_dev, acc_dev, scratch);
}

}  // extern "C"
