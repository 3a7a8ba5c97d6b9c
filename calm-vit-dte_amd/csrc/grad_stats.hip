// Gradient monitor: per-tensor statistics of the TRUE gradient (corrected for the deferred spectral-norm layers, unscaled),
// of the weights and of the Adam update direction, read off calm_optim_step's own table in front of the step, in three
// launches (calm_grad_stats).  With inv = 1 / grad_scale (1 without a scale), per tensor and all in fp32:
//     plain tensor            g' = G[i] * inv
//     spectral-norm tensor    c = <G, W_orig> / sigma;   g' = ((G[i] - c u[r] v[col]) * (1 / sigma)) * inv
//     direction               d = (1 / bc1) * (m / (sqrtf(v) * (1 / sqrtf(bc2)) + eps)),  bc = 1 - beta^t as update_chunk
//                             (optim.hip) forms them; t < 1: no direction, dir_sq = 0 and the moments are not read
//   pass 1  gstat_gw        chunks of spectral-norm tensors: the per-chunk partial of <G, W_orig> in the thread / block order
//                           of optim_stats (thread t adds elements i0 + t, i0 + t + 256, ... serially, then block_sum_256),
//                           so c has the bits calm_optim_step and calm_grad_accum give it; plain chunks write nothing
//   pass 2  gstat_chunks    every workgroup of a spectral-norm tensor sums the tensor's partials in chunk order (one thread,
//                           broadcast through LDS, as accum_apply does: chunks^2 serial loads per tensor — 36 chunks at
//                           most on Small-224; a tensor of 10^8 elements would want c formed once, in a launch of its
//                           own); then per chunk: sum g'^2 and max |g'| over the elements whose g' is
//                           finite, sum p^2, max |p|, sum d^2, and the count of RAW G[i] that are inf / NaN.  g'^2 is summed
//                           element by element — not optim_finalize's expanded |G|^2 - 2c u^T G v + ... form, which cancels
//                           where G is nearly c u v^T.  A thread sums its elements serially, then block_sum_256 /
//                           block_max_256; one record of CS floats per chunk
//   pass 3  gstat_finalize  ONE workgroup: thread k owns tensors k, k + 256, ...: the chunk records added (maxima taken) in
//                           chunk order, the record of out[] written, the sticky fields advanced; then the call's summary
// A chunk whose grad + i0, param + i0, exp_avg + i0 and exp_avg_sq + i0 are all 16-byte aligned is read as 16-byte vectors
// with a single-word tail (a thread's serial sum then runs over its vectors' elements in address order), any other chunk
// as single words.  Nothing but out, summary and scratch is written; every value has one writer and a fixed order: no
// atomics, and no result depends on the grid.
#include "chunk_table.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = CHUNK_ELEMS;           // elements per work item (64 per thread)
constexpr int CS = 6;                        // per-chunk record: grad_sq, grad_absmax, param_sq, param_absmax, dir_sq, nonfinite
// scratch layout: [n_chunks: <G, W_orig> partials][CS x n_chunks]

struct DirParams { float beta1, beta2, eps; int step; };

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e38f; }   // false for inf and NaN

__global__ __launch_bounds__(NT) void gstat_gw(const calm_optim_tensor* __restrict__ T, const int* __restrict__ chunk_tensor,
                                               float* __restrict__ chunk_gw) {
    __shared__ float red[4];
    const calm_optim_tensor e = T[chunk_tensor[blockIdx.x]];
    if (!e.sn_sigma) return;
    const auto [i0, i1] = chunk_span(blockIdx.x, CHUNK, e.chunk0, e.numel);
    const float gw = chunk_gw_partial(e, i0, i1, red);
    if (threadIdx.x == 0) chunk_gw[blockIdx.x] = gw;
}

struct Acc {
    float g2 = 0.f, gmax = 0.f, p2 = 0.f, pmax = 0.f, d2 = 0.f;
    int bad = 0;
};

// one chunk [i0, i1) of tensor e; c and inv_sg only for SN, the moments only with DIR
template <bool SN, bool DIR>
__device__ __forceinline__ Acc stats_span(const calm_optim_tensor& e, long i0, long i1, float c, float inv_sg, float inv,
                                          float inv_bc1, float inv_sqrt_bc2, float eps) {
    const gf32* g = (const gf32*)e.grad;
    const gf32* p = (const gf32*)e.param;
    const gf32* m = (const gf32*)e.exp_avg;
    const gf32* v = (const gf32*)e.exp_avg_sq;
    const gf32* su = (const gf32*)e.sn_u;
    const gf32* sv = (const gf32*)e.sn_v;
    const unsigned cols = (unsigned)e.cols;
    Acc a;
    const auto element = [&](float gi, float pi, float mi, float vi, unsigned r, unsigned cc) __attribute__((always_inline)) {
        a.bad += !finite_f(gi);
        const float x = (SN ? (gi - c * su[r] * sv[cc]) * inv_sg : gi) * inv;
        if (finite_f(x)) { a.g2 += x * x; a.gmax = fmaxf(a.gmax, fabsf(x)); }
        a.p2 += pi * pi;
        a.pmax = fmaxf(a.pmax, fabsf(pi));
        if (DIR) {
            const float d = inv_bc1 * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
            a.d2 += d * d;
        }
    };
    // the 32-bit row / column split of optim_update (rows * cols < 2^31, checked by the host)
    const auto scalar = [&](long b, long end) __attribute__((always_inline)) {
        for (long i = b + threadIdx.x; i < end; i += NT) {
            unsigned r = 0, cc = 0;
            if (SN) { r = (unsigned)i / cols; cc = (unsigned)i - r * cols; }
            element(g[i], p[i], DIR ? m[i] : 0.f, DIR ? v[i] : 0.f, r, cc);
        }
    };
    if (dev_aligned16(g + i0) && dev_aligned16(p + i0) && (!DIR || (dev_aligned16(m + i0) && dev_aligned16(v + i0)))) {
        const long v1 = i0 + ((i1 - i0) & ~3L);
#pragma unroll 2
        for (long i = i0 + 4 * threadIdx.x; i < v1; i += 4 * NT) {
            const f32x4 g4 = *(const gf32x4*)(g + i), p4 = *(const gf32x4*)(p + i);
            f32x4 m4 = {0.f, 0.f, 0.f, 0.f}, v4 = {0.f, 0.f, 0.f, 0.f};
            if (DIR) { m4 = *(const gf32x4*)(m + i); v4 = *(const gf32x4*)(v + i); }
            unsigned r = 0, cc = 0;
            if (SN) { r = (unsigned)i / cols; cc = (unsigned)i - r * cols; }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                element(g4[k], p4[k], m4[k], v4[k], r, cc);
                if (SN && ++cc == cols) { cc = 0; ++r; }         // (cols = 1: every element starts a row)
            }
        }
        scalar(v1, i1);
    } else {
        scalar(i0, i1);
    }
    return a;
}

__global__ __launch_bounds__(NT) void gstat_chunks(const calm_optim_tensor* __restrict__ T, const int* __restrict__ chunk_tensor,
                                                   DirParams dp, const int* __restrict__ step_dev,
                                                   const float* __restrict__ grad_scale, const float* __restrict__ chunk_gw,
                                                   float* __restrict__ chunk_rec) {
    __shared__ float red[4];
    __shared__ float c_lds;
    const calm_optim_tensor e = T[chunk_tensor[blockIdx.x]];
    const auto [i0, i1] = chunk_span(blockIdx.x, CHUNK, e.chunk0, e.numel);
    const float inv = grad_scale ? 1.0f / grad_scale[0] : 1.0f;
    const int t = step_dev ? step_dev[0] : dp.step;
    const bool dir = t >= 1;                                     // (uniform over the grid)
    float inv_bc1 = 0.f, inv_sqrt_bc2 = 0.f;
    if (dir) {
        const float bc1 = 1.0f - powf(dp.beta1, (float)t), bc2 = 1.0f - powf(dp.beta2, (float)t);
        inv_bc1 = 1.0f / bc1;
        inv_sqrt_bc2 = 1.0f / sqrtf(bc2);
    }
    Acc a;
    if (e.sn_sigma) {                                            // (uniform over the workgroup)
        const float sg = e.sn_sigma[0];
        const float c = tensor_sn_c(e, chunk_gw, sg, &c_lds), inv_sg = 1.0f / sg;
        a = dir ? stats_span<true, true>(e, i0, i1, c, inv_sg, inv, inv_bc1, inv_sqrt_bc2, dp.eps)
                : stats_span<true, false>(e, i0, i1, c, inv_sg, inv, 0.f, 0.f, 0.f);
    } else {
        a = dir ? stats_span<false, true>(e, i0, i1, 0.f, 1.f, inv, inv_bc1, inv_sqrt_bc2, dp.eps)
                : stats_span<false, false>(e, i0, i1, 0.f, 1.f, inv, 0.f, 0.f, 0.f);
    }
    const float g2 = block_sum_256(a.g2, red), gmax = block_max_256(a.gmax, red);
    const float p2 = block_sum_256(a.p2, red), pmax = block_max_256(a.pmax, red);
    const float d2 = block_sum_256(a.d2, red);
    const float bad = block_sum_256((float)a.bad, red);          // at most 64 per thread, CHUNK per workgroup: exact
    if (threadIdx.x == 0) {
        float* rec = chunk_rec + (long)CS * blockIdx.x;
        rec[0] = g2; rec[1] = gmax; rec[2] = p2; rec[3] = pmax; rec[4] = d2; rec[5] = bad;
    }
}

__global__ __launch_bounds__(NT) void gstat_finalize(const calm_optim_tensor* __restrict__ T, int n,
                                                     const float* __restrict__ chunk_rec, calm_grad_stat* __restrict__ out,
                                                     int* __restrict__ summary) {
    __shared__ int first_lds[NT / CALM_WAVE];
    const int call = summary[0];                                 // this call's 0-based index
    int first = 0x7fffffff;                                      // the lowest tensor of this thread with a non-finite G
    for (int t = threadIdx.x; t < n; t += NT) {
        const calm_optim_tensor e = T[t];
        const int nch = chunk_count(CHUNK, e.numel);
        calm_grad_stat s = out[t];                               // (the sticky fields are carried over)
        float g2 = 0.f, gmax = 0.f, p2 = 0.f, pmax = 0.f, d2 = 0.f;
        int bad = 0;
        for (int k = 0; k < nch; ++k) {                          // fixed order: chunk 0, 1, 2, ...
            const float* rec = chunk_rec + (long)CS * (e.chunk0 + k);
            g2 += rec[0]; gmax = fmaxf(gmax, rec[1]); p2 += rec[2]; pmax = fmaxf(pmax, rec[3]); d2 += rec[4];
            bad += (int)rec[5];
        }
        s.grad_sq = g2; s.grad_absmax = gmax; s.param_sq = p2; s.param_absmax = pmax; s.dir_sq = d2; s.nonfinite = bad;
        if (bad > 0) {
            s.bad_calls += 1;
            if (s.first_bad_call < 0) s.first_bad_call = call;
            first = min(first, t);
        }
        out[t] = s;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
    if ((threadIdx.x & 63) == 0) first_lds[threadIdx.x >> 6] = first;
    __syncthreads();
    if (threadIdx.x == 0) {
        first = min(min(first_lds[0], first_lds[1]), min(first_lds[2], first_lds[3]));
        summary[0] = call + 1;
        if (first != 0x7fffffff) {
            summary[1] += 1;
            if (summary[2] < 0) { summary[2] = call; summary[3] = first; }
        }
    }
}

}  // namespace

extern "C" {

int64_t calm_grad_stats_scratch_floats(int32_t n_tensors, int32_t n_chunks) {
    if (n_tensors <= 0 || n_chunks <= 0) return CALM_E_INVAL;
    return (int64_t)(1 + CS) * n_chunks;
}

int calm_grad_stats(const calm_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev,
                    int32_t n_chunks, const calm_optim_hparams* hp, const int32_t* step_dev, const float* grad_scale,
                    calm_grad_stat* out_dev, int32_t* summary_dev, float* scratch, void* stream) {
    if (!tensors_dev || !chunk_tensor_dev || !hp || !out_dev || !summary_dev || !scratch || n_tensors <= 0 || n_chunks <= 0)
        return CALM_E_INVAL;
    if (hp->beta1 < 0.f || hp->beta1 >= 1.f || hp->beta2 < 0.f || hp->beta2 >= 1.f) return CALM_E_INVAL;
    float* chunk_gw = scratch;
    float* chunk_rec = scratch + n_chunks;
    const DirParams dp{hp->beta1, hp->beta2, hp->eps, hp->step};
    if (int e = calm_launch(gstat_gw, n_chunks, NT, 0, stream, tensors_dev, chunk_tensor_dev, chunk_gw)) return e;
    if (int e = calm_launch(gstat_chunks, n_chunks, NT, 0, stream, tensors_dev, chunk_tensor_dev, dp, step_dev, grad_scale,
                            chunk_gw, chunk_rec))
        return e;
    return calm_launch(gstat_finalize, 1, NT, 0, stream, tensors_dev, n_tensors, chunk_rec, out_dev, summary_dev);
}

}  // extern "C"
