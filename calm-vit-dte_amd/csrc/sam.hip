// Sharpness-aware minimisation: the perturbation w += rho * s / ||s|| along the TRUE gradient (corrected for the deferred
// spectral-norm layers, unscaled) of the first backward, and the way back, over calm_optim_step's own table
// (calm_sam_perturb: four launches, calm_sam_restore: one).  With inv = 1 / grad_scale (1 without a scale), all in fp32:
//     plain tensor            g' = G[i] * inv
//     spectral-norm tensor    c = <G, W_orig> / sigma;   g' = ((G[i] - c u[r] v[col]) * (1 / sigma)) * inv
//     direction               s = g'   |   adaptive (ASAM): t = |w[i]| + eta, s = t * g'
//   pass 1  sam_gw         chunks of spectral-norm tensors: the per-chunk partial of <G, W_orig> (chunk_gw_partial: the thread /
//                          block order of optim_stats, so c has the bits calm_optim_step, calm_grad_accum and
//                          calm_grad_stats give it); plain chunks write nothing
//   pass 2  sam_sq         every workgroup of a spectral-norm tensor forms c (tensor_sn_c), then per chunk: sum s^2 — a
//                          thread sums its elements serially, then block_sum_256 — and whether a RAW G[i] is inf / NaN
//   pass 3  sam_finalize   ONE workgroup: thread k owns tensors k, k + 256, ... in rising order: a tensor's chunk sums added
//                          in chunk order, the thread's tensors added serially, then block_sum_256; c of every spectral-norm
//                          tensor stored for pass 4; norm = sqrtf(total), found_inf, scale = found_inf ? 0 : rho / (norm + eps)
//   pass 4  sam_apply      backup[i] = w[i] (the bits), always; found_inf == 0: w[i] = w[i] + (adaptive ? scale * t : scale) * s
//   calm_sam_restore       w[i] = backup[i], bits moved as 32-bit words: no arithmetic touches them
// A chunk whose operand addresses (pass 2: grad + i0, adaptive also param + i0; pass 4: grad + i0 unless found_inf,
// param + i0, backup + i0; restore: param + i0, backup + i0) are all 16-byte aligned is read as 16-byte vectors with a
// single-word tail (a thread's serial sum then runs over its vectors' elements in address order), any other chunk as
// single words.  Every value has one writer and every sum a fixed order: no atomics, and no result depends on the grid.
#include "chunk_table.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = CHUNK_ELEMS;           // elements per work item (64 per thread)
constexpr int U = 4;                         // 16-byte vectors a thread has in flight per operand (pass 4, restore)

struct Globals { float norm, found_inf, scale, pad; };
// scratch layout: [n_chunks: <G, W_orig> partials][n_chunks: sum s^2][n_chunks: non-finite flag][n_tensors: c][Globals]

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e38f; }   // false for inf and NaN

__global__ __launch_bounds__(NT) void sam_gw(const calm_optim_tensor* __restrict__ T, const int* __restrict__ chunk_tensor,
                                             float* __restrict__ chunk_gw) {
    __shared__ float red[4];
    const calm_optim_tensor e = T[chunk_tensor[blockIdx.x]];
    if (!e.sn_sigma) return;
    const auto [i0, i1] = chunk_span(blockIdx.x, CHUNK, e.chunk0, e.numel);
    const float gw = chunk_gw_partial(e, i0, i1, red);
    if (threadIdx.x == 0) chunk_gw[blockIdx.x] = gw;
}

// what both passes over the elements know of a tensor: c and inv_sg only for SN, eta only for AD
struct Dir { float c, inv_sg, inv, eta; };

// s of one element, and t (1 unless AD)
template <bool SN, bool AD>
__device__ __forceinline__ float sam_s(const Dir& d, float gi, float wi, float u, float v, float& t) {
    const float x = (SN ? (gi - d.c * u * v) * d.inv_sg : gi) * d.inv;
    t = AD ? fabsf(wi) + d.eta : 1.f;
    return AD ? t * x : x;
}

struct Sq { float s2 = 0.f; int bad = 0; };

// pass 2 over one chunk [i0, i1) of tensor e
template <bool SN, bool AD>
__device__ __forceinline__ Sq sq_span(const calm_optim_tensor& e, long i0, long i1, const Dir& d) {
    const gf32* g = (const gf32*)e.grad;
    const gf32* p = (const gf32*)e.param;
    const gf32* su = (const gf32*)e.sn_u;
    const gf32* sv = (const gf32*)e.sn_v;
    const unsigned cols = (unsigned)e.cols;
    Sq a;
    const auto element = [&](float gi, float pi, unsigned r, unsigned cc) __attribute__((always_inline)) {
        a.bad |= !finite_f(gi);
        float t;
        const float s = sam_s<SN, AD>(d, gi, pi, SN ? su[r] : 0.f, SN ? sv[cc] : 0.f, t);
        a.s2 += s * s;
    };
    // the 32-bit row / column split of optim_update (rows * cols < 2^31, checked by the host)
    const auto scalar = [&](long b, long end) __attribute__((always_inline)) {
        for (long i = b + threadIdx.x; i < end; i += NT) {
            unsigned r = 0, cc = 0;
            if (SN) { r = (unsigned)i / cols; cc = (unsigned)i - r * cols; }
            element(g[i], AD ? p[i] : 0.f, r, cc);
        }
    };
    if (dev_aligned16(g + i0) && (!AD || dev_aligned16(p + i0))) {  // (the weights are an operand only with AD)
        const long v1 = i0 + ((i1 - i0) & ~3L);
#pragma unroll 2
        for (long i = i0 + 4 * threadIdx.x; i < v1; i += 4 * NT) {
            const f32x4 g4 = *(const gf32x4*)(g + i);
            f32x4 p4 = {0.f, 0.f, 0.f, 0.f};
            if (AD) p4 = *(const gf32x4*)(p + i);
            unsigned r = 0, cc = 0;
            if (SN) { r = (unsigned)i / cols; cc = (unsigned)i - r * cols; }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                element(g4[k], p4[k], r, cc);
                if (SN && ++cc == cols) { cc = 0; ++r; }         // (cols = 1: every element starts a row)
            }
        }
        scalar(v1, i1);
    } else {
        scalar(i0, i1);
    }
    return a;
}

template <bool AD>
__global__ __launch_bounds__(NT) void sam_sq(const calm_optim_tensor* __restrict__ T, const int* __restrict__ chunk_tensor,
                                             float eta, const float* __restrict__ grad_scale,
                                             const float* __restrict__ chunk_gw, float* __restrict__ chunk_s2,
                                             float* __restrict__ chunk_bad) {
    __shared__ float red[4];
    __shared__ float c_lds;
    const calm_optim_tensor e = T[chunk_tensor[blockIdx.x]];
    const auto [i0, i1] = chunk_span(blockIdx.x, CHUNK, e.chunk0, e.numel);
    Dir d{0.f, 1.f, grad_scale ? 1.0f / grad_scale[0] : 1.0f, eta};
    Sq a;
    if (e.sn_sigma) {                                            // (uniform over the workgroup)
        const float sg = e.sn_sigma[0];
        d.c = tensor_sn_c(e, chunk_gw, sg, &c_lds);
        d.inv_sg = 1.0f / sg;
        a = sq_span<true, AD>(e, i0, i1, d);
    } else {
        a = sq_span<false, AD>(e, i0, i1, d);
    }
    const float s2 = block_sum_256(a.s2, red);
    const float bad = block_sum_256((float)a.bad, red);          // at most 1 per thread: exact
    if (threadIdx.x == 0) { chunk_s2[blockIdx.x] = s2; chunk_bad[blockIdx.x] = bad > 0.f ? 1.f : 0.f; }
}

__global__ __launch_bounds__(NT) void sam_finalize(const calm_optim_tensor* __restrict__ T, int n, calm_sam_hparams hp,
                                                   const float* __restrict__ chunk_gw, const float* __restrict__ chunk_s2,
                                                   const float* __restrict__ chunk_bad, float* __restrict__ tensor_c,
                                                   Globals* __restrict__ G, float* __restrict__ out) {
    __shared__ float red[4];
    float acc = 0.f, bad = 0.f;
    for (int t = threadIdx.x; t < n; t += NT) {                  // this thread's tensors, in rising order
        const calm_optim_tensor e = T[t];
        const int nch = chunk_count(CHUNK, e.numel);
        float s2 = 0.f, gw = 0.f;
        for (int k = 0; k < nch; ++k) {                          // fixed order: chunk 0, 1, 2, ...
            s2 += chunk_s2[e.chunk0 + k];
            bad = fmaxf(bad, chunk_bad[e.chunk0 + k]);
            if (e.sn_sigma) gw += chunk_gw[e.chunk0 + k];
        }
        tensor_c[t] = e.sn_sigma ? gw / e.sn_sigma[0] : 0.f;     // the operations of tensor_sn_c: the same bits
        acc += s2;
    }
    acc = block_sum_256(acc, red);
    bad = block_sum_256(bad, red);                               // at most 256: exact
    if (threadIdx.x == 0) {
        const float norm = sqrtf(acc);
        const bool found = bad > 0.f || !finite_f(norm);
        const float scale = found ? 0.f : hp.rho / (norm + hp.eps);
        G->norm = norm; G->found_inf = found ? 1.f : 0.f; G->scale = scale; G->pad = 0.f;
        out[0] = norm; out[1] = found ? 1.f : 0.f; out[2] = scale;
    }
}

// pass 4 over one chunk [i0, i1) of tensor e: w -> b always; with MOVE also w + step -> w
template <bool MOVE, bool SN, bool AD>
__device__ __forceinline__ void apply_span(const calm_optim_tensor& e, gf32* b, long i0, long i1, const Dir& d, float scale) {
    const gf32* g = (const gf32*)e.grad;
    gf32* p = (gf32*)e.param;
    const gf32* su = (const gf32*)e.sn_u;
    const gf32* sv = (const gf32*)e.sn_v;
    const unsigned cols = (unsigned)e.cols;
    const auto moved = [&](float gi, float wi, unsigned r, unsigned cc) __attribute__((always_inline)) {
        float t;
        const float s = sam_s<SN, AD>(d, gi, wi, SN ? su[r] : 0.f, SN ? sv[cc] : 0.f, t);
        return wi + (AD ? scale * t : scale) * s;
    };
    const auto scalar = [&](long lo, long end) __attribute__((always_inline)) {
        for (long i = lo + threadIdx.x; i < end; i += NT) {
            const float wi = p[i];
            b[i] = wi;
            if (MOVE) {
                unsigned r = 0, cc = 0;
                if (SN) { r = (unsigned)i / cols; cc = (unsigned)i - r * cols; }
                p[i] = moved(g[i], wi, r, cc);
            }
        }
    };
    if (dev_aligned16(p + i0) && dev_aligned16(b + i0) && (!MOVE || dev_aligned16(g + i0))) {
        const long v1 = i0 + ((i1 - i0) & ~3L);
        struct Pair { f32x4 g, w; };
        const auto load = [&](long i) __attribute__((always_inline)) {
            Pair q;
            q.w = *(const gf32x4*)(p + i);
            q.g = MOVE ? *(const gf32x4*)(g + i) : q.w;         // found_inf: the gradient is not read
            return q;
        };
        const auto store = [&](long i, const Pair& q) __attribute__((always_inline)) {
            *(gf32x4*)(b + i) = q.w;
            if (MOVE) {
                unsigned r = 0, cc = 0;
                if (SN) { r = (unsigned)i / cols; cc = (unsigned)i - r * cols; }
                f32x4 out;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    out[k] = moved(q.g[k], q.w[k], r, cc);
                    if (SN && ++cc == cols) { cc = 0; ++r; }     // (cols = 1: every element starts a row)
                }
                *(gf32x4*)(p + i) = out;
            }
        };
        loads_ahead_of_stores<U, 4, NT>(i0, v1, load, store);
        scalar(v1, i1);
    } else {
        scalar(i0, i1);
    }
}

template <bool AD>
__global__ __launch_bounds__(NT) void sam_apply(const calm_optim_tensor* __restrict__ T, const int* __restrict__ chunk_tensor,
                                                float eta, const float* __restrict__ grad_scale,
                                                const float* __restrict__ tensor_c, const Globals* __restrict__ G,
                                                float* const* __restrict__ backup) {
    const int t = chunk_tensor[blockIdx.x];
    const calm_optim_tensor e = T[t];
    const auto [i0, i1] = chunk_span(blockIdx.x, CHUNK, e.chunk0, e.numel);
    gf32* b = (gf32*)backup[t];
    Dir d{0.f, 1.f, grad_scale ? 1.0f / grad_scale[0] : 1.0f, eta};
    const float scale = G->scale;
    if (G->found_inf != 0.f) {                                   // (uniform over the grid) no parameter is written
        apply_span<false, false, false>(e, b, i0, i1, d, 0.f);
    } else if (e.sn_sigma) {                                     // (uniform over the workgroup)
        d.c = tensor_c[t];
        d.inv_sg = 1.0f / e.sn_sigma[0];
        apply_span<true, true, AD>(e, b, i0, i1, d, scale);
    } else {
        apply_span<true, false, AD>(e, b, i0, i1, d, scale);
    }
}

__global__ __launch_bounds__(NT) void sam_restore(const calm_optim_tensor* __restrict__ T, const int* __restrict__ chunk_tensor,
                                                  const float* const* __restrict__ backup) {
    const int t = chunk_tensor[blockIdx.x];
    const calm_optim_tensor e = T[t];
    const auto [i0, i1] = chunk_span(blockIdx.x, CHUNK, e.chunk0, e.numel);
    gu32* p = (gu32*)e.param;
    const gu32* b = (const gu32*)backup[t];
    long v1 = i0;
    if (dev_aligned16(p + i0) && dev_aligned16(b + i0)) {
        v1 = i0 + ((i1 - i0) & ~3L);
        loads_ahead_of_stores<U, 4, NT>(i0, v1, [&](long i) __attribute__((always_inline)) { return *(const gu32x4*)(b + i); },
                                        [&](long i, const u32x4& w) __attribute__((always_inline)) { *(gu32x4*)(p + i) = w; });
    }
    loads_ahead_of_stores<U, 1, NT>(v1, i1, [&](long i) __attribute__((always_inline)) { return b[i]; },
                                    [&](long i, uint32_t w) __attribute__((always_inline)) { p[i] = w; });
}

}  // namespace

extern "C" {

int64_t calm_sam_scratch_floats(int32_t n_tensors, int32_t n_chunks) {
    if (n_tensors <= 0 || n_chunks <= 0) return CALM_E_INVAL;
    return 3 * (int64_t)n_chunks + n_tensors + (int64_t)(sizeof(Globals) / sizeof(float));
}

int calm_sam_perturb(const calm_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev,
                     int32_t n_chunks, const calm_sam_hparams* hp, const float* grad_scale, float* const* backup_dev,
                     float* scratch, float* stats_out, void* stream) {
    if (!tensors_dev || !chunk_tensor_dev || !hp || !backup_dev || !scratch || !stats_out || n_tensors <= 0 || n_chunks <= 0)
        return CALM_E_INVAL;
    if (!(hp->rho >= 0.f) || !(hp->eps > 0.f) || (hp->adaptive != 0 && hp->adaptive != 1)) return CALM_E_INVAL;   // (NaN too)
    if (hp->adaptive && !(hp->eta >= 0.f)) return CALM_E_INVAL;
    float* chunk_gw = scratch;
    float* chunk_s2 = scratch + n_chunks;
    float* chunk_bad = scratch + 2 * (size_t)n_chunks;
    float* tensor_c = scratch + 3 * (size_t)n_chunks;
    Globals* G = reinterpret_cast<Globals*>(tensor_c + n_tensors);
    const bool ad = hp->adaptive != 0;
    if (int e = calm_launch(sam_gw, n_chunks, NT, 0, stream, tensors_dev, chunk_tensor_dev, chunk_gw)) return e;
    if (int e = calm_launch(ad ? sam_sq<true> : sam_sq<false>, n_chunks, NT, 0, stream, tensors_dev, chunk_tensor_dev, hp->eta,
                            grad_scale, chunk_gw, chunk_s2, chunk_bad))
        return e;
    if (int e = calm_launch(sam_finalize, 1, NT, 0, stream, tensors_dev, n_tensors, *hp, chunk_gw, chunk_s2, chunk_bad,
                            tensor_c, G, stats_out))
        return e;
    return calm_launch(ad ? sam_apply<true> : sam_apply<false>, n_chunks, NT, 0, stream, tensors_dev, chunk_tensor_dev, hp->eta,
                       grad_scale, tensor_c, G, backup_dev);
}

int calm_sam_restore(const calm_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev,
                     int32_t n_chunks, const float* const* backup_dev, void* stream) {
    if (!tensors_dev || !chunk_tensor_dev || !backup_dev || n_tensors <= 0 || n_chunks <= 0) return CALM_E_INVAL;
    return calm_launch(sam_restore, n_chunks, NT, 0, stream, tensors_dev, chunk_tensor_dev, backup_dev);
}

}  // extern "C"
