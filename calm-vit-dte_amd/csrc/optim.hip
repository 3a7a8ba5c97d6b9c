// Optimizer-side step of the training iteration in three launches over ALL parameters
// (distributed_trainer_cls.py:88-96,158: GradScaler.unscale_ + inf check, clip_grad_norm_(1.0), AdamW(lr, betas, wd),
// zero_grad) — the reference issues one foreach/fused ATen call per stage over 521 tensors; here also the
// spectral-norm weight-gradient correction of every deferred layer is folded in (otherwise 2 launches per layer in
// backward, ~600 per step):
//     dW_orig = (G - <G, W_orig/sigma> u v^T) / sigma          G = gradient w.r.t. the normalised weight
//   pass 1  optim_stats     per chunk: sum g^2, non-finite flag; deferred layers also <G, W_orig> and u^T G v — stored
//                           as per-chunk partials (no atomics: every sum below has a fixed order, so the clip
//                           coefficient and the correction coefficients are bit-identical on all data-parallel ranks)
//   pass 2  optim_finalize  per tensor: its chunks' partials summed in chunk order; c = <G,W>/sigma,
//                           ||dW||^2 = (|G|^2 - 2c u^T G v + c^2 |u|^2 |v|^2)/sigma^2;
//                           total norm, clip coefficient = min(1, max_norm / (norm + 1e-6)), found_inf; the device
//                           step counter advances unless found_inf (torch's fused AdamW: steps -= found_inf)
//   pass 3  optim_update    g' = ((G - c u_i v_j)/sigma) * clip / grad_scale; AdamW exactly as torch.optim.AdamW:
//                           p *= 1 - lr*wd; m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2;
//                           p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps);   skipped entirely if found_inf
//           optim_update_groups  the same update with lr and wd of the tensor's parameter group (calm_optim_step_groups)
// Work item = chunk of CHUNK consecutive elements of one tensor (table built by the host).
//
// calm_optim_step_lamb: LAMB (You et al. 2020, as timm's `Lamb` decides which tensors adapt) over the same table in four
// launches.  lr_t, wd_t = the tensor's group's with a group table, hparams' (lr_dev) otherwise; all in fp32:
//   pass 1, 2  optim_stats, optim_finalize: the kernels above on the scratch layout above — the norm, the clip coefficient,
//                           found_inf and the step counter have calm_optim_step's bits
//   pass 3  lamb_moments    g' as pass 3 above; m = m + (g' - m)(1 - b1); v = v b2 + g'^2 (1 - b2), both stored;
//                           r = (m / (sqrt(v) * (1 / sqrt(1 - b2^t)) + eps)) / (1 - b1^t);  u = r + wd_t * w  (lamb_u: its
//                           three roundings are never contracted, so pass 4 forms the same bits); per chunk sum w^2 and
//                           sum u^2 — a thread adds its elements serially, then block_sum_256; w is not written
//   pass 4  lamb_apply      thread 0 of every workgroup adds its tensor's partials in chunk order (tensor_sn_c's scheme: no
//                           fifth launch, chunks^2 eight-byte loads per tensor); wn = sqrt(W2), un = sqrt(U2);
//                           trust = (adapt_t && wn > 0 && un > 0) ? wn / un : 1, adapt_t = always_adapt || wd_t != 0;
//                           trust_clip > 0: trust = min(trust, trust_clip); the tensor's first chunk stores (wn, un, trust);
//                           lr_t != 0: u = lamb_u(stored m, stored v, w), w = w - (lr_t * trust) * u
//   found_inf: passes 3 and 4 return at once — nothing is written, trust_out included.
// A chunk whose operand addresses (pass 3: grad, param, exp_avg, exp_avg_sq + i0; pass 4: the last three) are all 16-byte
// aligned moves as 16-byte vectors with a single-word tail (a thread's serial sums then run over its vectors' elements in
// address order), any other chunk as single words.  No atomics; every sum has a fixed order; no result depends on the grid.
#include "chunk_table.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = CHUNK_ELEMS;           // elements per work item (64 per thread)
constexpr int ST = 6;                        // per-tensor scratch: sum g^2, <G,W>, u^T G v, |u|^2, |v|^2, c
constexpr int CP = 3;                        // per-chunk partials: sum g^2, <G,W>, u^T G v

struct Globals { float total_sq, norm, clip, found_inf; };
// scratch layout: [ST x n_tensors][Globals][CP x n_chunks]

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e38f; }   // false for inf and NaN

__global__ __launch_bounds__(NT) void optim_stats(const calm_optim_tensor* __restrict__ T, const int* __restrict__ chunk_tensor,
                                                  float* __restrict__ stats, Globals* __restrict__ G,
                                                  float* __restrict__ chunk_part) {
    __shared__ float red[4];
    const int t = chunk_tensor[blockIdx.x];
    const calm_optim_tensor e = T[t];
    const auto [i0, i1] = chunk_span(blockIdx.x, CHUNK, e.chunk0, e.numel);
    float s2 = 0.f, gw = 0.f, guv = 0.f;
    bool bad = false;
    if (e.sn_sigma) {
        for (long i = i0 + threadIdx.x; i < i1; i += NT) {
            const float g = e.grad[i];
            // rows * cols < 2^31 for a spectral-norm layer (checked by the host): 32-bit division, not the 64-bit sequence
            const unsigned r = (unsigned)i / (unsigned)e.cols, c = (unsigned)i - r * (unsigned)e.cols;
            s2 += g * g; gw += g * e.param[i]; guv += g * e.sn_u[r] * e.sn_v[c];
            bad |= !finite_f(g);
        }
    } else {
        for (long i = i0 + threadIdx.x; i < i1; i += NT) {
            const float g = e.grad[i];
            s2 += g * g;
            bad |= !finite_f(g);
        }
    }
    s2 = block_sum_256(s2, red);
    if (threadIdx.x == 0) chunk_part[CP * blockIdx.x] = s2;
    if (e.sn_sigma) {
        gw = block_sum_256(gw, red);
        guv = block_sum_256(guv, red);
        if (threadIdx.x == 0) { chunk_part[CP * blockIdx.x + 1] = gw; chunk_part[CP * blockIdx.x + 2] = guv; }
        if (i0 == 0) {                         // the tensor's first chunk also measures u and v
            float uu = 0.f, vv = 0.f;
            for (int r = threadIdx.x; r < e.rows; r += NT) uu += e.sn_u[r] * e.sn_u[r];
            for (int c = threadIdx.x; c < e.cols; c += NT) vv += e.sn_v[c] * e.sn_v[c];
            uu = block_sum_256(uu, red);
            vv = block_sum_256(vv, red);
            if (threadIdx.x == 0) { stats[ST * t + 3] = uu; stats[ST * t + 4] = vv; }
        }
    }
    if (bad) G->found_inf = 1.f;              // benign race: every writer stores the same value
}

__global__ __launch_bounds__(NT) void optim_finalize(const calm_optim_tensor* __restrict__ T, int n, float* __restrict__ stats,
                                                     Globals* __restrict__ G, float max_norm, const float* __restrict__ grad_scale,
                                                     float* __restrict__ out, const float* __restrict__ chunk_part,
                                                     int* __restrict__ step_dev) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int t = threadIdx.x; t < n; t += NT) {
        const calm_optim_tensor e = T[t];
        const int nch = chunk_count(CHUNK, e.numel);
        float n2 = 0.f, gw = 0.f, guv = 0.f;
        for (int k = 0; k < nch; ++k) {                             // fixed order: chunk 0, 1, 2, ...
            const float* cp = chunk_part + (long)CP * (e.chunk0 + k);
            n2 += cp[0];
            if (e.sn_sigma) { gw += cp[1]; guv += cp[2]; }
        }
        if (e.sn_sigma) {
            const float uu = stats[ST * t + 3], vv = stats[ST * t + 4];
            const float sg = e.sn_sigma[0];
            const float c = gw / sg;                                // <G, W_orig / sigma>
            stats[ST * t + 5] = c;
            n2 = (n2 - 2.f * c * guv + c * c * uu * vv) / (sg * sg);
        }
        acc += fmaxf(n2, 0.f);
    }
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) {
        const float inv_scale = grad_scale ? 1.0f / grad_scale[0] : 1.0f;
        const float norm = sqrtf(acc) * inv_scale;
        const bool bad = G->found_inf != 0.f || !finite_f(norm);
        float clip = max_norm > 0.f ? fminf(1.0f, max_norm / (norm + 1e-6f)) : 1.0f;
        G->total_sq = acc;
        G->norm = norm;
        G->clip = clip * inv_scale;
        G->found_inf = bad ? 1.f : 0.f;
        out[0] = norm;
        out[1] = bad ? 1.f : 0.f;
        if (step_dev && !bad) step_dev[0] += 1;      // a skipped step does not advance the bias-correction count
    }
}

// The update of one chunk with the tensor's rate and weight decay: shared by both update kernels, so that equal
// hyper-parameters give equal bits whichever of them runs.
__device__ __forceinline__ void update_chunk(const calm_optim_tensor& e, int t, int chunk, const float* __restrict__ stats,
                                             const Globals* __restrict__ G, const calm_optim_hparams& hp, float lr, float wd) {
    const auto [i0, i1] = chunk_span(chunk, CHUNK, e.chunk0, e.numel);
    const float mul = G->clip;
    const float decay = 1.0f - lr * wd;
    const float bc1 = 1.0f - powf(hp.beta1, (float)hp.step), bc2 = 1.0f - powf(hp.beta2, (float)hp.step);
    const float step_size = lr / bc1, inv_sqrt_bc2 = 1.0f / sqrtf(bc2);
    const bool sn = e.sn_sigma != nullptr;
    const float c = sn ? stats[ST * t + 5] : 0.f, inv_sg = sn ? 1.0f / e.sn_sigma[0] : 1.f;
    for (long i = i0 + threadIdx.x; i < i1; i += NT) {
        float g = e.grad[i];
        if (sn) {
            const unsigned r = (unsigned)i / (unsigned)e.cols, cc = (unsigned)i - r * (unsigned)e.cols;
            g = (g - c * e.sn_u[r] * e.sn_v[cc]) * inv_sg;
        }
        g *= mul;
        float p = e.param[i] * decay;
        const float m = e.exp_avg[i] + (g - e.exp_avg[i]) * (1.0f - hp.beta1);          // lerp_
        const float v = e.exp_avg_sq[i] * hp.beta2 + g * g * (1.0f - hp.beta2);
        const float denom = sqrtf(v) * inv_sqrt_bc2 + hp.eps;
        p -= step_size * (m / denom);
        e.param[i] = p; e.exp_avg[i] = m; e.exp_avg_sq[i] = v;
    }
}

__global__ __launch_bounds__(NT) void optim_update(const calm_optim_tensor* __restrict__ T, const int* __restrict__ chunk_tensor,
                                                   const float* __restrict__ stats, const Globals* __restrict__ G,
                                                   calm_optim_hparams hp, const int* __restrict__ step_dev,
                                                   const float* __restrict__ lr_dev) {
    if (G->found_inf != 0.f) return;          // the reference's scaler.step() skips optimizer.step() on inf/NaN
    if (step_dev) hp.step = step_dev[0];      // already advanced by optim_finalize for this (un-skipped) step
    if (lr_dev) hp.lr = lr_dev[0];            // a captured step follows the LR schedule through this device scalar
    const int t = chunk_tensor[blockIdx.x];
    const calm_optim_tensor e = T[t];
    update_chunk(e, t, blockIdx.x, stats, G, hp, hp.lr, hp.weight_decay);
}

// Pass 3 with parameter groups: the rate and the weight decay are those of the tensor's group, read from the device
// table once per workgroup (the index is uniform: a scalar load); hp.lr and hp.weight_decay are not read.
__global__ __launch_bounds__(NT) void optim_update_groups(const calm_optim_tensor* __restrict__ T, const int* __restrict__ chunk_tensor,
                                                          const float* __restrict__ stats, const Globals* __restrict__ G,
                                                          calm_optim_hparams hp, const int* __restrict__ step_dev,
                                                          const calm_optim_group* __restrict__ groups) {
    if (G->found_inf != 0.f) return;
    if (step_dev) hp.step = step_dev[0];
    const int t = chunk_tensor[blockIdx.x];
    const calm_optim_tensor e = T[t];
    const calm_optim_group gr = groups[e.group];
    update_chunk(e, t, blockIdx.x, stats, G, hp, gr.lr, gr.weight_decay);
}

// ---- LAMB ---------------------------------------------------------------------------------------------------------------
constexpr int LP = 2;                        // per-chunk partials behind calm_optim_step's scratch: sum w^2, sum u^2
constexpr int LU3 = 2, LU4 = 4;              // 16-byte vectors a thread has in flight per operand (pass 3: four operands)

struct LambCoef { float b1c, b2, b2c, inv_sqrt_bc2, eps, bc1, wd; };

__device__ __forceinline__ LambCoef lamb_coef(float beta1, float beta2, float eps, int step, float wd) {
    const float bc1 = 1.0f - powf(beta1, (float)step), bc2 = 1.0f - powf(beta2, (float)step);   // update_chunk's
    return {1.0f - beta1, beta2, 1.0f - beta2, 1.0f / sqrtf(bc2), eps, bc1, wd};
}

// u of one element from the NEW moments and the OLD weight; passes 3 and 4 must agree to the bit: no contraction
__device__ __forceinline__ float lamb_u(const LambCoef& k, float m, float v, float w) {
#pragma clang fp contract(off)
    const float r = (m / (sqrtf(v) * k.inv_sqrt_bc2 + k.eps)) / k.bc1;
    const float d = k.wd * w;
    return r + d;
}

struct LambSums { float w2 = 0.f, u2 = 0.f; };

// pass 3 over one chunk [i0, i1) of tensor e
template <bool SN>
__device__ __forceinline__ LambSums lamb_moments_span(const calm_optim_tensor& e, long i0, long i1, const LambCoef& k, float c,
                                                      float inv_sg, float mul) {
    const gf32* g = (const gf32*)e.grad;
    const gf32* p = (const gf32*)e.param;
    gf32* ma = (gf32*)e.exp_avg;
    gf32* va = (gf32*)e.exp_avg_sq;
    const gf32* su = (const gf32*)e.sn_u;
    const gf32* sv = (const gf32*)e.sn_v;
    const unsigned cols = (unsigned)e.cols;
    LambSums a;
    const auto element = [&](float gi, float wi, float& mi, float& vi, unsigned r, unsigned cc) __attribute__((always_inline)) {
        if (SN) gi = (gi - c * su[r] * sv[cc]) * inv_sg;
        gi *= mul;
        mi = mi + (gi - mi) * k.b1c;                             // lerp_
        vi = vi * k.b2 + gi * gi * k.b2c;
        const float u = lamb_u(k, mi, vi, wi);
        a.w2 += wi * wi;
        a.u2 += u * u;
    };
    // the 32-bit row / column split of optim_update (rows * cols < 2^31, checked by the host)
    const auto scalar = [&](long b, long end) __attribute__((always_inline)) {
        for (long i = b + threadIdx.x; i < end; i += NT) {
            unsigned r = 0, cc = 0;
            if (SN) { r = (unsigned)i / cols; cc = (unsigned)i - r * cols; }
            float mi = ma[i], vi = va[i];
            element(g[i], p[i], mi, vi, r, cc);
            ma[i] = mi; va[i] = vi;
        }
    };
    if (dev_aligned16(g + i0) && dev_aligned16(p + i0) && dev_aligned16(ma + i0) && dev_aligned16(va + i0)) {
        const long v1 = i0 + ((i1 - i0) & ~3L);
        struct Quad { f32x4 g, w, m, v; };
        const auto load = [&](long i) __attribute__((always_inline)) {
            Quad q;
            q.g = *(const gf32x4*)(g + i); q.w = *(const gf32x4*)(p + i);
            q.m = *(const gf32x4*)(ma + i); q.v = *(const gf32x4*)(va + i);
            return q;
        };
        const auto store = [&](long i, const Quad& q) __attribute__((always_inline)) {
            unsigned r = 0, cc = 0;
            if (SN) { r = (unsigned)i / cols; cc = (unsigned)i - r * cols; }
            f32x4 m4 = q.m, v4 = q.v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float mi = m4[j], vi = v4[j];
                element(q.g[j], q.w[j], mi, vi, r, cc);
                m4[j] = mi; v4[j] = vi;
                if (SN && ++cc == cols) { cc = 0; ++r; }         // (cols = 1: every element starts a row)
            }
            *(gf32x4*)(ma + i) = m4;
            *(gf32x4*)(va + i) = v4;
        };
        loads_ahead_of_stores<LU3, 4, NT>(i0, v1, load, store);
        scalar(v1, i1);
    } else {
        scalar(i0, i1);
    }
    return a;
}

__global__ __launch_bounds__(NT) void lamb_moments(const calm_optim_tensor* __restrict__ T, const int* __restrict__ chunk_tensor,
                                                   const float* __restrict__ stats, const Globals* __restrict__ G,
                                                   const calm_optim_hparams hp, const int* __restrict__ step_dev,
                                                   const calm_optim_group* __restrict__ groups, float* __restrict__ lamb_part) {
    __shared__ float red[4];
    if (G->found_inf != 0.f) return;          // a skipped step writes nothing: not the moments, not the partials
    const int step = step_dev ? step_dev[0] : hp.step;     // already advanced by optim_finalize for this (un-skipped) step
    const int t = chunk_tensor[blockIdx.x];
    const calm_optim_tensor e = T[t];
    const auto [i0, i1] = chunk_span(blockIdx.x, CHUNK, e.chunk0, e.numel);
    const LambCoef k = lamb_coef(hp.beta1, hp.beta2, hp.eps, step, groups ? groups[e.group].weight_decay : hp.weight_decay);
    const float mul = G->clip;
    LambSums a;
    if (e.sn_sigma) {                         // (uniform over the workgroup)
        a = lamb_moments_span<true>(e, i0, i1, k, stats[ST * t + 5], 1.0f / e.sn_sigma[0], mul);
    } else {
        a = lamb_moments_span<false>(e, i0, i1, k, 0.f, 1.f, mul);
    }
    const float w2 = block_sum_256(a.w2, red);
    const float u2 = block_sum_256(a.u2, red);
    if (threadIdx.x == 0) { lamb_part[LP * blockIdx.x] = w2; lamb_part[LP * blockIdx.x + 1] = u2; }
}

__global__ __launch_bounds__(NT) void lamb_apply(const calm_optim_tensor* __restrict__ T, const int* __restrict__ chunk_tensor,
                                                 const Globals* __restrict__ G, const calm_optim_hparams hp,
                                                 const calm_lamb_hparams lhp,
                                                 const int* __restrict__ step_dev, const float* __restrict__ lr_dev,
                                                 const calm_optim_group* __restrict__ groups,
                                                 const float* __restrict__ lamb_part, float* __restrict__ trust_out) {
    __shared__ float trust_lds;
    if (G->found_inf != 0.f) return;
    const int step_no = step_dev ? step_dev[0] : hp.step;
    const int t = chunk_tensor[blockIdx.x];
    const calm_optim_tensor e = T[t];
    const auto [i0, i1] = chunk_span(blockIdx.x, CHUNK, e.chunk0, e.numel);
    float lr = hp.lr, wd = hp.weight_decay;
    if (lr_dev) lr = lr_dev[0];               // a captured step follows the LR schedule through this device scalar
    if (groups) { const calm_optim_group gr = groups[e.group]; lr = gr.lr; wd = gr.weight_decay; }
    const LambCoef k = lamb_coef(hp.beta1, hp.beta2, hp.eps, step_no, wd);
    if (threadIdx.x == 0) {
        const int nch = chunk_count(CHUNK, e.numel);
        float W2 = 0.f, U2 = 0.f;
        for (int c = 0; c < nch; ++c) {                          // fixed order: chunk 0, 1, 2, ...
            W2 += lamb_part[LP * (e.chunk0 + c)];
            U2 += lamb_part[LP * (e.chunk0 + c) + 1];
        }
        const float wn = sqrtf(W2), un = sqrtf(U2);
        const bool adapt = lhp.always_adapt != 0 || wd != 0.f;
        float trust = (adapt && wn > 0.f && un > 0.f) ? wn / un : 1.0f;
        if (lhp.trust_clip > 0.f) trust = fminf(trust, lhp.trust_clip);
        if (trust_out && i0 == 0) { trust_out[3 * t] = wn; trust_out[3 * t + 1] = un; trust_out[3 * t + 2] = trust; }
        trust_lds = trust;
    }
    __syncthreads();
    if (lr == 0.f) return;                    // a frozen tensor keeps its bits (its moments moved in pass 3)
    const float step = lr * trust_lds;
    gf32* p = (gf32*)e.param;
    const gf32* ma = (const gf32*)e.exp_avg;
    const gf32* va = (const gf32*)e.exp_avg_sq;
    const auto scalar = [&](long b, long end) __attribute__((always_inline)) {
        for (long i = b + threadIdx.x; i < end; i += NT) {
            const float wi = p[i];
            p[i] = wi - step * lamb_u(k, ma[i], va[i], wi);
        }
    };
    if (dev_aligned16(p + i0) && dev_aligned16(ma + i0) && dev_aligned16(va + i0)) {
        const long v1 = i0 + ((i1 - i0) & ~3L);
        struct Triple { f32x4 w, m, v; };
        const auto load = [&](long i) __attribute__((always_inline)) {
            Triple q;
            q.w = *(const gf32x4*)(p + i); q.m = *(const gf32x4*)(ma + i); q.v = *(const gf32x4*)(va + i);
            return q;
        };
        const auto store = [&](long i, const Triple& q) __attribute__((always_inline)) {
            f32x4 out;
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = q.w[j] - step * lamb_u(k, q.m[j], q.v[j], q.w[j]);
            *(gf32x4*)(p + i) = out;
        };
        loads_ahead_of_stores<LU4, 4, NT>(i0, v1, load, store);
        scalar(v1, i1);
    } else {
        scalar(i0, i1);
    }
}

// passes 1 and 2 of both entry points: scratch cleared, per-chunk partials, the norm / clip / found_inf / step count
int stats_and_finalize(const calm_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev, int32_t n_chunks,
                       float* scratch, float max_norm, const float* grad_scale, float* stats_out, int32_t* step_dev, void* stream) {
    const size_t scratch_bytes = sizeof(float) * ST * (size_t)n_tensors + sizeof(Globals);
    if (hipError_t e = hipMemsetAsync(scratch, 0, scratch_bytes, as_stream(stream))) return (int)e;
    Globals* G = reinterpret_cast<Globals*>(scratch + ST * (size_t)n_tensors);
    float* chunk_part = scratch + ST * (size_t)n_tensors + sizeof(Globals) / sizeof(float);     // every entry is written
    if (int e = calm_launch(optim_stats, n_chunks, NT, 0, stream, tensors_dev, chunk_tensor_dev, scratch, G, chunk_part))
        return e;
    return calm_launch(optim_finalize, 1, NT, 0, stream, tensors_dev, n_tensors, scratch, G, max_norm, grad_scale,
                       stats_out, chunk_part, step_dev);
}

bool bad_step_args(const void* tensors_dev, int32_t n_tensors, const void* chunk_tensor_dev, int32_t n_chunks, const void* scratch,
                   const calm_optim_hparams* hp, const void* stats_out, const void* step_dev) {
    if (!tensors_dev || !chunk_tensor_dev || !scratch || !hp || !stats_out || n_tensors <= 0 || n_chunks <= 0) return true;
    return (!step_dev && hp->step < 1) || hp->beta1 < 0.f || hp->beta1 >= 1.f || hp->beta2 < 0.f || hp->beta2 >= 1.f;
}

}  // namespace

extern "C" {

int32_t calm_optim_chunk_elems(void) { return CHUNK; }

int calm_optim_step(const calm_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev,
                    int32_t n_chunks, float* scratch, const calm_optim_hparams* hp, const float* grad_scale,
                    float* stats_out, int32_t* step_dev, const float* lr_dev, void* stream) {
    if (bad_step_args(tensors_dev, n_tensors, chunk_tensor_dev, n_chunks, scratch, hp, stats_out, step_dev) || hp->lr < 0.f)
        return CALM_E_INVAL;
    if (int e = stats_and_finalize(tensors_dev, n_tensors, chunk_tensor_dev, n_chunks, scratch, hp->max_norm, grad_scale,
                                   stats_out, step_dev, stream))
        return e;
    const Globals* G = reinterpret_cast<const Globals*>(scratch + ST * (size_t)n_tensors);
    return calm_launch(optim_update, n_chunks, NT, 0, stream, tensors_dev, chunk_tensor_dev, scratch, G, *hp, step_dev, lr_dev);
}

int calm_optim_step_groups(const calm_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev,
                           int32_t n_chunks, float* scratch, const calm_optim_hparams* hp, const calm_optim_group* groups_dev,
                           int32_t n_groups, const float* grad_scale, float* stats_out, int32_t* step_dev, void* stream) {
    if (bad_step_args(tensors_dev, n_tensors, chunk_tensor_dev, n_chunks, scratch, hp, stats_out, step_dev) || !groups_dev ||
        n_groups <= 0)
        return CALM_E_INVAL;
    if (int e = stats_and_finalize(tensors_dev, n_tensors, chunk_tensor_dev, n_chunks, scratch, hp->max_norm, grad_scale,
                                   stats_out, step_dev, stream))
        return e;
    const Globals* G = reinterpret_cast<const Globals*>(scratch + ST * (size_t)n_tensors);
    return calm_launch(optim_update_groups, n_chunks, NT, 0, stream, tensors_dev, chunk_tensor_dev, scratch, G, *hp, step_dev,
                       groups_dev);
}

int64_t calm_optim_lamb_scratch_floats(int32_t n_tensors, int32_t n_chunks) {
    if (n_tensors <= 0 || n_chunks <= 0) return CALM_E_INVAL;
    return ST * (int64_t)n_tensors + (int64_t)(sizeof(Globals) / sizeof(float)) + (CP + LP) * (int64_t)n_chunks;
}

int calm_optim_step_lamb(const calm_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev,
                         int32_t n_chunks, float* scratch, const calm_optim_hparams* hp, const calm_lamb_hparams* lhp,
                         const calm_optim_group* groups_dev, int32_t n_groups, const float* grad_scale, float* stats_out,
                         float* trust_out, int32_t* step_dev, const float* lr_dev, void* stream) {
    if (bad_step_args(tensors_dev, n_tensors, chunk_tensor_dev, n_chunks, scratch, hp, stats_out, step_dev) || !lhp)
        return CALM_E_INVAL;
    if (groups_dev ? n_groups <= 0 : hp->lr < 0.f) return CALM_E_INVAL;
    if (!(lhp->trust_clip >= 0.f) || (lhp->always_adapt != 0 && lhp->always_adapt != 1)) return CALM_E_INVAL;   // (NaN too)
    if (int e = stats_and_finalize(tensors_dev, n_tensors, chunk_tensor_dev, n_chunks, scratch, hp->max_norm, grad_scale,
                                   stats_out, step_dev, stream))
        return e;
    const Globals* G = reinterpret_cast<const Globals*>(scratch + ST * (size_t)n_tensors);
    float* lamb_part = scratch + ST * (size_t)n_tensors + sizeof(Globals) / sizeof(float) + CP * (size_t)n_chunks;
    if (int e = calm_launch(lamb_moments, n_chunks, NT, 0, stream, tensors_dev, chunk_tensor_dev, scratch, G, *hp, step_dev,
                            groups_dev, lamb_part))
        return e;
    return calm_launch(lamb_apply, n_chunks, NT, 0, stream, tensors_dev, chunk_tensor_dev, G, *hp, *lhp, step_dev,
                       groups_dev ? nullptr : lr_dev, groups_dev, lamb_part, trust_out);
}

}  // extern "C"
