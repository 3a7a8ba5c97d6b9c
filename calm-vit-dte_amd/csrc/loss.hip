// The loss end of the step: soft-target cross-entropy (distributed_trainer_cls.py:63,86), the token-layout Huber loss of
// the generative trainer (distributed_trainer_reg.py:59,78-81), binary cross-entropy with logits (the DeiT III / timm
// recipe's loss on the same soft targets) and the device-side step metrics (cls:98-102, CALM_ViT_V2.py:228-239).  Every
// cross-workgroup sum goes through the caller's `partials` and ONE final workgroup that adds them in a fixed order: no
// atomics, results repeat bit for bit.
#include <math.h>

#include "common.h"

#define LOSS_NT 256

// ---- block-wide helpers (256 threads = 4 waves; `red` is >= 8 floats of LDS) -------------------------------------------
// (value, index) maximum with ties going to the LOWEST index; NaN never wins a comparison, so it is never selected
__device__ __forceinline__ void argmax_merge(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        argmax_merge(v, i, ov, oi);
    }
}
__device__ __forceinline__ void block_argmax_256(float& v, int& i, float* red) {
    wave_argmax(v, i);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        red[w] = v;
        red[4 + w] = __int_as_float(i);
    }
    __syncthreads();
    v = red[0];
    i = __float_as_int(red[4]);
#pragma unroll
    for (int k = 1; k < 4; ++k) argmax_merge(v, i, red[k], __float_as_int(red[4 + k]));
}

// ---- soft-target cross-entropy -----------------------------------------------------------------------------------------
// One workgroup per row.  Pass 1: row maximum (with its index), the targets' maximum index, sum of the targets, NaN flag.
// Pass 2 (the row is 4 KB at C = 1000: it comes back from the cache): sum exp(z - max) and sum y (max - z).
//   row loss = sum_c y_c (max - z_c) + log(sum exp(z - max)) * sum_c y_c
// — both terms are sums of non-negative products for probability targets, nothing cancels (lse * sum y - sum y z would).
// c4: number of leading float4 groups of a row that may be read as 16-byte vectors (0: scalar path for the whole row).
static __global__ __launch_bounds__(LOSS_NT) void soft_ce_fwd_kernel(const float* __restrict__ logits, long ld,
                                                                     const float* __restrict__ targets, long td,
                                                                     float* __restrict__ row_stats,
                                                                     float* __restrict__ partials, int B, int C, int c4) {
    __shared__ float red[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* z = logits + (long)b * ld;
    const float* y = targets + (long)b * td;
    float zm = -INFINITY, ym = -INFINITY, ysum = 0.f;
    int zi = 0x7fffffff, yi = 0x7fffffff;
    bool bad = false;
    for (int q = tid; q < c4; q += LOSS_NT) {
        const f32x4 zv = *reinterpret_cast<const f32x4*>(z + 4 * q);
        const f32x4 yv = *reinterpret_cast<const f32x4*>(y + 4 * q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bad |= (zv[k] != zv[k]) | (yv[k] != yv[k]);
            if (zv[k] > zm) { zm = zv[k]; zi = 4 * q + k; }
            if (yv[k] > ym) { ym = yv[k]; yi = 4 * q + k; }
            ysum += yv[k];
        }
    }
    for (int c = 4 * c4 + tid; c < C; c += LOSS_NT) {
        const float zc = z[c], yc = y[c];
        bad |= (zc != zc) | (yc != yc);
        if (zc > zm) { zm = zc; zi = c; }
        if (yc > ym) { ym = yc; yi = c; }
        ysum += yc;
    }
    // a thread that saw only -inf (or nothing) still holds index INT_MAX: the merge prefers any real index at equal value
    if (zm == -INFINITY && zi == 0x7fffffff && tid < C) zi = tid;
    if (ym == -INFINITY && yi == 0x7fffffff && tid < C) yi = tid;
    block_argmax_256(zm, zi, red);
    block_argmax_256(ym, yi, red);
    ysum = block_sum_256(ysum, red);
    const float nbad = block_sum_256(bad ? 1.f : 0.f, red);

    float se = 0.f, yd = 0.f;
    for (int q = tid; q < c4; q += LOSS_NT) {
        const f32x4 zv = *reinterpret_cast<const f32x4*>(z + 4 * q);
        const f32x4 yv = *reinterpret_cast<const f32x4*>(y + 4 * q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            se += __expf(zv[k] - zm);
            yd = fmaf(yv[k], zm - zv[k], yd);
        }
    }
    for (int c = 4 * c4 + tid; c < C; c += LOSS_NT) {
        se += __expf(z[c] - zm);
        yd = fmaf(y[c], zm - z[c], yd);
    }
    se = block_sum_256(se, red);
    yd = block_sum_256(yd, red);
    if (tid == 0) {
        const float ls = logf(se);
        row_stats[2 * b] = zm;
        row_stats[2 * b + 1] = ls;
        partials[b] = fmaf(ls, ysum, yd);
        partials[B + b] = (nbad == 0.f && zi == yi) ? 1.f : 0.f;
    }
}

// The final pass of the losses: ONE workgroup adds n partials in a fixed order (thread t takes t, t + 256, ... in
// increasing index, then a fixed tree over the 256 running sums) and OVERWRITES the loss.  metrics (nullable) is the
// caller's float[4]; it is updated by one thread with a plain read-modify-write, ordered by the stream.  mscale: what
// turns the sum into B * loss for metrics[0] (1 for the cross-entropy, whose sum it is: s * 1.0f == s).
static __global__ __launch_bounds__(LOSS_NT) void loss_final_kernel(const float* __restrict__ part, int n, float scale,
                                                                    float* __restrict__ loss, const float* __restrict__ agree,
                                                                    float* __restrict__ metrics, int B, float mscale) {
    __shared__ float red[8];
    float s = 0.f, a = 0.f;
    for (int g = threadIdx.x; g < n; g += LOSS_NT) s += part[g];
    if (metrics)
        for (int g = threadIdx.x; g < B; g += LOSS_NT) a += agree[g];
    s = block_sum_256(s, red);
    a = block_sum_256(a, red);
    if (threadIdx.x == 0) {
        loss[0] = s * scale;
        if (metrics) {
            metrics[0] += s * mscale;
            metrics[1] += a;
            metrics[2] += (float)B;
            metrics[3] += 1.f;
        }
    }
}

// dlogits = dloss / B * (exp((z - max) - logsum) * sum_c y - y): one workgroup per row, sum_c y rebuilt in a fixed order
static __global__ __launch_bounds__(LOSS_NT) void soft_ce_bwd_kernel(const float* __restrict__ logits, long ld,
                                                                     const float* __restrict__ targets, long td,
                                                                     const float* __restrict__ row_stats,
                                                                     const float* __restrict__ dloss,
                                                                     float* __restrict__ dlogits, int B, int C, int c4) {
    __shared__ float red[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* z = logits + (long)b * ld;
    const float* y = targets + (long)b * td;
    float* dz = dlogits + (long)b * C;
    float ysum = 0.f;
    for (int q = tid; q < c4; q += LOSS_NT) {
        const f32x4 yv = *reinterpret_cast<const f32x4*>(y + 4 * q);
        ysum += (yv[0] + yv[1]) + (yv[2] + yv[3]);
    }
    for (int c = 4 * c4 + tid; c < C; c += LOSS_NT) ysum += y[c];
    ysum = block_sum_256(ysum, red);
    const float zm = row_stats[2 * b], ls = row_stats[2 * b + 1];
    const float g = dloss[0] / (float)B;
    for (int q = tid; q < c4; q += LOSS_NT) {
        const f32x4 zv = *reinterpret_cast<const f32x4*>(z + 4 * q);
        const f32x4 yv = *reinterpret_cast<const f32x4*>(y + 4 * q);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = g * fmaf(__expf((zv[k] - zm) - ls), ysum, -yv[k]);
        *reinterpret_cast<f32x4*>(dz + 4 * q) = o;
    }
    for (int c = 4 * c4 + tid; c < C; c += LOSS_NT) dz[c] = g * fmaf(__expf((z[c] - zm) - ls), ysum, -y[c]);
}

// ---- binary cross-entropy with logits ----------------------------------------------------------------------------------
// Every class is its own two-way problem: l(z, t) = max(z, 0) - z t + log(1 + exp(-|z|)), evaluated as
//   |z| * (z >= 0 ? 1 - t : t) + log1p(exp(-|z|))
// — exp never sees a positive argument, and for t in [0, 1] both terms are non-negative, so nothing cancels
// (max(z, 0) - z t does at z >> 0, t -> 1).  t is the target, or (y > threshold) with CALM_BCE_THRESHOLD.
__device__ __forceinline__ float bce_target(float y, bool thresholded, float threshold) {
    return thresholded ? (y > threshold ? 1.f : 0.f) : y;
}
__device__ __forceinline__ float bce_term(float z, float t) {
    const float a = fabsf(z);
    return fmaf(a, z >= 0.f ? 1.f - t : t, log1pf(__expf(-a)));
}
// sigmoid(z) - t with the two-branch sigmoid (one exponential of -|z|); z - z is 0 for a finite logit and NaN for an
// infinite one, whose loss is not finite either: the gradient says so and the scaled optimizer step is skipped
__device__ __forceinline__ float bce_slope(float z, float t) {
    const float e = __expf(-fabsf(z));
    const float s = (z >= 0.f ? 1.f : e) / (1.f + e);
    return (s - t) + (z - z);
}

// One workgroup per row, ONE pass: the row's loss sum, the maxima of z and of the ORIGINAL y with their lowest indices,
// the NaN flag.  c4 as in soft_ce_fwd_kernel.
static __global__ __launch_bounds__(LOSS_NT) void bce_fwd_kernel(const float* __restrict__ logits, long ld,
                                                                 const float* __restrict__ targets, long td,
                                                                 int thresholded, float threshold,
                                                                 float* __restrict__ partials, int B, int C, int c4) {
    __shared__ float red[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* z = logits + (long)b * ld;
    const float* y = targets + (long)b * td;
    float zm = -INFINITY, ym = -INFINITY, acc = 0.f;
    int zi = 0x7fffffff, yi = 0x7fffffff;
    bool bad = false;
    for (int q = tid; q < c4; q += LOSS_NT) {
        const f32x4 zv = *reinterpret_cast<const f32x4*>(z + 4 * q);
        const f32x4 yv = *reinterpret_cast<const f32x4*>(y + 4 * q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bad |= (zv[k] != zv[k]) | (yv[k] != yv[k]);
            if (zv[k] > zm) { zm = zv[k]; zi = 4 * q + k; }
            if (yv[k] > ym) { ym = yv[k]; yi = 4 * q + k; }
            acc += bce_term(zv[k], bce_target(yv[k], thresholded, threshold));
        }
    }
    for (int c = 4 * c4 + tid; c < C; c += LOSS_NT) {
        const float zc = z[c], yc = y[c];
        bad |= (zc != zc) | (yc != yc);
        if (zc > zm) { zm = zc; zi = c; }
        if (yc > ym) { ym = yc; yi = c; }
        acc += bce_term(zc, bce_target(yc, thresholded, threshold));
    }
    // (as soft_ce_fwd_kernel: a thread that saw only -inf, or nothing, must not win with index INT_MAX)
    if (zm == -INFINITY && zi == 0x7fffffff && tid < C) zi = tid;
    if (ym == -INFINITY && yi == 0x7fffffff && tid < C) yi = tid;
    block_argmax_256(zm, zi, red);
    block_argmax_256(ym, yi, red);
    acc = block_sum_256(acc, red);
    const float nbad = block_sum_256(bad ? 1.f : 0.f, red);
    if (tid == 0) {
        partials[b] = acc;
        partials[B + b] = (nbad == 0.f && zi == yi) ? 1.f : 0.f;
    }
}

// dlogits = dloss / denom * (sigmoid(z) - t), denom = B C or B: one workgroup per row, nothing saved, nothing summed
static __global__ __launch_bounds__(LOSS_NT) void bce_bwd_kernel(const float* __restrict__ logits, long ld,
                                                                 const float* __restrict__ targets, long td,
                                                                 int thresholded, float threshold, float denom,
                                                                 const float* __restrict__ dloss,
                                                                 float* __restrict__ dlogits, int C, int c4) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* z = logits + (long)b * ld;
    const float* y = targets + (long)b * td;
    float* dz = dlogits + (long)b * C;
    const float g = dloss[0] / denom;
    for (int q = tid; q < c4; q += LOSS_NT) {
        const f32x4 zv = *reinterpret_cast<const f32x4*>(z + 4 * q);
        const f32x4 yv = *reinterpret_cast<const f32x4*>(y + 4 * q);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = g * bce_slope(zv[k], bce_target(yv[k], thresholded, threshold));
        *reinterpret_cast<f32x4*>(dz + 4 * q) = o;
    }
    for (int c = 4 * c4 + tid; c < C; c += LOSS_NT) dz[c] = g * bce_slope(z[c], bce_target(y[c], thresholded, threshold));
}

// ---- top-1 count against integer labels --------------------------------------------------------------------------------
// ONE workgroup of 16 waves, a wave per row in turn (the eval loop's metric: B x C floats through one CU); the count is
// combined through LDS and added to the caller's metrics by one thread.
#define TOP1_NT 1024
static __global__ __launch_bounds__(TOP1_NT) void top1_count_kernel(const float* __restrict__ logits, long ld,
                                                                    const long long* __restrict__ labels,
                                                                    float* __restrict__ metrics, int B, int C, int c4) {
    __shared__ float cnt[TOP1_NT / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float hits = 0.f;
    for (int b = w; b < B; b += TOP1_NT / 64) {
        const float* z = logits + (long)b * ld;
        float zm = -INFINITY;
        int zi = 0x7fffffff;
        bool bad = false;
        for (int q = lane; q < c4; q += 64) {
            const f32x4 zv = *reinterpret_cast<const f32x4*>(z + 4 * q);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bad |= zv[k] != zv[k];
                if (zv[k] > zm) { zm = zv[k]; zi = 4 * q + k; }
            }
        }
        for (int c = 4 * c4 + lane; c < C; c += 64) {
            const float zc = z[c];
            bad |= zc != zc;
            if (zc > zm) { zm = zc; zi = c; }
        }
        if (zm == -INFINITY && zi == 0x7fffffff && lane < C) zi = lane;
        wave_argmax(zm, zi);
        const bool any_bad = __any(bad);
        if (!any_bad && (long long)zi == labels[b]) hits += 1.f;      // (every lane holds the same row result)
    }
    if (lane == 0) cnt[w] = hits;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < TOP1_NT / 64; ++k) t += cnt[k];
        metrics[1] += t;
        metrics[2] += (float)B;
    }
}

// ---- validation metrics: top-k, cross-entropy, per-class counts --------------------------------------------------------
// Launch 1, eval_rows_kernel: one wave per row, four rows per workgroup, ceil(B / 4) workgroups (top1_count_kernel above
// sends everything through one CU).  Pass 1: row maximum with its lowest index and the NaN flag; pass 2 (the row comes
// back from the cache): sum exp(z - max) and the number of classes that BEAT the label — z_c > z_l, or z_c == z_l and
// c < l — so the label is in the top k exactly when beaten < k.  One 16-byte record per row, written by lane 0.
// Launch 2, eval_fold_kernel: one workgroup folds the records into the caller's accumulators; every counter has one
// owning thread and the loss is added in a fixed order.
#define EVAL_SKIPPED 1       // record flags: the label is outside [0, C)
#define EVAL_NONFINITE 2     //               the row holds a NaN
#define EVAL_FOLD_NT 1024    // threads of the fold = rows per staged chunk = stride between the classes a thread owns
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
struct EvalKs { int k[4]; int nk; };

__device__ __forceinline__ float bf16_bits_to_float(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
// the logits of one row in storage type T (float, or the bits of a bf16): element c, or group q of VEC elements
template <bool BF16> struct EvalRow;
template <> struct EvalRow<false> {
    static constexpr int VEC = 4;
    const float* z;
    __device__ __forceinline__ float at(int c) const { return z[c]; }
    __device__ __forceinline__ void group(int q, float* v) const {
        const f32x4 t = *reinterpret_cast<const f32x4*>(z + 4 * q);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = t[k];
    }
};
template <> struct EvalRow<true> {
    static constexpr int VEC = 8;
    const unsigned short* z;
    __device__ __forceinline__ float at(int c) const { return bf16_bits_to_float(z[c]); }
    __device__ __forceinline__ void group(int q, float* v) const {
        const u16x8 t = *reinterpret_cast<const u16x8*>(z + 8 * q);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = bf16_bits_to_float(t[k]);
    }
};

// cv: number of leading VEC-element groups of a row that may be read as 16-byte vectors (0: scalar path for the whole row)
template <bool BF16>
static __global__ __launch_bounds__(LOSS_NT) void eval_rows_kernel(const void* __restrict__ logits, long ld,
                                                                   const long long* __restrict__ labels,
                                                                   float* __restrict__ partials, int B, int C, int cv) {
    using Row = EvalRow<BF16>;
    constexpr int VEC = Row::VEC;
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (LOSS_NT / 64) + (threadIdx.x >> 6);
    if (b >= B) return;                                              // (whole waves leave; nothing below is block-wide)
    const long long lab = labels[b];
    i32x4 rec = {0, 0, 0, EVAL_SKIPPED};
    if (lab >= 0 && lab < C) {
        const int l = (int)lab;
        Row row{reinterpret_cast<decltype(Row::z)>(logits) + (long)b * ld};
        const float zl = row.at(l);
        float zm = -INFINITY;
        int zi = 0x7fffffff;
        bool bad = false;
        float v[VEC];
        for (int q = lane; q < cv; q += 64) {
            row.group(q, v);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                bad |= v[k] != v[k];
                if (v[k] > zm) { zm = v[k]; zi = VEC * q + k; }
            }
        }
        for (int c = VEC * cv + lane; c < C; c += 64) {
            const float zc = row.at(c);
            bad |= zc != zc;
            if (zc > zm) { zm = zc; zi = c; }
        }
        if (zm == -INFINITY && zi == 0x7fffffff && lane < C) zi = lane;     // (as top1_count_kernel: an all -inf row -> 0)
        wave_argmax(zm, zi);
        const bool any_bad = __any(bad);

        float se = 0.f;
        int beaten = 0;
        for (int q = lane; q < cv; q += 64) {
            row.group(q, v);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                se += __expf(v[k] - zm);
                beaten += (v[k] > zl) | ((v[k] == zl) & (VEC * q + k < l));
            }
        }
        for (int c = VEC * cv + lane; c < C; c += 64) {
            const float zc = row.at(c);
            se += __expf(zc - zm);
            beaten += (zc > zl) | ((zc == zl) & (c < l));
        }
        se = wave_sum(se);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) beaten += __shfl_xor(beaten, o, 64);
        const float nll = (zm - zl) + logf(se);
        rec = i32x4{__float_as_int(nll), beaten, zi, any_bad ? EVAL_NONFINITE : 0};
    }
    if (lane == 0) *reinterpret_cast<i32x4*>(partials + 4 * (long)b) = rec;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Rows are staged EVAL_FOLD_NT at a time: thread t reads record and label of row r0 + t, keeps the scalar tallies and its
// share of the loss (rows t, t + 1024, ... in increasing order; a fixed tree over the 1024 running sums at the end), and
// leaves (label, or -1 when the row is not counted), (label where the prediction equals it, or -1) and (pred, or -1 when
// the row is not finite) in LDS.  Thread t then owns classes t, t + 1024, ...: it scans the staged rows once per owned
// class and adds what it found to that class's support, top-1 hits and confusion row with plain read-modify-writes — no
// other thread touches those addresses.
static __global__ __launch_bounds__(EVAL_FOLD_NT) void eval_fold_kernel(const float* __restrict__ partials,
                                                                        const long long* __restrict__ labels,
                                                                        long long* __restrict__ counts,
                                                                        double* __restrict__ loss_sum,
                                                                        long long* __restrict__ confusion, int B, int C,
                                                                        const EvalKs ks) {
    __shared__ i32x4 key_v[EVAL_FOLD_NT / 4];                        // (read back sixteen rows at a time)
    __shared__ i32x4 hit_v[EVAL_FOLD_NT / 4];
    __shared__ int pred_s[EVAL_FOLD_NT];
    int* key_s = reinterpret_cast<int*>(key_v);
    int* hit_s = reinterpret_cast<int*>(hit_v);
    __shared__ float redf[EVAL_FOLD_NT / 64];
    __shared__ int redi[7][EVAL_FOLD_NT / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    float s = 0.f;
    int tally[7] = {0, 0, 0, 0, 0, 0, 0};                            // rows, skipped, nonfinite, hits@ks[0..3]
    for (int r0 = 0; r0 < B; r0 += EVAL_FOLD_NT) {
        const int n = B - r0 < EVAL_FOLD_NT ? B - r0 : EVAL_FOLD_NT;
        int key = -1, pred = -1;
        if (t < n) {
            const i32x4 rec = *reinterpret_cast<const i32x4*>(partials + 4 * (long)(r0 + t));
            if (rec[3] & EVAL_SKIPPED) {
                tally[1] += 1;
            } else {
                tally[0] += 1;
                key = (int)labels[r0 + t];
                if (rec[3] & EVAL_NONFINITE) {
                    tally[2] += 1;
                } else {
                    pred = rec[2];
                    s += __int_as_float(rec[0]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) tally[3 + i] += (i < ks.nk) & (rec[1] < ks.k[i]);
                }
            }
        }
        key_s[t] = key;
        hit_s[t] = pred == key ? key : -1;                           // (the label where the row is a top-1 hit)
        pred_s[t] = pred;
        __syncthreads();
        // Every thread reads the same addresses (LDS broadcasts), sixteen rows per turn, and the counting does not branch.
        // This loop is the launch: ONE CU runs C x n compares twice (label, hit), ~100 instructions per wave and turn —
        // 14 us of a 17 us call at B = 256, C = 1000 (rocprofv3; the row kernel takes 4.6).  A wave holds 64 classes, so
        // SOME lane matches in most groups of sixteen rows: a row-by-row walk of every group with a match (two dependent
        // LDS reads and a branch per row) took 21 us.  Only the confusion matrix needs the rows one by one, and it reads
        // LDS again only for a row that matches.
        const int n16 = (n + 15) & ~15;                               // (keys behind row n are -1)
        for (int c = t; c < C; c += EVAL_FOLD_NT) {
            int sup = 0, h1 = 0;
            for (int r = 0; r < n16; r += 16) {
                i32x4 k[4];
                int m = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    k[j] = key_v[(r >> 2) + j];
                    const i32x4 h = hit_v[(r >> 2) + j];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        m += k[j][e] == c;
                        h1 += h[e] == c;
                    }
                }
                sup += m;
                if (confusion && m) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if (k[j][e] != c) continue;
                            const int p = pred_s[r + 4 * j + e];
                            if ((unsigned)p < (unsigned)C) confusion[(long)c * C + p] += 1;      // (-1: not finite)
                        }
                    }
                }
            }
            if (sup) counts[7 + c] += sup;
            if (h1) counts[7 + (long)C + c] += h1;
        }
        __syncthreads();
    }
    s = wave_sum(s);
#pragma unroll
    for (int i = 0; i < 7; ++i) tally[i] = wave_sum_int(tally[i]);
    if (lane == 0) {
        redf[w] = s;
#pragma unroll
        for (int i = 0; i < 7; ++i) redi[i][w] = tally[i];
    }
    __syncthreads();
    if (t == 0) {
        float total = 0.f;
#pragma unroll
        for (int k = 0; k < EVAL_FOLD_NT / 64; ++k) total += redf[k];
        loss_sum[0] += (double)total;
    }
    if (t >= 64 && t < 64 + 3 + ks.nk) {                             // (one owner per scalar counter, off thread 0's wave)
        const int i = t - 64;
        long long total = 0;
#pragma unroll
        for (int k = 0; k < EVAL_FOLD_NT / 64; ++k) total += redi[i][k];
        counts[i] += total;
    }
}

// ---- knowledge distillation: cross-entropy + KL / hard-label term ------------------------------------------------------
// One workgroup per row; thread t owns the 8-element groups t, t + 256, ... of the row in all three inputs.  Up to
// DISTILL_CACHED_C classes that is ONE group per thread, loaded once and kept in registers (24 values) through the three
// passes of the forward, so every input is read from memory once; longer rows are read again per pass (12 bytes per class
// and row: they come back from the cache).  Each pass ends in one block-wide combine through its own LDS slots (one
// barrier per pass).  The launches are bound by latency, not bandwidth: 3 MB at B = 256, C = 1000.
//   pass 1: max / argmax of z, t and y (ties to the lowest index), sum y, NaN flags
//   pass 2: sum exp(z - zm), sum exp((z - zm) / T), sum exp((t - tm) / T), sum y (zm - z)
//   pass 3 (soft): sum q (log q - log pT) with log q = (t - tm) / T - lsq, log pT = (z - zm) / T - lsT, q = exp(log q)
#define DISTILL_CACHED_C (8 * LOSS_NT)
struct DistillArgs {
    const float* logits;
    const void* teacher;
    const float* targets;
    long ld, tld, td;
    float inv_t, alpha, w, gw;   // 1 / T;  alpha;  the distillation term's weight in the loss: alpha T^2 (soft) or alpha
                                 // (hard); in the gradient: alpha T or alpha
    int mode, B, C;
    int zvec, tvec, yvec;        // whether the rows of each input may be read as 16-byte vectors
};

// n <= 8 elements from c0 on of an fp32 row / a teacher row in its storage type (elements behind n are 0 and not used)
__device__ __forceinline__ void distill_load8(const float* row, int c0, int n, bool vec, float* v) {
    if (vec && n == 8) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(row + c0);
        const f32x4 b = *reinterpret_cast<const f32x4*>(row + c0 + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = a[k]; v[4 + k] = b[k]; }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = k < n ? row[c0 + k] : 0.f;
    }
}
template <bool BF16>
__device__ __forceinline__ void distill_load8_teacher(const void* row, int c0, int n, bool vec, float* v) {
    if constexpr (BF16) {
        const unsigned short* r = reinterpret_cast<const unsigned short*>(row);
        if (vec && n == 8) {
            const u16x8 a = *reinterpret_cast<const u16x8*>(r + c0);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = bf16_bits_to_float(a[k]);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = k < n ? bf16_bits_to_float(r[c0 + k]) : 0.f;
        }
    } else {
        distill_load8(reinterpret_cast<const float*>(row), c0, n, vec, v);
    }
}

// body(c0, n, z, t, y) for every group this thread owns, in increasing c0
template <bool CACHED, bool BF16, class Body>
__device__ __forceinline__ void distill_groups(const DistillArgs& a, const float* z, const void* t, const float* y,
                                               const float* zc, const float* tc, const float* yc, int nc, Body&& body) {
    if constexpr (CACHED) {
        if (nc > 0) body(8 * (int)threadIdx.x, nc, zc, tc, yc);
    } else {
        const int groups = (a.C + 7) >> 3;
        for (int q = threadIdx.x; q < groups; q += LOSS_NT) {
            const int c0 = 8 * q, n = a.C - c0 < 8 ? a.C - c0 : 8;
            float z8[8], t8[8], y8[8];
            distill_load8(z, c0, n, a.zvec, z8);
            distill_load8_teacher<BF16>(t, c0, n, a.tvec, t8);
            distill_load8(y, c0, n, a.yvec, y8);
            body(c0, n, z8, t8, y8);
        }
    }
}

template <bool CACHED, bool BF16>
static __global__ __launch_bounds__(LOSS_NT) void distill_fwd_kernel(const DistillArgs a, float* __restrict__ row_stats,
                                                                     float* __restrict__ partials) {
    __shared__ float red1[4][8], red2[4][4], red3[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int B = a.B, C = a.C;
    const float* z = a.logits + (long)b * a.ld;
    const float* y = a.targets + (long)b * a.td;
    const void* t = BF16 ? static_cast<const void*>(reinterpret_cast<const unsigned short*>(a.teacher) + (long)b * a.tld)
                         : static_cast<const void*>(reinterpret_cast<const float*>(a.teacher) + (long)b * a.tld);
    float zc[8], tc[8], yc[8];
    int nc = 0;
    if (CACHED && 8 * tid < C) {
        nc = C - 8 * tid < 8 ? C - 8 * tid : 8;
        distill_load8(z, 8 * tid, nc, a.zvec, zc);
        distill_load8_teacher<BF16>(t, 8 * tid, nc, a.tvec, tc);
        distill_load8(y, 8 * tid, nc, a.yvec, yc);
    }

    // pass 1
    float zm = -INFINITY, tm = -INFINITY, ym = -INFINITY, ysum = 0.f;
    int zi = 0x7fffffff, ti = 0x7fffffff, yi = 0x7fffffff;
    bool bad_z = false, bad_t = false, bad_y = false;
    distill_groups<CACHED, BF16>(a, z, t, y, zc, tc, yc, nc, [&](int c0, int n, const float* zv, const float* tv, const float* yv) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < n) {
                bad_z |= zv[k] != zv[k];
                bad_t |= tv[k] != tv[k];
                bad_y |= yv[k] != yv[k];
                if (zv[k] > zm) { zm = zv[k]; zi = c0 + k; }
                if (tv[k] > tm) { tm = tv[k]; ti = c0 + k; }
                if (yv[k] > ym) { ym = yv[k]; yi = c0 + k; }
                ysum += yv[k];
            }
        }
    });
    // a thread that saw only -inf (or nothing) still holds index INT_MAX: the merge prefers any real index at equal value
    if (8 * tid < C) {
        if (zm == -INFINITY && zi == 0x7fffffff) zi = 8 * tid;
        if (tm == -INFINITY && ti == 0x7fffffff) ti = 8 * tid;
        if (ym == -INFINITY && yi == 0x7fffffff) yi = 8 * tid;
    }
    wave_argmax(zm, zi);
    wave_argmax(tm, ti);
    wave_argmax(ym, yi);
    ysum = wave_sum(ysum);
    const int bad = (__any(bad_z) ? 1 : 0) | (__any(bad_t) ? 2 : 0) | (__any(bad_y) ? 4 : 0);
    if (lane == 0) {
        red1[w][0] = zm; red1[w][1] = __int_as_float(zi);
        red1[w][2] = tm; red1[w][3] = __int_as_float(ti);
        red1[w][4] = ym; red1[w][5] = __int_as_float(yi);
        red1[w][6] = ysum; red1[w][7] = __int_as_float(bad);
    }
    __syncthreads();
    zm = red1[0][0]; zi = __float_as_int(red1[0][1]);
    tm = red1[0][2]; ti = __float_as_int(red1[0][3]);
    ym = red1[0][4]; yi = __float_as_int(red1[0][5]);
    int any_bad = __float_as_int(red1[0][7]);
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        argmax_merge(zm, zi, red1[k][0], __float_as_int(red1[k][1]));
        argmax_merge(tm, ti, red1[k][2], __float_as_int(red1[k][3]));
        argmax_merge(ym, yi, red1[k][4], __float_as_int(red1[k][5]));
        any_bad |= __float_as_int(red1[k][7]);
    }
    ysum = (red1[0][6] + red1[1][6]) + (red1[2][6] + red1[3][6]);

    // pass 2
    const float inv_t = a.inv_t;
    float se1 = 0.f, set = 0.f, seq = 0.f, yd = 0.f;
    distill_groups<CACHED, BF16>(a, z, t, y, zc, tc, yc, nc, [&](int, int n, const float* zv, const float* tv, const float* yv) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < n) {
                const float dz = zv[k] - zm;
                se1 += __expf(dz);
                set += __expf(dz * inv_t);
                seq += __expf((tv[k] - tm) * inv_t);
                yd = fmaf(yv[k], -dz, yd);
            }
        }
    });
    se1 = wave_sum(se1);
    set = wave_sum(set);
    seq = wave_sum(seq);
    yd = wave_sum(yd);
    if (lane == 0) { red2[w][0] = se1; red2[w][1] = set; red2[w][2] = seq; red2[w][3] = yd; }
    __syncthreads();
    const float ls1 = logf((red2[0][0] + red2[1][0]) + (red2[2][0] + red2[3][0]));
    const float lst = logf((red2[0][1] + red2[1][1]) + (red2[2][1] + red2[3][1]));
    const float lsq = logf((red2[0][2] + red2[1][2]) + (red2[2][2] + red2[3][2]));
    yd = (red2[0][3] + red2[1][3]) + (red2[2][3] + red2[3][3]);

    // pass 3
    float d;
    if (a.mode == CALM_DISTILL_SOFT) {
        float acc = 0.f;
        distill_groups<CACHED, BF16>(a, z, t, y, zc, tc, yc, nc, [&](int, int n, const float* zv, const float* tv, const float*) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k < n) {
                    const float lq = (tv[k] - tm) * inv_t - lsq;
                    const float lp = (zv[k] - zm) * inv_t - lst;
                    const float q = __expf(lq);
                    acc += q == 0.f ? 0.f : q * (lq - lp);           // (a NaN is not 0: it goes on)
                }
            }
        });
        acc = wave_sum(acc);
        if (lane == 0) red3[w] = acc;
        __syncthreads();
        d = (red3[0] + red3[1]) + (red3[2] + red3[3]);
    } else {
        d = (zm - z[ti < C ? ti : 0]) + ls1;                         // -log p1_k (every thread reads the one address)
        if (any_bad & 2) d = NAN;                                    // the argmax skipped a NaN: hand it on
    }
    if (tid == 0) {
        const float ce = fmaf(ls1, ysum, yd);
        float* rs = row_stats + (long)b * CALM_DISTILL_ROW_STATS;
        rs[0] = zm; rs[1] = ls1; rs[2] = lst; rs[3] = tm; rs[4] = lsq; rs[5] = (float)ti; rs[6] = ysum;
        rs[7] = (a.mode == CALM_DISTILL_HARD && (any_bad & 2)) ? NAN : 0.f;      // (the backward adds it: NaN loss, NaN gradient)
        partials[b] = (1.f - a.alpha) * ce + a.w * d;
        partials[B + b] = ce;
        partials[2 * B + b] = d;
        partials[3 * B + b] = (!(any_bad & 5) && zi == yi) ? 1.f : 0.f;
        partials[4 * B + b] = (!(any_bad & 3) && zi == ti) ? 1.f : 0.f;
    }
}

// ONE workgroup adds the five per-row values in a fixed order (thread t takes rows t, t + 256, ... in increasing index,
// then a fixed tree over the 256 running sums), overwrites the loss and updates the two metric buffers
static __global__ __launch_bounds__(LOSS_NT) void distill_final_kernel(const float* __restrict__ part, int B,
                                                                       float* __restrict__ loss, float* __restrict__ metrics,
                                                                       float* __restrict__ dmetrics) {
    __shared__ float red[8];
    float s[DISTILL_PART_ROWS];
#pragma unroll
    for (int k = 0; k < DISTILL_PART_ROWS; ++k) {
        float v = 0.f;
        for (int g = threadIdx.x; g < B; g += LOSS_NT) v += part[(long)k * B + g];
        s[k] = block_sum_256(v, red);
    }
    if (threadIdx.x == 0) {
        loss[0] = s[0] / (float)B;
        if (metrics) {
            metrics[0] += s[0];
            metrics[1] += s[3];
            metrics[2] += (float)B;
            metrics[3] += 1.f;
        }
        if (dmetrics) {
            dmetrics[0] += s[1];
            dmetrics[1] += s[2];
            dmetrics[2] += s[4];
            dmetrics[3] += (float)B;
        }
    }
}

// One workgroup per row, every input read once, nothing summed: all the row quantities are in row_stats.
template <bool BF16>
static __global__ __launch_bounds__(LOSS_NT) void distill_bwd_kernel(const DistillArgs a, const float* __restrict__ row_stats,
                                                                     const float* __restrict__ dloss,
                                                                     float* __restrict__ dlogits, int dvec) {
    const int b = blockIdx.x, C = a.C;
    const float* z = a.logits + (long)b * a.ld;
    const float* y = a.targets + (long)b * a.td;
    const void* t = BF16 ? static_cast<const void*>(reinterpret_cast<const unsigned short*>(a.teacher) + (long)b * a.tld)
                         : static_cast<const void*>(reinterpret_cast<const float*>(a.teacher) + (long)b * a.tld);
    float* dz = dlogits + (long)b * C;
    const float* rs = row_stats + (long)b * CALM_DISTILL_ROW_STATS;
    const float zm = rs[0], ls1 = rs[1], lst = rs[2], tm = rs[3], lsq = rs[4], ysum = rs[6], poison = rs[7];
    const int kt = (int)rs[5];
    const float g = dloss[0] / (float)a.B;
    const float inv_t = a.inv_t, ce_w = 1.f - a.alpha;
    const bool soft = a.mode == CALM_DISTILL_SOFT;
    const float kd_w = a.gw;
    const int groups = (C + 7) >> 3;
    for (int q = threadIdx.x; q < groups; q += LOSS_NT) {
        const int c0 = 8 * q, n = C - c0 < 8 ? C - c0 : 8;
        float zv[8], tv[8] = {}, yv[8], o[8];
        distill_load8(z, c0, n, a.zvec, zv);
        distill_load8(y, c0, n, a.yvec, yv);
        if (soft) distill_load8_teacher<BF16>(t, c0, n, a.tvec, tv);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float dzk = zv[k] - zm;
            const float p1 = __expf(dzk - ls1);
            float kd;
            if (soft) kd = __expf(dzk * inv_t - lst) - __expf((tv[k] - tm) * inv_t - lsq);
            else kd = (p1 - (c0 + k == kt ? 1.f : 0.f)) + poison;
            o[k] = g * fmaf(ce_w, fmaf(p1, ysum, -yv[k]), kd_w * kd);
        }
        if (dvec && n == 8) {
            *reinterpret_cast<f32x4*>(dz + c0) = f32x4{o[0], o[1], o[2], o[3]};
            *reinterpret_cast<f32x4*>(dz + c0 + 4) = f32x4{o[4], o[5], o[6], o[7]};
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k < n) dz[c0 + k] = o[k];
        }
    }
}

// ---- token-layout Huber ------------------------------------------------------------------------------------------------
// A token row (b,i) is 3S contiguous floats, tokens[b,i,3j+c], against the three S-float rows x[b,c,i,:].  A workgroup
// takes R consecutive token rows per turn: the 3R image rows are staged into LDS with 16-byte loads ([r][c][j], the
// channel planes side by side), then every thread reads 16 bytes of tokens and picks its four partners from LDS — the
// interleave happens on chip, both tensors stream through coalesced vector accesses.  Dynamic LDS: R * 3S floats, then 8
// floats for the block sum (nothing static in front of it: the 16-byte carve stays aligned).
struct HuberGeom {
    int S, R, row4, groups;       // row4 = 3S/4 float4 per token row; groups = ceil(B*S / R)
    long rows;                    // B*S
};

template <bool BWD>
static __global__ __launch_bounds__(LOSS_NT) void huber_tokens_kernel(const float* __restrict__ tokens,
                                                                      const float* __restrict__ x, float delta,
                                                                      const float* __restrict__ dloss,
                                                                      float* __restrict__ out, const HuberGeom g) {
    extern __shared__ f32x4 huber_lds[];
    float* xs = reinterpret_cast<float*>(huber_lds);
    const int S = g.S, row4 = g.row4, s4 = S >> 2, tid = threadIdx.x;
    float* red = xs + (long)g.R * 3 * S;
    float acc = 0.f;
    float scale = 0.f;
    if (BWD) scale = dloss[0] / (3.f * (float)g.rows * (float)S);
    for (int grp = blockIdx.x; grp < g.groups; grp += gridDim.x) {
        const long r0 = (long)grp * g.R;
        const long left = g.rows - r0;
        const int nr = left < g.R ? (int)left : g.R;
        const int n4 = nr * row4;
        for (int q = tid; q < n4; q += LOSS_NT) {
            const int rr = q / row4, rem = q - rr * row4;
            const int c = rem / s4, j4 = rem - c * s4;
            const long r = r0 + rr;
            const long b = r / S, i = r - b * S;
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + (((b * 3 + c) * S + i) * S + 4 * j4));
            *reinterpret_cast<f32x4*>(xs + (rr * 3 + c) * S + 4 * j4) = v;
        }
        __syncthreads();
        for (int q = tid; q < n4; q += LOSS_NT) {
            const int rr = q / row4, rem = q - rr * row4;
            const long off = (r0 + rr) * 3 * S + 4 * rem;
            const f32x4 t = *reinterpret_cast<const f32x4*>(tokens + off);
            const float* xr = xs + rr * 3 * S;
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = 4 * rem + k;
                const int j = e / 3, c = e - 3 * j;
                const float d = t[k] - xr[c * S + j];
                if (BWD) {
                    o[k] = scale * fminf(fmaxf(d, -delta), delta);
                    if (d != d) o[k] = d;                       // (fminf / fmaxf drop a NaN: hand it on)
                } else {
                    const float ad = fabsf(d);
                    acc += ad <= delta ? 0.5f * d * d : (ad != ad ? d : delta * (ad - 0.5f * delta));
                }
            }
            if (BWD) *reinterpret_cast<f32x4*>(out + off) = o;
        }
        __syncthreads();
    }
    if (!BWD) {
        acc = block_sum_256(acc, red);
        if (tid == 0) out[blockIdx.x] = acc;
    }
}

static bool huber_geom(int B, int S, HuberGeom* g) {
    if ((S & 3) != 0 || S > 4096) return false;                 // 3S floats of LDS per token row: 48 KB at S = 4096
    g->S = S;
    g->row4 = 3 * S / 4;
    const int r = 768 / g->row4;                               // ~3 float4 per thread and turn
    g->R = r < 1 ? 1 : r;
    g->rows = (long)B * S;
    const long groups = (g->rows + g->R - 1) / g->R;
    if (groups > 0x7fffffffl) return false;
    g->groups = (int)groups;
    return true;
}
// (HUBER_MAX_GRID: the reduction plan in common.h, which also sizes `partials`)
static inline int huber_grid(const HuberGeom& g) { return g.groups < HUBER_MAX_GRID ? g.groups : HUBER_MAX_GRID; }
static inline size_t huber_lds_bytes(const HuberGeom& g) { return ((size_t)g.R * 3 * g.S + 8) * sizeof(float); }

extern "C" {

static inline int vec_groups(const float* a, long lda, const float* b, long ldb, int C) {
    return (aligned16(a) && aligned16(b) && (lda & 3) == 0 && (ldb & 3) == 0) ? C >> 2 : 0;
}

int calm_soft_ce_fwd(const float* logits, int64_t ld, const float* targets, int64_t td, float* row_stats, float* loss,
                     float* metrics, int32_t B, int32_t C, float* partials, void* stream) {
    if (!logits || !targets || !row_stats || !loss || !partials || B <= 0 || C <= 0) return CALM_E_INVAL;
    const int c4 = vec_groups(logits, (long)ld, targets, (long)td, C);
    // one workgroup per sample: B row losses at partials, B agreement flags behind them (SOFT_CE_PART_ROWS * B floats)
    if (int e = calm_launch(soft_ce_fwd_kernel, B, LOSS_NT, 0, stream, logits, ld, targets, td, row_stats, partials, B, C, c4))
        return e;
    return calm_launch(loss_final_kernel, 1, LOSS_NT, 0, stream, partials, B, 1.0f / (float)B, loss, partials + B, metrics, B,
                       1.0f);
}

int calm_soft_ce_bwd(const float* logits, int64_t ld, const float* targets, int64_t td, const float* row_stats,
                     const float* dloss, float* dlogits, int32_t B, int32_t C, void* stream) {
    if (!logits || !targets || !row_stats || !dloss || !dlogits || B <= 0 || C <= 0) return CALM_E_INVAL;
    const int c4 = (C & 3) == 0 && aligned16(dlogits) ? vec_groups(logits, (long)ld, targets, (long)td, C) : 0;
    return calm_launch(soft_ce_bwd_kernel, B, LOSS_NT, 0, stream, logits, ld, targets, td, row_stats, dloss, dlogits, B, C, c4);
}

// the checks both directions share, all before any launch
static int bce_args(const float* logits, const float* targets, int32_t flags, float threshold, int32_t B, int32_t C) {
    if (!logits || !targets || B <= 0 || C <= 0) return CALM_E_INVAL;
    if (flags & ~(CALM_BCE_SUM_CLASSES | CALM_BCE_THRESHOLD)) return CALM_E_INVAL;
    if ((flags & CALM_BCE_THRESHOLD) && !isfinite(threshold)) return CALM_E_INVAL;
    if ((int64_t)B * C >= ((int64_t)1 << 31)) return CALM_E_UNSUPP;      // (the divisor B C and the flat dlogits index)
    return 0;
}

int calm_bce_fwd(const float* logits, int64_t ld, const float* targets, int64_t td, int32_t flags, float threshold,
                 float* loss, float* metrics, int32_t B, int32_t C, float* partials, void* stream) {
    if (!loss || !partials) return CALM_E_INVAL;
    if (int e = bce_args(logits, targets, flags, threshold, B, C)) return e;
    const int c4 = vec_groups(logits, (long)ld, targets, (long)td, C);
    const int thresholded = (flags & CALM_BCE_THRESHOLD) != 0;
    const bool sum_classes = (flags & CALM_BCE_SUM_CLASSES) != 0;
    // one workgroup per sample: B row sums at partials, B agreement flags behind them (BCE_PART_ROWS * B floats)
    if (int e = calm_launch(bce_fwd_kernel, B, LOSS_NT, 0, stream, logits, ld, targets, td, thresholded, threshold, partials,
                            B, C, c4))
        return e;
    const float scale = 1.0f / (sum_classes ? (float)B : (float)B * (float)C);
    return calm_launch(loss_final_kernel, 1, LOSS_NT, 0, stream, partials, B, scale, loss, partials + B, metrics, B,
                       sum_classes ? 1.0f : 1.0f / (float)C);
}

int calm_bce_bwd(const float* logits, int64_t ld, const float* targets, int64_t td, int32_t flags, float threshold,
                 const float* dloss, float* dlogits, int32_t B, int32_t C, void* stream) {
    if (!dloss || !dlogits) return CALM_E_INVAL;
    if (int e = bce_args(logits, targets, flags, threshold, B, C)) return e;
    const int c4 = (C & 3) == 0 && aligned16(dlogits) ? vec_groups(logits, (long)ld, targets, (long)td, C) : 0;
    const float denom = (flags & CALM_BCE_SUM_CLASSES) ? (float)B : (float)B * (float)C;
    return calm_launch(bce_bwd_kernel, B, LOSS_NT, 0, stream, logits, ld, targets, td,
                       (int)((flags & CALM_BCE_THRESHOLD) != 0), threshold, denom, dloss, dlogits, C, c4);
}

int calm_top1_count(const float* logits, int64_t ld, const int64_t* labels, float* metrics, int32_t B, int32_t C,
                    void* stream) {
    if (!logits || !labels || !metrics || B <= 0 || C <= 0) return CALM_E_INVAL;
    const int c4 = aligned16(logits) && (ld & 3) == 0 ? C >> 2 : 0;
    return calm_launch(top1_count_kernel, 1, TOP1_NT, 0, stream, logits, ld, reinterpret_cast<const long long*>(labels),
                       metrics, B, C, c4);
}

int calm_eval_metrics(const void* logits, int64_t ld, int32_t logits_type, const int64_t* labels, const int32_t* ks,
                      int32_t nk, int64_t* counts, double* loss_sum, int64_t* confusion, int32_t B, int32_t C,
                      float* partials, void* stream) {
    if (!logits || !labels || !ks || !counts || !loss_sum || !partials || B <= 0 || C <= 0 || ld < C) return CALM_E_INVAL;
    if (nk < 1 || nk > 4) return CALM_E_INVAL;
    if (logits_type != CALM_ST_F32 && logits_type != CALM_ST_BF16) return CALM_E_INVAL;
    EvalKs k{};
    k.nk = nk;
    for (int i = 0; i < nk; ++i) {
        if (ks[i] < 1) return CALM_E_INVAL;
        k.k[i] = ks[i];
    }
    if (C > 65536) return CALM_E_UNSUPP;                         // a fold thread owns C / 1024 classes, a scan of the chunk each
    if (!aligned16(partials)) return CALM_E_LAYOUT;              // (the records are 16-byte stores)
    const bool bf16 = logits_type == CALM_ST_BF16;
    const int vec = bf16 ? 8 : 4;
    const int cv = aligned16(logits) && (ld % vec) == 0 ? C / vec : 0;
    const int grid = (B + LOSS_NT / 64 - 1) / (LOSS_NT / 64);
    const long long* lab = reinterpret_cast<const long long*>(labels);
    if (int e = with_bool(bf16, [&](auto b16) {
            return calm_launch(eval_rows_kernel<decltype(b16)::value>, grid, LOSS_NT, 0, stream, logits, ld, lab, partials, B,
                               C, cv);
        }))
        return e;
    return calm_launch(eval_fold_kernel, 1, EVAL_FOLD_NT, 0, stream, partials, lab, reinterpret_cast<long long*>(counts),
                       loss_sum, reinterpret_cast<long long*>(confusion), B, C, k);
}

int calm_huber_tokens_fwd(const float* tokens, const float* x, float delta, float* loss, int32_t B, int32_t S,
                          float* partials, void* stream) {
    if (!tokens || !x || !loss || !partials || B <= 0 || S <= 0) return CALM_E_INVAL;
    HuberGeom g;
    if (!huber_geom(B, S, &g)) return CALM_E_UNSUPP;
    if (!aligned16(tokens) || !aligned16(x)) return CALM_E_LAYOUT;
    const int grid = huber_grid(g);
    if (int e = calm_launch(huber_tokens_kernel<false>, grid, LOSS_NT, huber_lds_bytes(g), stream, tokens, x, delta, nullptr,
                            partials, g))
        return e;
    return calm_launch(loss_final_kernel, 1, LOSS_NT, 0, stream, partials, grid, 1.0f / (3.0f * (float)g.rows * (float)S),
                       loss, nullptr, nullptr, 0, 1.0f);
}

int calm_huber_tokens_bwd(const float* tokens, const float* x, float delta, const float* dloss, float* dtokens, int32_t B,
                          int32_t S, void* stream) {
    if (!tokens || !x || !dloss || !dtokens || B <= 0 || S <= 0) return CALM_E_INVAL;
    HuberGeom g;
    if (!huber_geom(B, S, &g)) return CALM_E_UNSUPP;
    if (!aligned16(tokens) || !aligned16(x) || !aligned16(dtokens)) return CALM_E_LAYOUT;
    return calm_launch(huber_tokens_kernel<true>, huber_grid(g), LOSS_NT, huber_lds_bytes(g), stream, tokens, x, delta, dloss,
                       dtokens, g);
}

// the checks both directions share (all before any launch) and the kernels' view of the arguments
static int distill_args(const float* logits, int64_t ld, const void* teacher, int64_t tld, int32_t teacher_type,
                        const float* targets, int64_t td, float temperature, float alpha, int32_t mode, int32_t B, int32_t C,
                        DistillArgs* a) {
    if (!logits || !teacher || !targets || B <= 0 || C <= 0 || ld < C || tld < C || td < C) return CALM_E_INVAL;
    if (!(temperature > 0.f) || !isfinite(temperature) || !(alpha >= 0.f && alpha <= 1.f)) return CALM_E_INVAL;
    if (mode != CALM_DISTILL_SOFT && mode != CALM_DISTILL_HARD) return CALM_E_INVAL;
    if (teacher_type != CALM_ST_F32 && teacher_type != CALM_ST_BF16) return CALM_E_INVAL;
    if (C > 65536) return CALM_E_UNSUPP;                         // (the teacher argmax travels as a float in row_stats)
    const bool soft = mode == CALM_DISTILL_SOFT;
    a->logits = logits; a->teacher = teacher; a->targets = targets;
    a->ld = (long)ld; a->tld = (long)tld; a->td = (long)td;
    a->inv_t = 1.0f / temperature;
    a->alpha = alpha;
    a->w = soft ? alpha * temperature * temperature : alpha;
    a->gw = soft ? alpha * temperature : alpha;
    a->mode = mode; a->B = B; a->C = C;
    a->zvec = aligned16(logits) && (ld & 3) == 0;
    a->yvec = aligned16(targets) && (td & 3) == 0;
    a->tvec = aligned16(teacher) && (tld % (teacher_type == CALM_ST_BF16 ? 8 : 4)) == 0;
    return 0;
}

int calm_distill_fwd(const float* logits, int64_t ld, const void* teacher, int64_t tld, int32_t teacher_type,
                     const float* targets, int64_t td, float temperature, float alpha, int32_t mode, float* row_stats,
                     float* loss, float* metrics, float* dmetrics, int32_t B, int32_t C, float* partials, void* stream) {
    if (!row_stats || !loss || !partials) return CALM_E_INVAL;
    DistillArgs a;
    if (int e = distill_args(logits, ld, teacher, tld, teacher_type, targets, td, temperature, alpha, mode, B, C, &a)) return e;
    if (!aligned16(partials)) return CALM_E_LAYOUT;
    // one workgroup per sample: DISTILL_PART_ROWS * B floats of partials
    const bool bf16 = teacher_type == CALM_ST_BF16, cached = C <= DISTILL_CACHED_C;
    if (int e = with_bool(bf16, [&](auto b16) {
            return with_bool(cached, [&](auto c) {
                return calm_launch(distill_fwd_kernel<decltype(c)::value, decltype(b16)::value>, B, LOSS_NT, 0, stream, a,
                                   row_stats, partials);
            });
        }))
        return e;
    return calm_launch(distill_final_kernel, 1, LOSS_NT, 0, stream, partials, B, loss, metrics, dmetrics);
}

int calm_distill_bwd(const float* logits, int64_t ld, const void* teacher, int64_t tld, int32_t teacher_type,
                     const float* targets, int64_t td, float temperature, float alpha, int32_t mode, const float* row_stats,
                     const float* dloss, float* dlogits, int32_t B, int32_t C, void* stream) {
    if (!row_stats || !dloss || !dlogits) return CALM_E_INVAL;
    DistillArgs a;
    if (int e = distill_args(logits, ld, teacher, tld, teacher_type, targets, td, temperature, alpha, mode, B, C, &a)) return e;
    const int dvec = aligned16(dlogits) && (C & 3) == 0;
    return with_bool(teacher_type == CALM_ST_BF16, [&](auto b16) {
        return calm_launch(distill_bwd_kernel<decltype(b16)::value>, B, LOSS_NT, 0, stream, a, row_stats, dloss, dlogits, dvec);
    });
}

}  // extern "C"
