// Dropout of the CALM-ViT block (Vi_Tools:301 after out_proj * ls_att, Vi_Tools:203 inside the MLP) as ONE streaming
// kernel with a counter-based mask: no mask tensor exists in HBM, the backward regenerates it from the 16-byte key.
//
//   y[j] = x[j] * (word(e) >= thr ? scale : 0) + (residual ? residual[j] : 0),   e = e0 + j
//
// word(e) is output word e & 3 of Philox4x32-10 (Salmon et al., SC'11) on the counter (lo32(e >> 2), hi32(e >> 2),
// lo32(offset), hi32(offset)) under the key (lo32(seed), hi32(seed)): the mask is a function of (seed, offset, e) alone —
// not of the grid, the vector width or the storage types.  (seed, offset) are read from device memory, so the entry point
// needs no host synchronisation and a captured graph replays with whatever key its key tensor then holds.
//
// One Philox call serves four consecutive elements.  A thread owns units of 4 (all tensors fp32) or 8 (any tensor bf16)
// elements and moves every tensor as 16-byte vectors; the n % unit last elements, and every element when a base is not
// 16-byte aligned, take the element-wise loop.  The multiply and the add are two fp32 roundings (no contraction
// into an fma), bf16 inputs widen exactly and a bf16 output is one round-to-nearest-even of the fp32
// result.  It is a multiply, not a select: a dropped NaN / inf yields NaN.  y may alias x (each element is read by the
// thread that writes it, before it writes it).  No LDS, no atomics.
#include "common.h"
#include "philox.h"

// The multiply and the add round separately.  hipcc compiles with fp-contract=fast, and __fmul_rn / __fadd_rn are plain
// operators in the HIP headers — compiled there, they keep the `contract` flag and are fused into one fma all the same —
// so the two operations are written with operators here, under a pragma that drops the flag for this file.
#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 2048;   // 256 CUs x 8 blocks

inline int grid_for(int64_t work_items, int per_block) {
    int64_t g = (work_items + per_block - 1) / per_block;
    if (g > MAX_BLOCKS) g = MAX_BLOCKS;
    if (g < 1) g = 1;
    return (int)g;
}
bool st_ok(int t) { return t == CALM_ST_F32 || t == CALM_ST_BF16; }

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

typedef PhiloxKey DropKey;                          // key words and the upper counter words: the same for every element

__device__ __forceinline__ DropKey drop_key(const uint64_t* key) { return philox_key(key[0], key[1]); }

__device__ __forceinline__ float drop_one(float x, uint32_t word, uint32_t thr, float scale) {
    return x * (word >= thr ? scale : 0.0f);
}
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

__device__ __forceinline__ float ld1(const void* p, long i, int type) {
    return type == CALM_ST_BF16 ? (float)reinterpret_cast<const __bf16*>(p)[i] : reinterpret_cast<const float*>(p)[i];
}

// elements [first, n), one per thread and pass (each thread runs the Philox call of its element's group of four)
__device__ __forceinline__ void drop_elements(const void* x, const void* res, void* y, long first, long n, uint64_t g0,
                                              uint32_t thr, float scale, const DropKey& k, int x_type, int r_type,
                                              int y_type) {
    const long stride = (long)gridDim.x * NT;
    for (long j = first + (long)blockIdx.x * NT + threadIdx.x; j < n; j += stride) {
        const u32x4 w = philox4x32_10(g0 + (uint64_t)(j >> 2), k);
        const int q = (int)(j & 3);
        const uint32_t word = q == 0 ? w[0] : q == 1 ? w[1] : q == 2 ? w[2] : w[3];
        float v = drop_one(ld1(x, j, x_type), word, thr, scale);
        if (res) v = add_rn(v, ld1(res, j, r_type));
        if (y_type == CALM_ST_BF16) reinterpret_cast<__bf16*>(y)[j] = (__bf16)v;
        else reinterpret_cast<float*>(y)[j] = v;
    }
}

// EPT elements per thread and pass: 8 when a tensor is bf16 (its 16-byte vector), else 4.  R: 0 = no residual, 1 = fp32,
// 2 = bf16.  The tensors carry no __restrict__: y may be x.
template <bool X16, int R, bool Y16>
__global__ __launch_bounds__(NT) void dropout_vec_kernel(const void* x, const void* res, void* y, long n,
                                                         uint64_t g0, uint32_t thr, float scale,
                                                         const uint64_t* __restrict__ key) {
    constexpr int EPT = (X16 || Y16 || R == 2) ? 8 : 4;
    const DropKey k = drop_key(key);
    const long stride = (long)gridDim.x * NT, units = n / EPT;
    for (long u = (long)blockIdx.x * NT + threadIdx.x; u < units; u += stride) {
        f32x4 v[EPT / 4];
        if constexpr (X16 && EPT == 8) {                       // one 16-byte load of eight bf16
            const bf16x8 t = reinterpret_cast<const bf16x8*>(x)[u];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i / 4][i % 4] = (float)t[i];
        } else {
#pragma unroll
            for (int h = 0; h < EPT / 4; ++h) v[h] = reinterpret_cast<const f32x4*>(x)[u * (EPT / 4) + h];
        }
#pragma unroll
        for (int h = 0; h < EPT / 4; ++h) {
            const u32x4 w = philox4x32_10(g0 + (uint64_t)u * (EPT / 4) + h, k);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[h][i] = drop_one(v[h][i], w[i], thr, scale);
        }
        if constexpr (R == 2) {
            const bf16x8 t = reinterpret_cast<const bf16x8*>(res)[u];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i / 4][i % 4] = add_rn(v[i / 4][i % 4], (float)t[i]);
        } else if constexpr (R == 1) {
#pragma unroll
            for (int h = 0; h < EPT / 4; ++h) {
                const f32x4 t = reinterpret_cast<const f32x4*>(res)[u * (EPT / 4) + h];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[h][i] = add_rn(v[h][i], t[i]);
            }
        }
        if constexpr (Y16) {
            bf16x8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = (__bf16)v[i / 4][i % 4];
            reinterpret_cast<bf16x8*>(y)[u] = o;
        } else {
#pragma unroll
            for (int h = 0; h < EPT / 4; ++h) reinterpret_cast<f32x4*>(y)[u * (EPT / 4) + h] = v[h];
        }
    }
    drop_elements(x, R ? res : nullptr, y, units * EPT, n, g0, thr, scale, k, X16 ? CALM_ST_BF16 : CALM_ST_F32,
                  R == 2 ? CALM_ST_BF16 : CALM_ST_F32, Y16 ? CALM_ST_BF16 : CALM_ST_F32);       // the n % EPT last elements
}

// every element of a call whose bases are not all 16-byte aligned; storage types are run-time values here
__global__ __launch_bounds__(NT) void dropout_elem_kernel(const void* x, const void* res, void* y, long n, uint64_t g0,
                                                          uint32_t thr, float scale, const uint64_t* __restrict__ key,
                                                          int x_type, int r_type, int y_type) {
    drop_elements(x, res, y, 0, n, g0, thr, scale, drop_key(key), x_type, r_type, y_type);
}

}  // namespace

extern "C" {

int calm_dropout(const void* x, const void* residual, void* y, int64_t n, int64_t e0, float p, const uint64_t* key,
                 int32_t x_type, int32_t r_type, int32_t y_type, void* stream) {
    if (!x || !y || !key || n < 0 || !(p >= 0.0f && p < 1.0f) || e0 < 0 || (e0 & 3)) return CALM_E_INVAL;
    if (!st_ok(x_type) || !st_ok(r_type) || !st_ok(y_type)) return CALM_E_INVAL;
    if (n == 0) return 0;
    const uint32_t thr = (uint32_t)((double)p * 4294967296.0);
    const float scale = 1.0f / (1.0f - p);
    const uint64_t g0 = (uint64_t)e0 >> 2;
    const bool x16 = x_type == CALM_ST_BF16, y16 = y_type == CALM_ST_BF16, r16 = r_type == CALM_ST_BF16;
    const int ept = (x16 || y16 || (residual && r16)) ? 8 : 4;
    if (!(aligned16(x) && aligned16(y) && aligned16(residual)))
        return calm_launch(dropout_elem_kernel, grid_for(n, NT), NT, 0, stream, x, residual, y, n, g0, thr, scale, key,
                           x_type, r_type, y_type);
    const int r = !residual ? 0 : r16 ? 2 : 1;
    return with_bool(x16, [&](auto xb) {
        return with_int<0, 1, 2>(r, [&](auto rv) {
            return with_bool(y16, [&](auto yb) {
                return calm_launch(dropout_vec_kernel<decltype(xb)::value, decltype(rv)::value, decltype(yb)::value>,
                                   grid_for(n / ept, NT), NT, 0, stream, x, residual, y, n, g0, thr, scale, key);
            });
        });
    });
}

}  // extern "C"
