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
//
// Stochastic depth (calm_drop_path) is the per-sample sibling: row b of a [B, L] tensor is multiplied by ONE factor, decided
// by word(sample0 + b) of the same generator, under the same arithmetic contract and with the same vector / element-wise
// split.
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

// One unit of EPT elements — 8 when a tensor is bf16 (its 16-byte vector), else 4 — as EPT / 4 fp32 quads: a bf16 tensor
// moves as one 16-byte vector, an fp32 tensor as EPT / 4 of them.  R: 0 = no residual, 1 = fp32, 2 = bf16.
template <bool X16, int R, bool Y16>
constexpr int unit_elems() { return (X16 || Y16 || R == 2) ? 8 : 4; }

template <bool T16, int EPT>
__device__ __forceinline__ void load_unit(const void* p, long u, f32x4 (&v)[EPT / 4]) {
    if constexpr (T16) {                                       // one 16-byte load of eight bf16 (T16 implies EPT == 8)
        const bf16x8 t = reinterpret_cast<const bf16x8*>(p)[u];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i / 4][i % 4] = (float)t[i];
    } else {
#pragma unroll
        for (int h = 0; h < EPT / 4; ++h) v[h] = reinterpret_cast<const f32x4*>(p)[u * (EPT / 4) + h];
    }
}
template <int R, int EPT>
__device__ __forceinline__ void add_unit(const void* res, long u, f32x4 (&v)[EPT / 4]) {
    if constexpr (R != 0) {
        f32x4 t[EPT / 4];
        load_unit<R == 2, EPT>(res, u, t);
#pragma unroll
        for (int h = 0; h < EPT / 4; ++h)
#pragma unroll
            for (int i = 0; i < 4; ++i) v[h][i] = add_rn(v[h][i], t[h][i]);
    }
}
template <bool T16, int EPT>
__device__ __forceinline__ void store_unit(void* p, long u, const f32x4 (&v)[EPT / 4]) {
    if constexpr (T16) {
        bf16x8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (__bf16)v[i / 4][i % 4];
        reinterpret_cast<bf16x8*>(p)[u] = o;
    } else {
#pragma unroll
        for (int h = 0; h < EPT / 4; ++h) reinterpret_cast<f32x4*>(p)[u * (EPT / 4) + h] = v[h];
    }
}

// The tensors carry no __restrict__: y may be x.
template <bool X16, int R, bool Y16>
__global__ __launch_bounds__(NT) void dropout_vec_kernel(const void* x, const void* res, void* y, long n,
                                                         uint64_t g0, uint32_t thr, float scale,
                                                         const uint64_t* __restrict__ key) {
    constexpr int EPT = unit_elems<X16, R, Y16>();
    const DropKey k = drop_key(key);
    const long stride = (long)gridDim.x * NT, units = n / EPT;
    for (long u = (long)blockIdx.x * NT + threadIdx.x; u < units; u += stride) {
        f32x4 v[EPT / 4];
        load_unit<X16, EPT>(x, u, v);
#pragma unroll
        for (int h = 0; h < EPT / 4; ++h) {
            const u32x4 w = philox4x32_10(g0 + (uint64_t)u * (EPT / 4) + h, k);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[h][i] = drop_one(v[h][i], w[i], thr, scale);
        }
        add_unit<R, EPT>(res, u, v);
        store_unit<Y16, EPT>(y, u, v);
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

// ---- stochastic depth: one decision per sample (row), the word calm_dropout defines for element index sample0 + b ------
// A workgroup walks (sample, chunk-of-row) pairs, pair = blockIdx.x + i * gridDim.x = b * cpr + c with cpr chunks of NT
// units (vector kernel) or NT elements (element-wise kernel) per row.  (b, c) advance by (gridDim.x / cpr, gridDim.x % cpr)
// with a carry — both computed on the host — so the walk holds no division; the first pair's division is a 32-bit one
// (blockIdx.x < MAX_BLOCKS, and cpr32 = min(cpr, 2^31 - 1) divides like cpr below that).
struct PathWalk {
    long B, cpr, db, dc;
    uint32_t cpr32;
};

// f_b: the sample index, its Philox call and the factor are uniform over the workgroup — once per pair
__device__ __forceinline__ float path_factor(uint64_t s, uint32_t thr, float scale, const DropKey& k) {
    const u32x4 w = philox4x32_10(s >> 2, k);
    const int q = (int)(s & 3);
    const uint32_t word = q == 0 ? w[0] : q == 1 ? w[1] : q == 2 ? w[2] : w[3];
    return word >= thr ? scale : 0.0f;
}

// body(b, c, f) for every pair of this workgroup
template <class Body>
__device__ __forceinline__ void path_walk(const PathWalk& w, uint64_t sample0, uint32_t thr, float scale,
                                          const uint64_t* __restrict__ key, Body&& body) {
    const DropKey k = drop_key(key);
    long b = blockIdx.x / w.cpr32, c = blockIdx.x % w.cpr32;
    while (b < w.B) {
        body(b, c, path_factor(sample0 + (uint64_t)b, thr, scale, k));
        b += w.db;
        c += w.dc;
        if (c >= w.cpr) {
            c -= w.cpr;
            ++b;
        }
    }
}

// rows of UL units of EPT elements each (L == UL * EPT, every base 16-byte aligned: every row starts on a vector)
template <bool X16, int R, bool Y16>
__global__ __launch_bounds__(NT) void drop_path_vec_kernel(const void* x, const void* res, void* y, long UL, PathWalk w,
                                                           uint64_t sample0, uint32_t thr, float scale,
                                                           const uint64_t* __restrict__ key) {
    constexpr int EPT = unit_elems<X16, R, Y16>();
    path_walk(w, sample0, thr, scale, key, [&](long b, long c, float f) {
        const long ur = c * NT + threadIdx.x;                  // unit within the row
        if (ur >= UL) return;
        const long u = b * UL + ur;
        f32x4 v[EPT / 4];
        load_unit<X16, EPT>(x, u, v);
#pragma unroll
        for (int h = 0; h < EPT / 4; ++h) v[h] = v[h] * f;     // a multiply, not a select
        add_unit<R, EPT>(res, u, v);
        store_unit<Y16, EPT>(y, u, v);
    });
}

// any L and any alignment; storage types are run-time values here
__global__ __launch_bounds__(NT) void drop_path_elem_kernel(const void* x, const void* res, void* y, long L, PathWalk w,
                                                            uint64_t sample0, uint32_t thr, float scale,
                                                            const uint64_t* __restrict__ key, int x_type, int r_type,
                                                            int y_type) {
    path_walk(w, sample0, thr, scale, key, [&](long b, long c, float f) {
        const long jr = c * NT + threadIdx.x;
        if (jr >= L) return;
        const long j = b * L + jr;
        float v = ld1(x, j, x_type) * f;
        if (res) v = add_rn(v, ld1(res, j, r_type));
        if (y_type == CALM_ST_BF16) reinterpret_cast<__bf16*>(y)[j] = (__bf16)v;
        else reinterpret_cast<float*>(y)[j] = v;
    });
}

// the walk of B rows of `per_row` work items (units or elements) and its grid
inline PathWalk path_walk_for(int64_t B, int64_t per_row, int* grid) {
    const int64_t cpr = (per_row + NT - 1) / NT;
    *grid = (int)(B <= MAX_BLOCKS / cpr ? B * cpr : MAX_BLOCKS);       // min(B * cpr, MAX_BLOCKS) without the overflow
    return {B, cpr, *grid / cpr, *grid % cpr, (uint32_t)(cpr < 0x7fffffff ? cpr : 0x7fffffff)};
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

int calm_drop_path(const void* x, const void* residual, void* y, int64_t B, int64_t L, int64_t sample0, float p,
                   const uint64_t* key, int32_t x_type, int32_t r_type, int32_t y_type, void* stream) {
    if (!x || !y || !key || B < 0 || L < 0 || sample0 < 0 || !(p >= 0.0f && p < 1.0f)) return CALM_E_INVAL;
    if (!st_ok(x_type) || !st_ok(r_type) || !st_ok(y_type)) return CALM_E_INVAL;
    if (B == 0 || L == 0) return 0;
    const uint32_t thr = (uint32_t)((double)p * 4294967296.0);
    const float scale = 1.0f / (1.0f - p);
    const bool x16 = x_type == CALM_ST_BF16, y16 = y_type == CALM_ST_BF16, r16 = r_type == CALM_ST_BF16;
    const int ept = (x16 || y16 || (residual && r16)) ? 8 : 4;
    int grid;
    if (!(aligned16(x) && aligned16(y) && aligned16(residual)) || L % ept) {
        const PathWalk w = path_walk_for(B, L, &grid);
        return calm_launch(drop_path_elem_kernel, grid, NT, 0, stream, x, residual, y, L, w, (uint64_t)sample0, thr, scale,
                           key, x_type, r_type, y_type);
    }
    const PathWalk w = path_walk_for(B, L / ept, &grid);
    const int r = !residual ? 0 : r16 ? 2 : 1;
    return with_bool(x16, [&](auto xb) {
        return with_int<0, 1, 2>(r, [&](auto rv) {
            return with_bool(y16, [&](auto yb) {
                return calm_launch(drop_path_vec_kernel<decltype(xb)::value, decltype(rv)::value, decltype(yb)::value>,
                                   grid, NT, 0, stream, x, residual, y, L / ept, w, (uint64_t)sample0, thr, scale, key);
            });
        });
    });
}

}  // extern "C"
