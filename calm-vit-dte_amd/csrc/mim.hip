// Masked image modelling on row tokens (SimMIM / MAE style pre-training of the generative job): a per-sample patch mask with
// EXACTLY k set patches drawn from the counter-based generator of calm_dropout, the masked copy of the batch, and the Huber
// loss over the masked elements only.
//
// Tokens are [B, S, 3S] fp32, tokens[b, r, 3x + c] (the channels-last image).  Patch side p, S % p == 0, G = S / p <= 32,
// P = G * G <= 1024; pixel (r, x) lies in patch i = (r / p) * G + x / p, and mask is uint8 [B, P].
//
// calm_mim_draw: one workgroup per sample.  word(e) of dropout.hip for e = (sample0 + b) * 1024 + i, i < P, goes into LDS
// (one Philox call serves four patches: the slot stride 1024 is a multiple of four, so patch i is word i & 3 of call
// (sample0 + b) * 256 + (i >> 2)); every thread then ranks its patches against all P words — rank(i) = #{j : w_j < w_i, or
// w_j == w_i and j < i}, a permutation of 0 .. P - 1 — and sets the k lowest.  At most 2^20 compares per sample, all of
// them LDS broadcasts; no sort, no atomics, no host read of the key.
//
// The streaming kernels walk the flat tensor (n = 3 B S^2 < 2^31 elements) as 16-byte vectors when every base is 16-byte
// aligned, element by element otherwise, and the n % 4 last elements always one by one.  The mask decision is per ELEMENT:
// a vector whose four elements share a patch (the common case: one 32-bit division chain per vector, one mask byte) is
// decided at once, a vector that straddles a patch edge (3p % 4 != 0) or a row end (3S % 4 != 0) element by element.  All
// of them SELECT, none multiplies: what lies outside the mask is never combined with anything, and the loss kernels do not
// even load a vector that is wholly unmasked — at ratio 0.6 the backward reads 60 % of two tensors.
// Cross-workgroup sums: one block sum per workgroup into `partials`, one final workgroup in a fixed order (huber.h).
#include <math.h>

#include "common.h"
#include "huber.h"
#include "philox.h"

namespace {

constexpr int NT = HUBER_NT;
constexpr int DRAW_MAX_GRID = 65536;

struct MimGeom {
    uint32_t E, S, p, p3, G, P;                     // E = 3S elements per image row, p3 = 3p elements per patch row
};
struct MimFill { float v[3]; };

// the mask byte of element e
__device__ __forceinline__ uint32_t mim_slot(uint32_t e, const MimGeom& g) {
    const uint32_t row = e / g.E, col = e - row * g.E;
    const uint32_t b = row / g.S, r = row - b * g.S;
    return b * g.P + (r / g.p) * g.G + col / g.p3;
}

// the decisions of elements e0 .. e0 + 3 (e0 + 3 < n); returns how many are set
__device__ __forceinline__ int mim_vec_mask(uint32_t e0, const MimGeom& g, const uint8_t* __restrict__ mask, bool (&m)[4]) {
    const uint32_t row = e0 / g.E, col = e0 - row * g.E;
    const uint32_t pc = col / g.p3;
    if (col + 3 < (pc + 1) * g.p3) {                // one patch ((pc + 1) * p3 <= E: one row as well)
        const uint32_t b = row / g.S, r = row - b * g.S;
        const bool on = mask[b * g.P + (r / g.p) * g.G + pc] != 0;
        m[0] = m[1] = m[2] = m[3] = on;
        return on ? 4 : 0;
    }
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) c += (m[k] = mask[mim_slot(e0 + k, g)] != 0);
    return c;
}

__device__ __forceinline__ float fill_of(const MimFill& f, uint32_t c) { return c == 0 ? f.v[0] : c == 1 ? f.v[1] : f.v[2]; }

// ---- the mask -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void mim_draw_kernel(uint8_t* __restrict__ mask, long B, int P, int k, uint64_t sample0,
                                                      const uint64_t* __restrict__ key) {
    __shared__ uint32_t w[1024];
    const PhiloxKey pk = philox_key(key[0], key[1]);
    const int t = threadIdx.x;
    for (long b = blockIdx.x; b < B; b += gridDim.x) {             // (the same trip count for the whole workgroup)
        if (4 * t < P) {
            const u32x4 v = philox4x32_10((sample0 + (uint64_t)b) * 256u + (uint64_t)t, pk);
            w[4 * t] = v[0];
            w[4 * t + 1] = v[1];
            w[4 * t + 2] = v[2];
            w[4 * t + 3] = v[3];
        }
        __syncthreads();
        for (int i = t; i < P; i += NT) {
            const uint32_t wi = w[i];
            int rank = 0;
            for (int j = 0; j < P; ++j) {
                const uint32_t wj = w[j];
                rank += (wj < wi || (wj == wi && j < i)) ? 1 : 0;
            }
            mask[b * P + i] = rank < k ? 1 : 0;
        }
        __syncthreads();                                           // the next sample overwrites the words
    }
}

// ---- y = mask ? fill : x -----------------------------------------------------------------------------------------------------
// No __restrict__ on the tensors: y may be x (an element is read by the thread that writes it, before it writes it).  In
// place, a wholly unmasked vector is neither read nor written.
__global__ __launch_bounds__(NT) void mim_apply_kernel(const float* x, float* y, const uint8_t* __restrict__ mask,
                                                       const MimFill fill, const MimGeom g, uint32_t n, uint32_t n4) {
    const uint32_t stride = gridDim.x * NT, t0 = blockIdx.x * NT + threadIdx.x;
    const bool in_place = x == y;
    for (uint32_t q = t0; q < n4; q += stride) {
        bool m[4];
        const int set = mim_vec_mask(4 * q, g, mask, m);
        if (set == 0 && in_place) continue;
        const uint32_t c0 = (4 * q) % 3;                           // E % 3 == 0: the channel of element e is e % 3
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (set < 4) o = *reinterpret_cast<const f32x4*>(x + 4 * q);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = m[k] ? fill_of(fill, (c0 + k) % 3) : o[k];
        *reinterpret_cast<f32x4*>(y + 4 * q) = o;
    }
    for (uint32_t e = 4 * n4 + t0; e < n; e += stride) {
        if (mask[mim_slot(e, g)]) y[e] = fill_of(fill, e % 3);
        else if (!in_place) y[e] = x[e];
    }
}

// ---- Huber over the masked elements --------------------------------------------------------------------------------------
// forward: one block sum per workgroup into out[blockIdx.x]; backward: out = dtokens, every element written.
template <bool BWD>
__global__ __launch_bounds__(NT) void mim_huber_kernel(const float* __restrict__ tokens, const float* __restrict__ target,
                                                       const uint8_t* __restrict__ mask, float delta,
                                                       const float* __restrict__ dloss, float* __restrict__ out,
                                                       const MimGeom g, uint32_t n, uint32_t n4, float count) {
    __shared__ float red[8];
    const uint32_t stride = gridDim.x * NT, t0 = blockIdx.x * NT + threadIdx.x;
    float acc = 0.f, scale = 0.f;
    if (BWD) scale = dloss[0] / count;
    for (uint32_t q = t0; q < n4; q += stride) {
        bool m[4];
        const int set = mim_vec_mask(4 * q, g, mask, m);
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (set) {                                                 // a wholly unmasked vector is not loaded
            const f32x4 a = *reinterpret_cast<const f32x4*>(tokens + 4 * q);
            const f32x4 b = *reinterpret_cast<const f32x4*>(target + 4 * q);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = a[k] - b[k];
                if (BWD) o[k] = m[k] ? scale * huber_slope(d, delta) : 0.f;
                else acc += m[k] ? huber_value(d, delta) : 0.f;
            }
        }
        if (BWD) *reinterpret_cast<f32x4*>(out + 4 * q) = o;
    }
    for (uint32_t e = 4 * n4 + t0; e < n; e += stride) {
        float v = 0.f;
        if (mask[mim_slot(e, g)]) {
            const float d = tokens[e] - target[e];
            v = BWD ? scale * huber_slope(d, delta) : huber_value(d, delta);
        }
        if (BWD) out[e] = v;
        else acc += v;
    }
    if (!BWD) {
        acc = block_sum_256(acc, red);
        if (threadIdx.x == 0) out[blockIdx.x] = acc;
    }
}

inline int mim_grid(long n) {
    const long g = (n / 4 + NT - 1) / NT + 1;                      // ~one vector per thread and turn at the cap
    return g < MIM_MAX_GRID ? (int)g : MIM_MAX_GRID;
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// the shape checks the three streaming entry points share: 0 and the geometry, or the refusal
int mim_geom(int32_t B, int32_t S, int32_t p, MimGeom* g, long* n) {
    if (S <= 0 || p <= 0 || S % p) return CALM_E_INVAL;
    if (S / p > 32 || 3.0 * (double)B * (double)S * (double)S >= 2147483648.0) return CALM_E_UNSUPP;
    const uint32_t G = (uint32_t)(S / p);
    *g = MimGeom{3u * (uint32_t)S, (uint32_t)S, (uint32_t)p, 3u * (uint32_t)p, G, G * G};
    *n = 3l * B * S * S;
    return 0;
}

// the checks of the two loss entry points behind their null checks
int mim_huber_args(int32_t B, int32_t S, int32_t p, float delta, int64_t masked, MimGeom* g, long* n) {
    if (B <= 0 || !(delta > 0.0f) || !(fabsf(delta) <= 3.402823466e+38f) || masked <= 0) return CALM_E_INVAL;
    if (int e = mim_geom(B, S, p, g, n)) return e;
    if (masked > (int64_t)B * g->P) return CALM_E_INVAL;
    return 0;
}

}  // namespace

extern "C" {

int calm_mim_draw(uint8_t* mask, int64_t B, int32_t G, int32_t k, int64_t sample0, const uint64_t* key, void* stream) {
    if (!mask || !key || B < 0 || G < 1 || k < 0 || sample0 < 0 || B > (1ll << 53) - sample0) return CALM_E_INVAL;
    if ((int64_t)k > (int64_t)G * G) return CALM_E_INVAL;
    if (G > 32) return CALM_E_UNSUPP;
    if (B == 0) return 0;
    const int grid = (int)(B < DRAW_MAX_GRID ? B : DRAW_MAX_GRID);
    return calm_launch(mim_draw_kernel, grid, NT, 0, stream, mask, B, G * G, k, (uint64_t)sample0, key);
}

int calm_mim_apply(const float* x, float* y, const uint8_t* mask, const float* fill, int32_t B, int32_t S, int32_t p,
                   void* stream) {
    if (!x || !y || !mask || !fill || B < 0) return CALM_E_INVAL;
    MimGeom g;
    long n;
    if (int e = mim_geom(B, S, p, &g, &n)) return e;
    if (!aligned4(x) || !aligned4(y)) return CALM_E_LAYOUT;
    if (B == 0) return 0;
    const MimFill f{{fill[0], fill[1], fill[2]}};
    const long n4 = aligned16(x) && aligned16(y) ? n / 4 : 0;
    return calm_launch(mim_apply_kernel, mim_grid(n), NT, 0, stream, x, y, mask, f, g, (uint32_t)n, (uint32_t)n4);
}

int calm_mim_huber_fwd(const float* tokens, const float* target, const uint8_t* mask, float delta, float* loss, int32_t B,
                       int32_t S, int32_t p, int64_t masked, float* partials, void* stream) {
    if (!tokens || !target || !mask || !loss || !partials) return CALM_E_INVAL;
    MimGeom g;
    long n;
    if (int e = mim_huber_args(B, S, p, delta, masked, &g, &n)) return e;
    if (!aligned16(partials) || !aligned4(tokens) || !aligned4(target)) return CALM_E_LAYOUT;
    const float count = (float)(3.0 * (double)p * (double)p * (double)masked);
    const long n4 = aligned16(tokens) && aligned16(target) ? n / 4 : 0;
    const int grid = mim_grid(n);
    if (int e = calm_launch(mim_huber_kernel<false>, grid, NT, 0, stream, tokens, target, mask, delta, nullptr, partials, g,
                            (uint32_t)n, (uint32_t)n4, count))
        return e;
    return calm_launch(huber_rows_final_kernel, 1, NT, 0, stream, partials, grid, 1.0f / count, loss);
}

int calm_mim_huber_bwd(const float* tokens, const float* target, const uint8_t* mask, float delta, const float* dloss,
                       float* dtokens, int32_t B, int32_t S, int32_t p, int64_t masked, void* stream) {
    if (!tokens || !target || !mask || !dloss || !dtokens) return CALM_E_INVAL;
    MimGeom g;
    long n;
    if (int e = mim_huber_args(B, S, p, delta, masked, &g, &n)) return e;
    if (!aligned4(tokens) || !aligned4(target) || !aligned4(dtokens)) return CALM_E_LAYOUT;
    const float count = (float)(3.0 * (double)p * (double)p * (double)masked);
    const long n4 = aligned16(tokens) && aligned16(target) && aligned16(dtokens) ? n / 4 : 0;
    return calm_launch(mim_huber_kernel<true>, mim_grid(n), NT, 0, stream, tokens, target, mask, delta, dloss, dtokens, g,
                       (uint32_t)n, (uint32_t)n4, count);
}

}  // extern "C"
