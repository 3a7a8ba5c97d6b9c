// Device RandAugment (an addition to ABI v7): a uint8 -> uint8 stage in front of the collate.  Per sample the crop window
// and the flip, then a chain of up to CALM_RA_MAX_OPS operations, every one rounded to uint8 exactly as PIL rounds it; the
// contract — formulas, rounding, what a malformed record does — is the header's.
//
// Launches, all on the caller's stream:
//   for slot k = 0 .. n_slots - 1
//     when bit k of stats_mask is set: a memset of the histograms, then ra_stats_kernel — (chunks x B) workgroups; the
//       workgroups of a sample whose slot k is not CONTRAST / AUTOCONTRAST / EQUALIZE return at once, the others count R, G,
//       B and L of 4096 pixels into LDS and add the non-zero bins to the sample's four global histograms with integer
//       atomics: the sums do not depend on the order, so the stage repeats bit for bit;
//     ra_apply_kernel — (tiles x B) workgroups of 256 threads, a thread owns four neighbouring pixels of a row in the
//       three channels, four times.  It reads the previous image (slot 0: the source through crop and flip) and writes the
//       next: the two ping-pong images of the scratch, and `out` in the last slot.  The workgroup first turns its sample's
//       histograms into what the operation needs: the contrast mean (a 64-bit integer sum over the L bins), or the
//       3 x 256 look-up table in LDS (a block-wide integer prefix sum for EQUALIZE, fp64 without contraction for
//       AUTOCONTRAST).  The warps gather and SHARPNESS reads its neighbours from the previous image: nothing is staged
//       across launches except the image and the histograms.
//   n_slots == 0: one ra_apply_kernel launch that only crops and flips.
// A sample with fewer operations than n_slots is copied through the remaining slots.
// Addresses: a source pixel (c, y, x) is formed only from 0 <= y < H, 0 <= x < W and a corner clamped into the source; a
// gathered pixel only after its bounds test; a histogram bin only from a uint8; the look-up tables from a uint8.  The
// record supplies no other index.
#include "common.h"

// Every floating-point operation below is one IEEE operation in the order written: a fused multiply-add would skip the
// rounding of the product that PIL's (and Python's) arithmetic makes.  The operators are written out — the __fmul_rn family
// is defined in a header in front of this pragma and would be contracted.
#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int ITER = 4;                        // groups of four pixels per thread of the apply kernel
constexpr int STAT_PX = 4096;                  // pixels per workgroup of the statistics kernel
constexpr int MAX_SIDE = CALM_RA_MAX_SIDE;

struct RaFill { uint8_t v[4]; };

// the image a slot reads: the source batch with the sample's window inside, or a ping-pong image (window == image)
struct RaSrc {
    const uint8_t* p;                          // pixel (0, 0) of channel 0 of the window
    int64_t chs;                               // channel stride
    int rs;                                    // row stride
    int flip, W;
    __device__ __forceinline__ uint32_t px(int c, int y, int x) const {
        return p[c * chs + (int64_t)y * rs + (flip ? W - 1 - x : x)];
    }
};

__device__ __forceinline__ RaSrc ra_source(const uint8_t* src, int Hs, int Ws, int first, const calm_ra_sample* s, int b, int H,
                                           int W) {
    RaSrc r;
    if (first) {
        const int y0 = clampi(s->y0, 0, Hs - H), x0 = clampi(s->x0, 0, Ws - W);
        r.chs = (int64_t)Hs * Ws;
        r.rs = Ws;
        r.p = src + (int64_t)b * 3 * r.chs + (int64_t)y0 * Ws + x0;
        r.flip = s->flip != 0;
    } else {
        r.chs = (int64_t)H * W;
        r.rs = W;
        r.p = src + (int64_t)b * 3 * r.chs;
        r.flip = 0;
    }
    r.W = W;
    return r;
}

__device__ __forceinline__ int ra_slot_op(const calm_ra_sample* s, int slot, int n_slots) {
    const int n = clampi(s->n_ops, 0, n_slots);
    return slot < n ? s->op[slot] : (int)CALM_RA_OP_IDENTITY;
}
__device__ __forceinline__ bool ra_needs_stats(int op) {
    return op == CALM_RA_OP_CONTRAST || op == CALM_RA_OP_AUTOCONTRAST || op == CALM_RA_OP_EQUALIZE;
}

__device__ __forceinline__ uint32_t luma(uint32_t r, uint32_t g, uint32_t b) {
    return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16;
}

// Image.blend: t = d + f (s - d) in fp32, three roundings
__device__ __forceinline__ uint32_t blend(float d, float s, float f) {
    const float t = d + f * (s - d);                                 // (contraction is off in this file)
    if (f >= 0.0f && f <= 1.0f) return (uint32_t)(int)t & 255u;
    return t <= 0.0f ? 0u : t >= 255.0f ? 255u : (uint32_t)(int)t;
}

__global__ __launch_bounds__(NT) void ra_stats_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, int first,
                                                      const calm_ra_sample* __restrict__ samples, int* __restrict__ hist,
                                                      int H, int W, int slot, int n_slots) {
    __shared__ int h[4 * 256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const calm_ra_sample* s = samples + b;
    if (!ra_needs_stats(ra_slot_op(s, slot, n_slots))) return;      // uniform over the workgroup
    for (int i = tid; i < 4 * 256; i += NT) h[i] = 0;
    __syncthreads();
    const RaSrc im = ra_source(src, Hs, Ws, first, s, b, H, W);
    const int n = H * W, p0 = blockIdx.x * STAT_PX, p1 = min(p0 + STAT_PX, n);
    for (int p = p0 + tid; p < p1; p += NT) {
        const int y = p / W, x = p - y * W;
        const uint32_t r = im.px(0, y, x), g = im.px(1, y, x), bl = im.px(2, y, x);
        atomicAdd(&h[r], 1);
        atomicAdd(&h[256 + g], 1);
        atomicAdd(&h[512 + bl], 1);
        atomicAdd(&h[768 + luma(r, g, bl)], 1);
    }
    __syncthreads();
    int* out = hist + (int64_t)b * 1024;
    for (int i = tid; i < 4 * 256; i += NT)
        if (h[i]) atomicAdd(&out[i], h[i]);
}

// exclusive prefix sum of one value per thread over the 256 threads; red: 4 ints of LDS
__device__ __forceinline__ int block_excl_scan_256(int v, int* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) red[w] = inc;
    __syncthreads();
    int base = 0;
    for (int i = 0; i < w; ++i) base += red[i];
    return base + inc - v;
}

template <bool VEC>
__global__ __launch_bounds__(NT) void ra_apply_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, int first,
                                                      const calm_ra_sample* __restrict__ samples,
                                                      const int* __restrict__ hist, uint8_t* __restrict__ dst, int H, int W,
                                                      int slot, int n_slots, int has_stats, const RaFill fill) {
    __shared__ uint8_t lut[3][256];
    __shared__ int red[4], s_lo[3], s_hi[3], s_cnt[3];
    __shared__ unsigned long long s_sum;

    const int b = blockIdx.y, tid = threadIdx.x;
    const calm_ra_sample* s = samples + b;
    int op = ra_slot_op(s, slot, n_slots);
    if (op < 0 || op > CALM_RA_OP_EQUALIZE || (ra_needs_stats(op) && !has_stats)) op = CALM_RA_OP_IDENTITY;
    const float f = s->factor[slot < CALM_RA_MAX_OPS ? slot : 0];
    const int param = s->param[slot < CALM_RA_MAX_OPS ? slot : 0];
    const int* cf = s->coef[slot < CALM_RA_MAX_OPS ? slot : 0];
    const uint32_t A0 = (uint32_t)cf[0], A1 = (uint32_t)cf[1], A2 = (uint32_t)cf[2], A3 = (uint32_t)cf[3], A4 = (uint32_t)cf[4],
                   A5 = (uint32_t)cf[5];
    const RaSrc im = ra_source(src, Hs, Ws, first, s, b, H, W);

    float cmean = 0.0f;
    if (op == CALM_RA_OP_CONTRAST) {                                 // m = floor((2 sum L + n) / (2 n))
        if (tid == 0) s_sum = 0ull;
        __syncthreads();
        const unsigned long long part = (unsigned long long)tid * (unsigned long long)(uint32_t)hist[(int64_t)b * 1024 + 768 + tid];
        if (part) atomicAdd(&s_sum, part);
        __syncthreads();
        const unsigned long long n = (unsigned long long)H * W;
        cmean = (float)(int)((2ull * s_sum + n) / (2ull * n));
    } else if (op == CALM_RA_OP_AUTOCONTRAST || op == CALM_RA_OP_EQUALIZE) {
        if (tid < 3) { s_lo[tid] = 255; s_hi[tid] = 0; s_cnt[tid] = 0; }
        __syncthreads();
        int hv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            hv[c] = hist[(int64_t)b * 1024 + c * 256 + tid];
            if (hv[c] != 0) {
                atomicMin(&s_lo[c], tid);
                atomicMax(&s_hi[c], tid);
                atomicAdd(&s_cnt[c], 1);
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int v = tid;
            if (op == CALM_RA_OP_AUTOCONTRAST) {
                const int lo = s_lo[c], hi = s_hi[c];
                if (hi > lo) {
                    const double scale = 255.0 / (double)(hi - lo);
                    const double off = -(double)lo * scale;
                    v = clampi((int)((double)tid * scale + off), 0, 255);
                }
            } else {
                const int before = block_excl_scan_256(hv[c], red);          // every thread takes part
                if (s_cnt[c] >= 2) {                                         // (the histogram sums to H W)
                    const int hlast = hist[(int64_t)b * 1024 + c * 256 + s_hi[c]];
                    const int step = (H * W - hlast) / 255;
                    if (step != 0) v = min((step / 2 + before) / step, 255);
                }
            }
            lut[c][tid] = (uint8_t)v;
        }
        __syncthreads();
    }

    const int G = (W + 3) >> 2, ngroups = H * G;
    const bool small = H < 3 || W < 3;
    const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
#pragma unroll 1
    for (int it = 0; it < ITER; ++it) {
        const int g = (blockIdx.x * ITER + it) * NT + tid;
        if (g >= ngroups) break;
        const int y = g / G, x0 = (g - y * G) * 4;
        uint32_t v[3][4], o[3][4];
        if (op != CALM_RA_OP_AFFINE) {
            if (VEC && !first) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t d = *reinterpret_cast<const uint32_t*>(im.p + c * im.chs + (int64_t)y * W + x0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[c][j] = (d >> (8 * j)) & 255u;
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[c][j] = x0 + j < W ? im.px(c, y, x0 + j) : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j;
            if (x >= W) { o[0][j] = o[1][j] = o[2][j] = 0u; continue; }
            switch (op) {
            case CALM_RA_OP_AFFINE: {
                const int xin = (int)(A2 + A1 * (uint32_t)y + A0 * (uint32_t)x) >> 16;
                const int yin = (int)(A5 + A4 * (uint32_t)y + A3 * (uint32_t)x) >> 16;
                const bool in = xin >= 0 && xin < W && yin >= 0 && yin < H;
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c][j] = in ? im.px(c, yin, xin) : (uint32_t)fill.v[c];
                break;
            }
            case CALM_RA_OP_BRIGHTNESS:
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c][j] = blend(0.0f, (float)v[c][j], f);
                break;
            case CALM_RA_OP_COLOR: {
                const float L = (float)luma(v[0][j], v[1][j], v[2][j]);
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c][j] = blend(L, (float)v[c][j], f);
                break;
            }
            case CALM_RA_OP_CONTRAST:
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c][j] = blend(cmean, (float)v[c][j], f);
                break;
            case CALM_RA_OP_SHARPNESS: {
                const bool interior = !small && y >= 1 && y <= H - 2 && x >= 1 && x <= W - 2;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float sm = (float)v[c][j];
                    if (interior) {
                        float acc = 0.5f;
#pragma unroll
                        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                            for (int dx = -1; dx <= 1; ++dx)
                                acc = acc + (float)im.px(c, y + dy, x + dx) * (dy == 0 && dx == 0 ? k5 : k1);
                        sm = (float)clampi((int)acc, 0, 255);
                    }
                    o[c][j] = blend(sm, (float)v[c][j], f);
                }
                break;
            }
            case CALM_RA_OP_POSTERIZE: {
                const int bits = param < 0 || param > 8 ? 8 : param;
                const uint32_t mask = (0xFFu << (8 - bits)) & 0xFFu;
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c][j] = v[c][j] & mask;
                break;
            }
            case CALM_RA_OP_SOLARIZE:
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c][j] = (int)v[c][j] < param ? v[c][j] : 255u - v[c][j];
                break;
            case CALM_RA_OP_AUTOCONTRAST:
            case CALM_RA_OP_EQUALIZE:
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c][j] = lut[c][v[c][j]];
                break;
            default:
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c][j] = v[c][j];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint8_t* q = dst + (((int64_t)b * 3 + c) * H + y) * W + x0;
            if (VEC) {                                              // W % 4 == 0 and 4-byte aligned images
                *reinterpret_cast<uint32_t*>(q) = o[c][0] | o[c][1] << 8 | o[c][2] << 16 | o[c][3] << 24;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x0 + j < W) q[j] = (uint8_t)o[c][j];
            }
        }
    }
}

inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

int ra_check_shape(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return CALM_E_INVAL;
    if (B > 65535 || H > MAX_SIDE || W > MAX_SIDE) return CALM_E_UNSUPP;       // grid dimension y; 32-bit warp arithmetic
    return 0;
}

}  // namespace

extern "C" {

int64_t calm_randaugment_scratch_bytes(int32_t B, int32_t H, int32_t W) {
    const int rc = ra_check_shape(B, H, W);
    if (rc != 0) return rc;
    return (int64_t)B * 1024 * sizeof(int32_t) + 2 * align16((int64_t)B * 3 * H * W);
}

int calm_randaugment_u8(const uint8_t* img_u8, int32_t Hs, int32_t Ws, const calm_ra_sample* samples_dev, uint8_t* out,
                        int32_t B, int32_t H, int32_t W, int32_t n_slots, uint32_t stats_mask, const uint8_t* fill,
                        void* scratch, int64_t scratch_bytes, void* stream) {
    if (!img_u8 || !samples_dev || !out || !scratch) return CALM_E_INVAL;
    const int rc = ra_check_shape(B, H, W);
    if (rc == CALM_E_INVAL) return rc;
    if (H > Hs || W > Ws || n_slots < 0 || n_slots > CALM_RA_MAX_OPS) return CALM_E_INVAL;
    if (rc != 0) return rc;
    if (scratch_bytes < calm_randaugment_scratch_bytes(B, H, W) || (reinterpret_cast<uintptr_t>(scratch) & 15u) != 0)
        return CALM_E_INVAL;
    RaFill fl = {};
    if (fill)
        for (int c = 0; c < 3; ++c) fl.v[c] = fill[c];
    const int64_t img_bytes = align16((int64_t)B * 3 * H * W), hist_bytes = (int64_t)B * 1024 * sizeof(int32_t);
    int* hist = static_cast<int*>(scratch);
    uint8_t* buf[2] = {static_cast<uint8_t*>(scratch) + hist_bytes, static_cast<uint8_t*>(scratch) + hist_bytes + img_bytes};
    const int groups = H * ((W + 3) / 4);
    const dim3 grid((groups + NT * ITER - 1) / (NT * ITER), B), sgrid((H * W + STAT_PX - 1) / STAT_PX, B);
    // a dword of four pixels: every row of every image then starts at a multiple of 4 (the scratch images do, 16-byte aligned)
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
    const int passes = n_slots > 0 ? n_slots : 1;
    for (int k = 0; k < passes; ++k) {
        const uint8_t* src = k == 0 ? img_u8 : buf[(k - 1) & 1];
        uint8_t* dst = k == passes - 1 ? out : buf[k & 1];
        const int first = k == 0, sh = k == 0 ? Hs : H, sw = k == 0 ? Ws : W;
        const int has_stats = n_slots > 0 && ((stats_mask >> k) & 1u);
        if (has_stats) {
            const hipError_t e = hipMemsetAsync(hist, 0, hist_bytes, as_stream(stream));
            if (e != hipSuccess) return (int)e;
            const int r = calm_launch(ra_stats_kernel, sgrid, NT, 0, stream, src, sh, sw, first, samples_dev, hist, H, W, k, n_slots);
            if (r != 0) return r;
        }
        const int r = with_bool(vec, [&](auto v) {
            return calm_launch(ra_apply_kernel<decltype(v)::value>, grid, NT, 0, stream, src, sh, sw, first, samples_dev, hist,
                               dst, H, W, k, n_slots, has_stats, fl);
        });
        if (r != 0) return r;
    }
    return 0;
}

}  // extern "C"
