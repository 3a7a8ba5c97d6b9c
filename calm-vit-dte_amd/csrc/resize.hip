// Device resize (an addition to ABI v7): the reference's transforms.Resize((256, 256)) on a PIL image
// (distributed_trainer_cls.py:129), i.e. Image.resize(size, BILINEAR) — antialiased, horizontal pass then vertical pass,
// 22-bit fixed-point coefficients, the intermediate rounded to uint8 — over a ragged batch of HWC uint8 images packed
// into one byte buffer.  Integer arithmetic from the coefficients on: the output equals PIL's byte for byte.
//
// One launch.  A workgroup owns one sample and one 16 x 64 tile of output pixels.  It computes the tile's tap bounds and
// weight sums in fp64 (resize_coeffs.h) into LDS, then walks the source rows the tile needs in chunks of up to 32:
//   horizontal pass: a thread owns one output column and every fourth row of the chunk; it reads its taps straight from
//     the source row — aligned dwords, bytes selected with v_alignbyte, since a row starts at a multiple of 3w bytes —
//     multiplies by the column's coefficients from LDS and writes the rounded uint8 into LDS, planar;
//   vertical pass: a thread owns four neighbouring pixels of one output row in the three channels and adds the chunk's
//     rows times the row's coefficients into 32-bit integers (the sums are associative: any split over chunks is exact).
// LDS is bounded whatever the source size: 32 rows of intermediate, 32 horizontal taps per column at a time (a column
// with more taps — a scale above 15 — goes through them in rounds, the partial sums staying in registers) and the
// vertical coefficients of the 32 rows in flight.  The number of chunks follows from the sample's scale, which is uniform
// over the workgroup, so every barrier is too.
// (resized_crop.hip restates this tile loop with a source box and an output window: a fix here has to be mirrored there.)
#include "common.h"
#include "resize_coeffs.h"

namespace {

constexpr int NT = 256;
constexpr int TH = 16, TW = 64;                // output pixels of a workgroup
constexpr int CH = 32;                         // source rows per chunk
constexpr int KC = 32;                         // horizontal taps per column held in LDS (a multiple of 4)
constexpr int MAX_SIDE = 16384;

// PIL's clip8((2^21 + sum) >> 22); the sum arrives without the 2^21
__device__ __forceinline__ uint32_t fix8(uint32_t acc) {
    const int v = (int)(acc + (1u << (CALM_RESIZE_PRECISION_BITS - 1))) >> CALM_RESIZE_PRECISION_BITS;
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

template <bool VEC>
__global__ __launch_bounds__(NT) void resize_u8_kernel(const uint8_t* __restrict__ packed, int64_t nbytes,
                                                       const calm_resize_sample* __restrict__ samples,
                                                       uint8_t* __restrict__ out, int oh, int ow) {
    __shared__ uint32_t hbuf[CH * 3 * TW / 4];      // horizontal pass, uint8 [row][channel][column]
    __shared__ int kxs[KC * TW];                    // [tap][column]: a wave reads one tap of 64 columns, 64 banks
    __shared__ int kys[TH * CH];                    // [output row][chunk row], 0 outside the row's taps
    __shared__ double xcen[TW], xww[TW], ycen[TH], yww[TH];
    __shared__ int xlo[TW], xn[TW], ylo[TH], yn[TH];

    const int tid = threadIdx.x, b = blockIdx.z, oy0 = blockIdx.y * TH, ox0 = blockIdx.x * TW;
    const calm_resize_sample s = samples[b];
    const int h = s.h, w = s.w;
    // a record that does not describe an image inside the buffer is never read: its output is zeros
    const bool ok = h >= 1 && h <= MAX_SIDE && w >= 1 && w <= MAX_SIDE && s.offset >= 0 && s.offset <= nbytes &&
                    (int64_t)3 * h * w <= nbytes - s.offset;
    const CalmResizeAxis ax = calm_resize_axis(ok ? w : 1, ow), ay = calm_resize_axis(ok ? h : 1, oh);

    if (tid < TW) {
        CalmResizeTaps t = {0, 0, 0.0, 0.0};
        if (ok && ox0 + tid < ow) t = calm_resize_taps(ax, w, ox0 + tid);
        xlo[tid] = t.lo; xn[tid] = t.n; xcen[tid] = t.center; xww[tid] = t.ww;
    } else if (tid < TW + TH) {
        const int i = tid - TW;
        CalmResizeTaps t = {0, 0, 0.0, 0.0};
        if (ok && oy0 + i < oh) t = calm_resize_taps(ay, h, oy0 + i);
        ylo[i] = t.lo; yn[i] = t.n; ycen[i] = t.center; yww[i] = t.ww;
    }
    __syncthreads();

    const int last = min(TH, oh - oy0) - 1;                         // lo and lo + n do not decrease with the row
    const int ybeg = ylo[0], yend = ylo[last] + yn[last];
    const int nxmax = min(ax.kmax, w);                              // no column has more taps
    const uint8_t* src = packed + s.offset;

    const int hx = tid & 63, hr = tid >> 6;                         // horizontal pass: column, first row
    const int lo = xlo[hx], n = xn[hx];
    const int vy = tid >> 4, vq = tid & 15;                         // vertical pass: row, group of 4 columns
    const int my_ylo = ylo[vy], my_yn = yn[vy];
    uint32_t vacc[3][4] = {};
    int loaded = -1;                                                // first tap of the coefficients in kxs

    for (int y0c = ybeg; y0c < yend; y0c += CH) {
        const int rows = min(CH, yend - y0c);
        for (int e = tid; e < TH * CH; e += NT) {
            const int i = e / CH, j = y0c + (e % CH) - ylo[i];
            int k = 0;
            if (j >= 0 && j < yn[i]) {
                const CalmResizeTaps t = {ylo[i], yn[i], ycen[i], yww[i]};
                k = calm_resize_k(ay, t, j);
            }
            kys[e] = k;
        }

        uint32_t hacc[CH / 4][3] = {};
        for (int t0 = 0; t0 < nxmax; t0 += KC) {
            if (t0 != loaded) {
                __syncthreads();
                const int kfill = min(KC, (nxmax - t0 + 3) & ~3);   // whole groups of 4 taps, zeros past a column's n
                for (int e = tid; e < kfill * TW; e += NT) {
                    const int j = t0 + e / TW, x = e % TW;
                    int k = 0;
                    if (j < xn[x]) {
                        const CalmResizeTaps t = {xlo[x], xn[x], xcen[x], xww[x]};
                        k = calm_resize_k(ax, t, j);
                    }
                    kxs[e] = k;
                }
                __syncthreads();
                loaded = t0;
            }
            const int jn = min(KC, n - t0);                         // this column's taps of the round
            if (jn <= 0) continue;
#pragma unroll
            for (int i = 0; i < CH / 4; ++i) {
                const int r = hr + 4 * i;
                if (r >= rows) continue;
                // bytes [a, a + 3 jn) of the row: only aligned dwords that hold at least one of them are loaded (such a
                // dword lies in the page of a byte of the image), and taps past jn meet a zero coefficient
                const uintptr_t a = reinterpret_cast<uintptr_t>(src + ((int64_t)(y0c + r) * w + lo + t0) * 3);
                const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
                const uint32_t sh = (uint32_t)(a & 3);
                const int nd = ((int)sh + 3 * jn + 3) >> 2;
                uint32_t d0 = q[0];
                for (int j = 0, g = 0; j < jn; j += 4, g += 3) {
                    const uint32_t d1 = g + 1 < nd ? q[g + 1] : 0u, d2 = g + 2 < nd ? q[g + 2] : 0u,
                                   d3 = g + 3 < nd ? q[g + 3] : 0u;
                    const uint32_t u0 = __builtin_amdgcn_alignbyte(d1, d0, sh);      // R0 G0 B0 R1
                    const uint32_t u1 = __builtin_amdgcn_alignbyte(d2, d1, sh);      // G1 B1 R2 G2
                    const uint32_t u2 = __builtin_amdgcn_alignbyte(d3, d2, sh);      // B2 R3 G3 B3
                    const uint32_t k0 = kxs[j * TW + hx], k1 = kxs[(j + 1) * TW + hx], k2 = kxs[(j + 2) * TW + hx],
                                   k3 = kxs[(j + 3) * TW + hx];
                    hacc[i][0] += __umul24(u0 & 255u, k0) + __umul24(u0 >> 24, k1) + __umul24((u1 >> 16) & 255u, k2) +
                                  __umul24((u2 >> 8) & 255u, k3);
                    hacc[i][1] += __umul24((u0 >> 8) & 255u, k0) + __umul24(u1 & 255u, k1) + __umul24(u1 >> 24, k2) +
                                  __umul24((u2 >> 16) & 255u, k3);
                    hacc[i][2] += __umul24((u0 >> 16) & 255u, k0) + __umul24((u1 >> 8) & 255u, k1) +
                                  __umul24(u2 & 255u, k2) + __umul24(u2 >> 24, k3);
                    d0 = d3;
                }
            }
        }
        uint8_t* hb = reinterpret_cast<uint8_t*>(hbuf);
#pragma unroll
        for (int i = 0; i < CH / 4; ++i) {
            const int r = hr + 4 * i;
            if (r < rows) {
#pragma unroll
                for (int c = 0; c < 3; ++c) hb[(r * 3 + c) * TW + hx] = (uint8_t)fix8(hacc[i][c]);
            }
        }
        __syncthreads();

        const int r0 = max(my_ylo - y0c, 0), r1 = min(my_ylo + my_yn - y0c, rows);
        for (int r = r0; r < r1; ++r) {
            const uint32_t ky = kys[vy * CH + r];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t v = hbuf[(r * 3 + c) * (TW / 4) + vq];
#pragma unroll
                for (int k = 0; k < 4; ++k) vacc[c][k] += __umul24((v >> (8 * k)) & 255u, ky);
            }
        }
        __syncthreads();                                            // the next chunk overwrites hbuf and kys
    }

    const int oy = oy0 + vy, ox = ox0 + 4 * vq;
    if (oy >= oh || ox >= ow) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        uint8_t* dst = out + (((int64_t)b * 3 + c) * oh + oy) * ow + ox;
        if (VEC) {                                                  // ow % 4 == 0 and a 4-byte aligned base
            *reinterpret_cast<uint32_t*>(dst) =
                fix8(vacc[c][0]) | fix8(vacc[c][1]) << 8 | fix8(vacc[c][2]) << 16 | fix8(vacc[c][3]) << 24;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ox + k < ow) dst[k] = (uint8_t)fix8(vacc[c][k]);
        }
    }
}

}  // namespace

extern "C" {

int calm_resize_coeffs(int32_t in, int32_t out, int32_t* bounds, int32_t* kk, int32_t ksize) {
    if (!bounds || !kk || in <= 0 || out <= 0 || ksize <= 0) return CALM_E_INVAL;
    if (in > MAX_SIDE || out > MAX_SIDE) return CALM_E_UNSUPP;
    const CalmResizeAxis a = calm_resize_axis(in, out);
    if (ksize < a.kmax) {                                           // a smaller row is fine when every pixel fits it
        for (int o = 0; o < out; ++o)
            if (calm_resize_taps(a, in, o).n > ksize) return CALM_E_INVAL;
    }
    for (int o = 0; o < out; ++o) {
        const CalmResizeTaps t = calm_resize_taps(a, in, o);
        bounds[2 * o] = t.lo;
        bounds[2 * o + 1] = t.n;
        int32_t* k = kk + (int64_t)o * ksize;
        for (int j = 0; j < ksize; ++j) k[j] = j < t.n ? calm_resize_k(a, t, j) : 0;
    }
    return 0;
}

int calm_resize_u8(const uint8_t* packed, int64_t nbytes, const calm_resize_sample* samples_dev, uint8_t* out, int32_t B,
                   int32_t oh, int32_t ow, void* stream) {
    if (!packed || !samples_dev || !out || nbytes <= 0 || B <= 0 || oh <= 0 || ow <= 0) return CALM_E_INVAL;
    if (B > 65535 || oh > MAX_SIDE || ow > MAX_SIDE) return CALM_E_UNSUPP;      // grid dimension z; the largest side
    const int tiles_y = (oh + TH - 1) / TH, tiles_x = (ow + TW - 1) / TW;
    const bool vec = ow % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
    return with_bool(vec, [&](auto v) {
        return calm_launch(resize_u8_kernel<decltype(v)::value>, dim3(tiles_x, tiles_y, B), NT, 0, stream, packed, nbytes,
                           samples_dev, out, oh, ow);
    });
}

}  // extern "C"
