// Device resized crop (an addition to ABI v7): Image.crop(box).resize((vw, vh), BILINEAR) — torchvision's resized_crop on
// a PIL image — over a ragged batch of HWC uint8 images packed into one byte buffer, per sample a source box and an
// output size, of which only an H x W window is computed; the window comes out as uint8 planar, as the normalised fp32
// image or as the first Block's row tokens.  It is the kernel of resize.hip with the box, the window and the epilogues
// added, and the same arithmetic: integer from the coefficients on, bit equality with the uint8 result of PIL.
//
// The contract is the header's formulas, horizontal pass then vertical pass, with in = bw / bh and out = vw / vh, the
// source indices shifted by bx0 / by0: crop then resize, pixels outside the box are never read (Image.resize(box=) reads
// them and is another function).  PIL itself departs from that pass order on very tall, narrow sources (w = 2 .. 6 with h
// above roughly 100 w, vertically downscaled: it runs the vertical pass first and a few bytes differ); the contract stays
// the formulas, as for calm_resize_u8.
//
// One launch.  A workgroup owns one sample and one 16 x 64 tile of the output window.  It computes the tile's tap bounds
// and weight sums in fp64 (resize_coeffs.h) into LDS for the window's pixels wy0 + y, wx0 + x of the vh x vw result, then
// walks the box's rows the tile needs in chunks of up to 32:
//   horizontal pass: a thread owns one output column and every fourth row of the chunk; it reads its taps straight from
//     the source row — aligned dwords, bytes selected with v_alignbyte — multiplies by the column's coefficients from LDS
//     and writes the rounded uint8 into LDS, planar.  The bytes a thread asks for are those of pixels bx0 + lo ..
//     bx0 + lo + n - 1 of row by0 + y, all inside the box and so inside the image, and only aligned dwords that hold at
//     least one of them are loaded: the guarantee of resize.hip survives the box, also in the last rows and columns of
//     the last image of the buffer;
//   vertical pass: a thread owns four neighbouring pixels of one output row in the three channels and adds the chunk's
//     rows times the row's coefficients into 32-bit integers.
// LDS is bounded whatever the source size (32 rows of intermediate, 32 horizontal taps per column at a time, more taps in
// rounds).  The sizes differ per sample but a workgroup has one sample: the number of chunks and rounds is uniform over
// the workgroup, so every barrier is.  A record that fails calm_rcrop_valid (rcrop_check.h) is tested before any address
// is formed, is never read and gives the output of an all-zero source.
// Epilogue: the twelve values of a thread are 4 pixels x 3 channels — one dword (uint8), one 16-byte store per channel
// (fp32 image) or three 16-byte stores of twelve consecutive floats (tokens) when W % 4 == 0 and the base is aligned,
// scalar stores otherwise.  No atomics; every output element is written once.
// (The tile loop restates resize.hip's, with bw / bh, the box pointer and the window offsets substituted: a fix to one of the
// two loops has to be mirrored in the other.)
#include "common.h"
#include "rcrop_check.h"
#include "resize_coeffs.h"

namespace {

constexpr int NT = 256;
constexpr int TH = 16, TW = 64;                // output pixels of a workgroup
constexpr int CH = 32;                         // source rows per chunk
constexpr int KC = 32;                         // horizontal taps per column held in LDS (a multiple of 4)
constexpr int MAX_SIDE = CALM_RCROP_MAX_SIDE;

struct RcropNorm {
    float mean[3], inv[3];                     // n(v) = fma(v, 1 / 255, -mean) * inv in fp32, inv = 1 / std: the operations
                                               // calm_collate_crop_mix's expression compiles to, written out
};

// PIL's clip8((2^21 + sum) >> 22); the sum arrives without the 2^21
__device__ __forceinline__ uint32_t fix8(uint32_t acc) {
    const int v = (int)(acc + (1u << (CALM_RESIZE_PRECISION_BITS - 1))) >> CALM_RESIZE_PRECISION_BITS;
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

template <int KIND, bool VEC>
__global__ __launch_bounds__(NT) void resized_crop_kernel(const uint8_t* __restrict__ packed, int64_t nbytes,
                                                          const calm_rcrop_sample* __restrict__ samples,
                                                          void* __restrict__ out, int H, int W, const RcropNorm nm) {
    __shared__ uint32_t hbuf[CH * 3 * TW / 4];      // horizontal pass, uint8 [row][channel][column]
    __shared__ int kxs[KC * TW];                    // [tap][column]: a wave reads one tap of 64 columns, 64 banks
    __shared__ int kys[TH * CH];                    // [output row][chunk row], 0 outside the row's taps
    __shared__ double xcen[TW], xww[TW], ycen[TH], yww[TH];
    __shared__ int xlo[TW], xn[TW], ylo[TH], yn[TH];

    const int tid = threadIdx.x, b = blockIdx.z, oy0 = blockIdx.y * TH, ox0 = blockIdx.x * TW;
    const calm_rcrop_sample s = samples[b];
    const bool ok = calm_rcrop_valid(s, nbytes, H, W);              // before any address is formed
    const int w = s.w, bh = ok ? s.bh : 1, bw = ok ? s.bw : 1;
    const CalmResizeAxis ax = calm_resize_axis(bw, ok ? s.vw : 1), ay = calm_resize_axis(bh, ok ? s.vh : 1);

    if (tid < TW) {
        CalmResizeTaps t = {0, 0, 0.0, 0.0};
        if (ok && ox0 + tid < W) t = calm_resize_taps(ax, bw, s.wx0 + ox0 + tid);
        xlo[tid] = t.lo; xn[tid] = t.n; xcen[tid] = t.center; xww[tid] = t.ww;
    } else if (tid < TW + TH) {
        const int i = tid - TW;
        CalmResizeTaps t = {0, 0, 0.0, 0.0};
        if (ok && oy0 + i < H) t = calm_resize_taps(ay, bh, s.wy0 + oy0 + i);
        ylo[i] = t.lo; yn[i] = t.n; ycen[i] = t.center; yww[i] = t.ww;
    }
    __syncthreads();

    const int last = min(TH, H - oy0) - 1;                          // lo and lo + n do not decrease with the row
    const int ybeg = ylo[0], yend = ylo[last] + yn[last];           // rows of the box; none for an invalid record
    const int nxmax = min(ax.kmax, bw);                             // no column has more taps
    // the box's first pixel; the offsets stay zero for an invalid record
    const uint8_t* src = packed + (ok ? s.offset + ((int64_t)s.by0 * w + s.bx0) * 3 : 0);

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
                // bytes [a, a + 3 jn) of box row y0c + r, box columns lo + t0 .. lo + t0 + jn - 1 (lo + n <= bw, y0c + r <
                // bh): only aligned dwords that hold at least one of them are loaded, and taps past jn meet a zero
                // coefficient.  The row stride is the image's, 3 w bytes.
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
    if (oy >= H || ox >= W) return;
    if constexpr (KIND == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint8_t* dst = static_cast<uint8_t*>(out) + (((int64_t)b * 3 + c) * H + oy) * W + ox;
            if (VEC) {                                              // W % 4 == 0 and a 4-byte aligned base
                *reinterpret_cast<uint32_t*>(dst) =
                    fix8(vacc[c][0]) | fix8(vacc[c][1]) << 8 | fix8(vacc[c][2]) << 16 | fix8(vacc[c][3]) << 24;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (ox + k < W) dst[k] = (uint8_t)fix8(vacc[c][k]);
            }
        }
    } else {
        float f[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) f[c][k] = fmaf((float)fix8(vacc[c][k]), 1.0f / 255.0f, -nm.mean[c]) * nm.inv[c];
        if constexpr (KIND == 1) {                                  // [B,3,H,W]
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float* dst = static_cast<float*>(out) + (((int64_t)b * 3 + c) * H + oy) * W + ox;
                if (VEC) {                                          // W % 4 == 0 and a 16-byte aligned base
                    *reinterpret_cast<f32x4*>(dst) = f32x4{f[c][0], f[c][1], f[c][2], f[c][3]};
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (ox + k < W) dst[k] = f[c][k];
                }
            }
        } else {                                                    // row tokens [B,H,3W]: twelve consecutive floats
            float* dst = static_cast<float*>(out) + ((int64_t)b * H + oy) * 3 * W + 3 * ox;
            if (VEC) {
                reinterpret_cast<f32x4*>(dst)[0] = f32x4{f[0][0], f[1][0], f[2][0], f[0][1]};
                reinterpret_cast<f32x4*>(dst)[1] = f32x4{f[1][1], f[2][1], f[0][2], f[1][2]};
                reinterpret_cast<f32x4*>(dst)[2] = f32x4{f[2][2], f[0][3], f[1][3], f[2][3]};
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (ox + k < W) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) dst[3 * k + c] = f[c][k];
                    }
            }
        }
    }
}

}  // namespace

extern "C" {

int calm_resized_crop_check(const calm_rcrop_sample* sample, int64_t nbytes, int32_t H, int32_t W) {
    return sample && calm_rcrop_valid(*sample, nbytes, H, W) ? 1 : 0;
}

int calm_resized_crop(const uint8_t* packed, int64_t nbytes, const calm_rcrop_sample* samples_dev, void* out, int32_t B,
                      int32_t H, int32_t W, int32_t out_kind, const float* mean, const float* std, void* stream) {
    if (!packed || !samples_dev || !out || nbytes <= 0 || B <= 0 || H <= 0 || W <= 0) return CALM_E_INVAL;
    if (out_kind < 0 || out_kind > 2 || (out_kind != 0 && (!mean || !std))) return CALM_E_INVAL;
    if (B > 65535 || H > MAX_SIDE || W > MAX_SIDE) return CALM_E_UNSUPP;        // grid dimension z; the largest side
    RcropNorm nm = {};
    if (out_kind != 0)
        for (int c = 0; c < 3; ++c) { nm.mean[c] = mean[c]; nm.inv[c] = 1.0f / std[c]; }
    const int tiles_y = (H + TH - 1) / TH, tiles_x = (W + TW - 1) / TW;
    const uintptr_t align = out_kind == 0 ? 3u : 15u;               // one dword of pixels, or 16-byte stores of floats
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & align) == 0;
    return with_int<0, 1, 2>(out_kind, [&](auto kind) {
        return with_bool(vec, [&](auto v) {
            return calm_launch(resized_crop_kernel<decltype(kind)::value, decltype(v)::value>, dim3(tiles_x, tiles_y, B),
                               NT, 0, stream, packed, nbytes, samples_dev, out, H, W, nm);
        });
    });
}

}  // extern "C"
