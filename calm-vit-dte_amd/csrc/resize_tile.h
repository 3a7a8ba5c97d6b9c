// The tile loop of the PIL-exact antialiased bilinear resize, once: resize.hip (the whole image into oh x ow) and
// resized_crop.hip (a source box into an H x W window of a vh x vw result) both run it and differ in how they read
// their record, decide `ok` and store the result.
//
// A workgroup of NT threads owns one sample and one TH x TW tile of output pixels.  It computes the tile's tap bounds and
// weight sums in fp64 (resize_coeffs.h) into LDS for the output pixels wy0 + y, wx0 + x, then walks the source rows the
// tile needs in chunks of up to CH:
//   horizontal pass: a thread owns one output column and every fourth row of the chunk; it reads its taps straight from
//     the source row — aligned dwords, bytes selected with v_alignbyte, since a row starts at a multiple of 3w bytes —
//     multiplies by the column's coefficients from LDS and writes the rounded uint8 into LDS, planar;
//   vertical pass: a thread owns four neighbouring pixels of one output row in the three channels and adds the chunk's
//     rows times the row's coefficients into 32-bit integers (the sums are associative: any split over chunks is exact).
// LDS is bounded whatever the source size: CH rows of intermediate, KC horizontal taps per column at a time (a column
// with more taps — a scale above 15 — goes through them in rounds, the partial sums staying in registers) and the
// vertical coefficients of the CH rows in flight.
//
// What is read.  `src` points at the first pixel of the source extent (the image, or the box inside it), rows are 3 w
// bytes apart.  A thread asks for the bytes of pixels lo .. lo + n - 1 of row y with lo + n <= bw and y < bh (the taps of
// resize_coeffs.h end at `in`), all inside the extent and so inside the image, and only aligned dwords that hold at least
// one of those bytes are loaded: such a dword lies in the page of a byte of the image, also in the last rows and columns
// of the last image of the buffer.  The bytes of such a dword that belong to no tap meet a zero coefficient or are
// shifted out.  With ok = false every pixel gets n = 0 taps: there are no rows to walk, nothing is read (src is not
// dereferenced) and vacc stays zero.
//
// Barriers.  A workgroup has one sample: the rows ybeg .. yend, the number of chunks and the number of coefficient rounds
// (nxmax) are the same for all of its threads, so every __syncthreads() below is reached by all of them; the per-thread
// conditions (a column's own n, a row past the chunk) only skip arithmetic between barriers.
#pragma once
#include "common.h"
#include "resize_coeffs.h"

namespace {

constexpr int NT = 256;
constexpr int TH = 16, TW = 64;                // output pixels of a workgroup
constexpr int CH = 32;                         // source rows per chunk
constexpr int KC = 32;                         // horizontal taps per column held in LDS (a multiple of 4)

// PIL's clip8((2^21 + sum) >> 22); the sum arrives without the 2^21
__device__ __forceinline__ uint32_t fix8(uint32_t acc) {
    const int v = (int)(acc + (1u << (CALM_RESIZE_PRECISION_BITS - 1))) >> CALM_RESIZE_PRECISION_BITS;
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

struct ResizeTileGeom {
    bool ok;                                   // false: no taps, nothing read, zeros
    const uint8_t* src;                        // first pixel of the source extent
    int w;                                     // pixels per image row (the row stride is 3 w bytes)
    int bw, bh;                                // the source extent: the `in` of the two axes
    CalmResizeAxis ax, ay;
    int wx0, wy0;                              // the tile's pixels are wx0 + x, wy0 + y of the axes' `out`
    int H, W;                                  // output extent: pixels at or past it are not computed
};

// vacc[c][k]: the 22-bit fixed-point sum (fix8 rounds it) of channel c of output pixel (blockIdx.y * TH + (tid >> 4),
// blockIdx.x * TW + 4 * (tid & 15) + k)
__device__ __forceinline__ void resize_tile(const ResizeTileGeom& geo, uint32_t (&vacc)[3][4]) {
    __shared__ uint32_t hbuf[CH * 3 * TW / 4];      // horizontal pass, uint8 [row][channel][column]
    __shared__ int kxs[KC * TW];                    // [tap][column]: a wave reads one tap of 64 columns, 64 banks
    __shared__ int kys[TH * CH];                    // [output row][chunk row], 0 outside the row's taps
    __shared__ double xcen[TW], xww[TW], ycen[TH], yww[TH];
    __shared__ int xlo[TW], xn[TW], ylo[TH], yn[TH];

    const int tid = threadIdx.x, oy0 = blockIdx.y * TH, ox0 = blockIdx.x * TW;
    // the geometry is read once and the sums are kept in a local array: the compiler simplifies this function before it
    // inlines it, when geo and vacc are still memory (reading the fields in place costs some 50 instructions per kernel)
    const bool ok = geo.ok;
    const uint8_t* src = geo.src;
    const int w = geo.w, bw = geo.bw, bh = geo.bh, wx0 = geo.wx0, wy0 = geo.wy0, H = geo.H, W = geo.W;
    const CalmResizeAxis ax = geo.ax, ay = geo.ay;

    if (tid < TW) {
        CalmResizeTaps t = {0, 0, 0.0, 0.0};
        if (ok && ox0 + tid < W) t = calm_resize_taps(ax, bw, wx0 + ox0 + tid);
        xlo[tid] = t.lo; xn[tid] = t.n; xcen[tid] = t.center; xww[tid] = t.ww;
    } else if (tid < TW + TH) {
        const int i = tid - TW;
        CalmResizeTaps t = {0, 0, 0.0, 0.0};
        if (ok && oy0 + i < H) t = calm_resize_taps(ay, bh, wy0 + oy0 + i);
        ylo[i] = t.lo; yn[i] = t.n; ycen[i] = t.center; yww[i] = t.ww;
    }
    __syncthreads();

    const int last = min(TH, H - oy0) - 1;                          // lo and lo + n do not decrease with the row
    const int ybeg = ylo[0], yend = ylo[last] + yn[last];           // rows of the extent; none when !ok
    const int nxmax = min(ax.kmax, bw);                             // no column has more taps

    const int hx = tid & 63, hr = tid >> 6;                         // horizontal pass: column, first row
    const int lo = xlo[hx], n = xn[hx];
    const int vy = tid >> 4, vq = tid & 15;                         // vertical pass: row, group of 4 columns
    const int my_ylo = ylo[vy], my_yn = yn[vy];
    uint32_t acc[3][4] = {};
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
                // bytes [a, a + 3 jn) of row y0c + r, columns lo + t0 .. lo + t0 + jn - 1 of the extent: the dwords q[0 ..
                // nd) are those that hold at least one of them, and taps past jn meet a zero coefficient
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
                for (int k = 0; k < 4; ++k) acc[c][k] += __umul24((v >> (8 * k)) & 255u, ky);
            }
        }
        __syncthreads();                                            // the next chunk overwrites hbuf and kys
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) vacc[c][k] = acc[c][k];
}

}  // namespace
