// The stores of a pixel quad, once: in the device input kernels (resize.hip, resized_crop.hip, augment.hip) a thread ends
// with twelve values v[c][k] — channel c of the four neighbouring pixels (y, x + k) of sample b in an H x W output — and
// writes them as uint8 planar [B,3,H,W], fp32 planar [B,3,H,W] or row tokens [B,H,3W].  VEC: W % 4 == 0 and an aligned
// base (4 bytes for uint8, 16 for fp32), so the quad lies inside the row and goes out as whole dwords / 16-byte stores;
// otherwise element by element, the pixels at or past W left out.  The caller has checked y < H and x < W.
// Values only: no device floating-point arithmetic lives here, the normalisations are bit contracts of their kernels
// (and randaugment.hip, which compiles without contraction, must not come to share such code with a contracting file).
#pragma once
#include "common.h"

struct Norm3 { float mean[3], inv[3]; };           // Normalize(mean, std) as a kernel argument, inv = 1 / std

static inline Norm3 norm3(const float* mean, const float* std) {
    Norm3 nm;
    for (int c = 0; c < 3; ++c) { nm.mean[c] = mean[c]; nm.inv[c] = 1.0f / std[c]; }
    return nm;
}

template <bool VEC>
__device__ __forceinline__ void store_quad_u8(uint8_t* out, int b, int H, int W, int y, int x, const uint32_t (&v)[3][4]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {                   // v: bytes, 0 .. 255
        uint8_t* dst = out + (((int64_t)b * 3 + c) * H + y) * W + x;
        if (VEC) {
            *reinterpret_cast<uint32_t*>(dst) = v[c][0] | v[c][1] << 8 | v[c][2] << 16 | v[c][3] << 24;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < W) dst[k] = (uint8_t)v[c][k];
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void store_quad_f32(float* out, int b, int H, int W, int y, int x, const float (&v)[3][4]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* dst = out + (((int64_t)b * 3 + c) * H + y) * W + x;
        if (VEC) {
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = v[c][k];
            *reinterpret_cast<f32x4*>(dst) = o;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < W) dst[k] = v[c][k];
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void store_quad_tokens(float* out, int b, int H, int W, int y, int x, const float (&v)[3][4]) {
    float* dst = out + ((int64_t)b * H + y) * 3 * W + 3 * x;        // out[b, y, 3 x + c]: twelve consecutive floats
    if (VEC) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = v[(4 * q + j) % 3][(4 * q + j) / 3];
            *reinterpret_cast<f32x4*>(dst + 4 * q) = o;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x + k < W) {
                dst[3 * k] = v[0][k]; dst[3 * k + 1] = v[1][k]; dst[3 * k + 2] = v[2][k];
            }
    }
}
