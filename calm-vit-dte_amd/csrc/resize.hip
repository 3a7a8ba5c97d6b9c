// Device resize (an addition to ABI v7): the reference's transforms.Resize((256, 256)) on a PIL image
// (distributed_trainer_cls.py:129), i.e. Image.resize(size, BILINEAR) — antialiased, horizontal pass then vertical pass,
// 22-bit fixed-point coefficients, the intermediate rounded to uint8 — over a ragged batch of HWC uint8 images packed
// into one byte buffer.  Integer arithmetic from the coefficients on: the output equals PIL's byte for byte.
//
// One launch.  A workgroup owns one sample and one 16 x 64 tile of output pixels and runs the tile loop of resize_tile.h
// (the LDS layout, the tap and coefficient fill, both passes, the read guarantee and the barriers are stated there, once,
// for this file and resized_crop.hip); this file reads the record, decides whether it may be read, and stores uint8.
#include "common.h"
#include "pixel_quad.h"
#include "resize_tile.h"

namespace {

constexpr int MAX_SIDE = 16384;

template <bool VEC>
__global__ __launch_bounds__(NT) void resize_u8_kernel(const uint8_t* __restrict__ packed, int64_t nbytes,
                                                       const calm_resize_sample* __restrict__ samples,
                                                       uint8_t* __restrict__ out, int oh, int ow) {
    const int tid = threadIdx.x, b = blockIdx.z, oy0 = blockIdx.y * TH, ox0 = blockIdx.x * TW;
    const calm_resize_sample s = samples[b];
    const int h = s.h, w = s.w;
    // a record that does not describe an image inside the buffer is never read: its output is zeros
    const bool ok = h >= 1 && h <= MAX_SIDE && w >= 1 && w <= MAX_SIDE && s.offset >= 0 && s.offset <= nbytes &&
                    (int64_t)3 * h * w <= nbytes - s.offset;
    // the whole image into (oh, ow): the extent is the image, the window starts at 0
    const ResizeTileGeom geo = {ok, packed + s.offset, w, w, h, calm_resize_axis(ok ? w : 1, ow),
                                calm_resize_axis(ok ? h : 1, oh), 0, 0, oh, ow};
    uint32_t vacc[3][4];
    resize_tile(geo, vacc);

    const int oy = oy0 + (tid >> 4), ox = ox0 + 4 * (tid & 15);
    if (oy >= oh || ox >= ow) return;
    uint32_t q[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) q[c][k] = fix8(vacc[c][k]);
    store_quad_u8<VEC>(out, b, oh, ow, oy, ox, q);
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
