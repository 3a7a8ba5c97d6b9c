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
// One launch.  A workgroup owns one sample and one 16 x 64 tile of the output window and runs the tile loop of
// resize_tile.h (shared with resize.hip; the LDS layout, both passes, the read guarantee and the barriers are stated
// there) with the box as the source extent — the bytes a thread asks for are those of pixels bx0 + lo .. bx0 + lo + n - 1
// of row by0 + y, all inside the box and so inside the image — and wy0, wx0 as the window's origin in the vh x vw result.
// A record that fails calm_rcrop_valid (rcrop_check.h) is tested before any address is formed, is never read and gives
// the output of an all-zero source.
// Epilogue: the twelve values of a thread are 4 pixels x 3 channels, stored by pixel_quad.h — one dword (uint8), one
// 16-byte store per channel (fp32 image) or three 16-byte stores of twelve consecutive floats (tokens) when W % 4 == 0
// and the base is aligned, scalar stores otherwise.  No atomics; every output element is written once.
#include "common.h"
#include "pixel_quad.h"
#include "rcrop_check.h"
#include "resize_tile.h"

namespace {

constexpr int MAX_SIDE = CALM_RCROP_MAX_SIDE;

// nm: n(v) = fma(v, 1 / 255, -mean) * inv in fp32, inv = 1 / std: the operations calm_collate_crop_mix's expression
// compiles to, written out
template <int KIND, bool VEC>
__global__ __launch_bounds__(NT) void resized_crop_kernel(const uint8_t* __restrict__ packed, int64_t nbytes,
                                                          const calm_rcrop_sample* __restrict__ samples,
                                                          void* __restrict__ out, int H, int W, const Norm3 nm) {
    const int tid = threadIdx.x, b = blockIdx.z, oy0 = blockIdx.y * TH, ox0 = blockIdx.x * TW;
    const calm_rcrop_sample s = samples[b];
    const bool ok = calm_rcrop_valid(s, nbytes, H, W);              // before any address is formed
    const int w = s.w, bh = ok ? s.bh : 1, bw = ok ? s.bw : 1;
    // the box's first pixel (the offsets stay zero for an invalid record), the box as the extent, the window's origin
    const ResizeTileGeom geo = {ok, packed + (ok ? s.offset + ((int64_t)s.by0 * w + s.bx0) * 3 : 0), w, bw, bh,
                                calm_resize_axis(bw, ok ? s.vw : 1), calm_resize_axis(bh, ok ? s.vh : 1), s.wx0, s.wy0,
                                H, W};
    uint32_t vacc[3][4];
    resize_tile(geo, vacc);

    const int oy = oy0 + (tid >> 4), ox = ox0 + 4 * (tid & 15);
    if (oy >= H || ox >= W) return;
    if constexpr (KIND == 0) {
        uint32_t q[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) q[c][k] = fix8(vacc[c][k]);
        store_quad_u8<VEC>(static_cast<uint8_t*>(out), b, H, W, oy, ox, q);
    } else {
        float f[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) f[c][k] = fmaf((float)fix8(vacc[c][k]), 1.0f / 255.0f, -nm.mean[c]) * nm.inv[c];
        if constexpr (KIND == 1) store_quad_f32<VEC>(static_cast<float*>(out), b, H, W, oy, ox, f);
        else store_quad_tokens<VEC>(static_cast<float*>(out), b, H, W, oy, ox, f);
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
    const Norm3 nm = out_kind != 0 ? norm3(mean, std) : Norm3{};
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
