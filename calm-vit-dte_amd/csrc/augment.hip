// Device-side photometric augmentation fused into the batch collate (an addition to ABI v7): the per-pixel half of the
// reference's transform list (distributed_trainer_cls.py:130-138) — RandomCrop, ColorJitter, RandomSolarize,
// RandomHorizontalFlip, RandomGrayscale, GaussianBlur(3), ToDtype(scale), Normalize — and the batch-level CutMix / MixUp
// of cls:58-61 in one pass over the uint8 batch.  Everything is fp32 on [0, 1] from v = u8 / 255 on: nothing is
// quantised between the operations (the reference rounds to 8 bits after each one; DESIGN.md states the difference).
//
// Two launches.  augment_stats_kernel: one workgroup per sample, the mean of gray over the cropped window as the image
// stands when the sample's contrast operation runs (the operations in front of it applied on the fly), summed in a fixed
// order.  augment_collate_kernel: one workgroup per 16 x 64 tile of output pixels; the tile and a one-pixel halo go through
// the pointwise chain once per pixel into LDS, the 3 x 3 blur reads LDS, then Normalize, the mix and the store.
//
// calm_augment_collate_erase is the same pass with RandomErasing between Normalize and the mix (the ERASE instantiations of
// the collate kernel): a sample's box is four integers read with its record, a predicate on the output pixels a thread
// owns, and the fill is a constant or counter-based noise — no extra LDS, no atomics, nothing addressed through the box.
#include "common.h"
#include "philox.h"
#include "pixel_quad.h"

namespace {

constexpr int NT = 256;
constexpr int TH = 16, TW = 64;                // output pixels of a workgroup
constexpr int LH = TH + 2, LW = TW + 2;        // with the blur's halo
constexpr int LS = 67;                         // LDS row stride: 67 = 3 (mod 4), so the four rows a wave reads at a column
                                               // stride of 4 floats fall on 64 different banks
constexpr int PLANE = LH * LS;

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float gray_of(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }
// blend(a, b, f) = clamp(f a + (1 - f) b, 0, 1)
__device__ __forceinline__ float blend(float a, float b, float f) { return clamp01(f * a + (1.0f - f) * b); }

// RGB -> HSV, h <- (h + f) mod 1, HSV -> RGB: the hexcone formulas (Python's colorsys), selects instead of branches
__device__ __forceinline__ void hue_shift(float& r, float& g, float& b, float f) {
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const float d = maxc - minc;
    if (d == 0.0f) return;                                  // s = 0: (v, v, v), which the pixel already is
    const float s = d / maxc;
    const float rc = (maxc - r) / d, gc = (maxc - g) / d, bc = (maxc - b) / d;
    float h = r == maxc ? bc - gc : g == maxc ? 2.0f + rc - bc : 4.0f + gc - rc;
    h = h / 6.0f;
    h = h - floorf(h);
    h = h + f;
    h = h - floorf(h);
    const float h6 = h * 6.0f;
    int i = (int)h6;                                        // 0..6 (6 when h rounded up to 1: sector 0 at fr = 0)
    const float fr = h6 - (float)i;
    if (i >= 6) i -= 6;
    const float v = maxc;
    const float p = v * (1.0f - s), q = v * (1.0f - s * fr), t = v * (1.0f - s * (1.0f - fr));
    r = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? t : v;
    g = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : p;
    b = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? v : i == 4 ? v : q;
}

// order[0..3] as one word (a run-time index into the byte array would put the struct into scratch)
__device__ __forceinline__ uint32_t order_word(const calm_aug_sample& s) {
    return (uint32_t)s.order[0] | (uint32_t)s.order[1] << 8 | (uint32_t)s.order[2] << 16 | (uint32_t)s.order[3] << 24;
}

// The first `upto` jitter operations of a sample in its order; unknown ids are skipped.  `mean` is the contrast mean.
__device__ __forceinline__ void jitter(float& r, float& g, float& b, const calm_aug_sample& s, int upto, float mean) {
    const uint32_t order = order_word(s);
    for (int k = 0; k < upto; ++k) {
        const int op = (order >> (8 * k)) & 255u;           // (uniform across the workgroup)
        if (op == CALM_AUG_OP_BRIGHTNESS) {
            r = blend(r, 0.0f, s.brightness); g = blend(g, 0.0f, s.brightness); b = blend(b, 0.0f, s.brightness);
        } else if (op == CALM_AUG_OP_CONTRAST) {
            r = blend(r, mean, s.contrast); g = blend(g, mean, s.contrast); b = blend(b, mean, s.contrast);
        } else if (op == CALM_AUG_OP_SATURATION) {
            const float y = gray_of(r, g, b);
            r = blend(r, y, s.saturation); g = blend(g, y, s.saturation); b = blend(b, y, s.saturation);
        } else if (op == CALM_AUG_OP_HUE) {
            hue_shift(r, g, b, s.hue);
        }
    }
}

// index of the sample's (first) contrast operation in its order, 4 = none
__device__ __forceinline__ int contrast_slot(const calm_aug_sample& s) {
    const uint32_t order = order_word(s);
    for (int k = 0; k < 4; ++k)
        if (((order >> (8 * k)) & 255u) == CALM_AUG_OP_CONTRAST) return k;
    return 4;
}

__global__ __launch_bounds__(NT) void augment_stats_kernel(const unsigned char* __restrict__ img, int Hs, int Ws,
                                                           const calm_aug_sample* __restrict__ samples,
                                                           float* __restrict__ gray_mean, int H, int W) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    const calm_aug_sample s = samples[b];
    const int kc = contrast_slot(s);
    if (kc == 4) {                                          // no contrast operation: nothing reads the mean
        if (threadIdx.x == 0) gray_mean[b] = 0.0f;
        return;
    }
    const int y0 = clampi(s.y0, 0, Hs - H), x0 = clampi(s.x0, 0, Ws - W);
    const long splane = (long)Hs * Ws;
    const unsigned char* src = img + (long)b * 3 * splane + (long)y0 * Ws + x0;
    float acc = 0.0f;
    for (int i = threadIdx.x; i < H * W; i += NT) {         // a thread's pixels in increasing i, then block_sum_256
        const int y = i / W, x = i - y * W;
        const long o = (long)y * Ws + x;
        float r = (float)src[o] / 255.0f, g = (float)src[splane + o] / 255.0f, bl = (float)src[2 * splane + o] / 255.0f;
        jitter(r, g, bl, s, kc, 0.0f);
        acc += gray_of(r, g, bl);
    }
    const float total = block_sum_256(acc, red);
    if (threadIdx.x == 0) gray_mean[b] = total / (float)(H * W);
}

// The halo'd tile of sample `b` in OUTPUT coordinates (rows ty0-1 .. ty0+TH, columns tx0-1 .. tx0+TW) after jitter,
// solarize and grayscale, as three planes.  Coordinates outside the window are reflected at the window's edge (-1 -> 1,
// H -> H-2) and then, being symmetric, the flip only mirrors the column that is read.  Without blur the halo is not needed
// and not computed.  Every coordinate is clamped into the window in the end: a tile's ragged part reads valid pixels.
__device__ __forceinline__ void load_tile(float* __restrict__ lds, const unsigned char* __restrict__ img, int Hs, int Ws,
                                          const calm_aug_sample& s, float mean, int b, int ty0, int tx0, int H, int W) {
    const int y0 = clampi(s.y0, 0, Hs - H), x0 = clampi(s.x0, 0, Ws - W);
    const long splane = (long)Hs * Ws;
    const unsigned char* src = img + (long)b * 3 * splane + (long)y0 * Ws + x0;
    const bool blur = (s.flags & CALM_AUG_BLUR) != 0, flip = (s.flags & CALM_AUG_FLIP) != 0;
    for (int e = threadIdx.x; e < LH * LW; e += NT) {
        const int ly = e / LW, lx = e - ly * LW;
        if (!blur && (ly == 0 || ly == LH - 1 || lx == 0 || lx == LW - 1)) continue;
        int y = ty0 + ly - 1, x = tx0 + lx - 1;
        y = y < 0 ? -y : y; y = y >= H ? 2 * H - 2 - y : y; y = clampi(y, 0, H - 1);
        x = x < 0 ? -x : x; x = x >= W ? 2 * W - 2 - x : x; x = clampi(x, 0, W - 1);
        if (flip) x = W - 1 - x;
        const long o = (long)y * Ws + x;
        float r = (float)src[o] / 255.0f, g = (float)src[splane + o] / 255.0f, bl = (float)src[2 * splane + o] / 255.0f;
        jitter(r, g, bl, s, 4, mean);
        if (s.flags & CALM_AUG_SOLARIZE) {
            r = r >= s.solarize_thr ? 1.0f - r : r;
            g = g >= s.solarize_thr ? 1.0f - g : g;
            bl = bl >= s.solarize_thr ? 1.0f - bl : bl;
        }
        if (s.flags & CALM_AUG_GRAYSCALE) r = g = bl = gray_of(r, g, bl);
        const int l = ly * LS + lx;
        lds[l] = r; lds[PLANE + l] = g; lds[2 * PLANE + l] = bl;
    }
}

// Four neighbouring output pixels of one plane: row `ly`, columns lx .. lx+3 in tile coordinates (LDS coordinates + 1)
__device__ __forceinline__ void blur4(const float* __restrict__ p, int ly, int lx, bool blur, float wc, float we,
                                      float out[4]) {
    if (!blur) {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = p[(ly + 1) * LS + lx + 1 + k];
        return;
    }
    float h[3][4];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        float v[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = p[(ly + dy) * LS + lx + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) h[dy][k] = we * v[k] + wc * v[k + 1] + we * v[k + 2];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = we * h[0][k] + wc * h[1][k] + we * h[2][k];
}

// RandomErasing (calm_augment_collate_erase): the per-sample boxes, the fill and the noise key.  Without ERASE the kernel
// reads none of it.
struct AugErase {
    const calm_erase_box* boxes;                   // DEVICE [B]
    int noise;                                     // value_mode: 0 constant, 1 standard normal noise
    float value[3];
    PhiloxKey key;
};

__device__ __forceinline__ bool in_box(const calm_erase_box& e, int y, int x) {
    return y >= e.y && y < e.y + e.h && x >= e.x && x < e.x + e.w;
}

// The fill of source sample s at output pixel (y, x), three channels: a function of (key, s, y, x) alone.  Box-Muller on
// one Philox call (include/calm_vit.h has the definition); the precise logf / sincospif / cospif, no fast intrinsics.
__device__ __forceinline__ void erase_fill(const AugErase& er, int s, int y, int x, int H, int W, float& f0, float& f1,
                                           float& f2) {
    if (!er.noise) {
        f0 = er.value[0]; f1 = er.value[1]; f2 = er.value[2];
        return;
    }
    const u32x4 w = philox4x32_10(((uint64_t)s * (uint64_t)H + (uint64_t)y) * (uint64_t)W + (uint64_t)x, er.key);
    const float ulp = 5.9604644775390625e-8f;                            // 2^-24: every product below is exact
    const float u1 = (float)((w[0] >> 8) + 1u) * ulp, u2 = (float)(w[1] >> 8) * ulp;
    const float u3 = (float)((w[2] >> 8) + 1u) * ulp, u4 = (float)(w[3] >> 8) * ulp;
    const float r1 = sqrtf(-2.0f * logf(u1)), r3 = sqrtf(-2.0f * logf(u3));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);
    f0 = r1 * cs; f1 = r1 * sn; f2 = r3 * cospif(2.0f * u4);
}

// The fills of a thread's four pixels of sample s where its box covers them (Philox runs only there)
__device__ __forceinline__ void erase_fill4(const AugErase& er, const calm_erase_box& e, int s, int y, int x, int H, int W,
                                            bool in[4], float f[3][4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        in[k] = in_box(e, y, x + k);
        f[0][k] = f[1][k] = f[2][k] = 0.0f;
        if (in[k]) erase_fill(er, s, y, x + k, H, W, f[0][k], f[1][k], f[2][k]);
    }
}

template <bool TOKENS, bool VEC, bool ERASE>
__global__ __launch_bounds__(NT) void augment_collate_kernel(const unsigned char* __restrict__ img, int Hs, int Ws,
                                                             const calm_aug_sample* __restrict__ samples,
                                                             const float* __restrict__ gray_mean,
                                                             float* __restrict__ out, int B, int H, int W, int mode,
                                                             float lam, int y1, int y2, int x1, int x2, Norm3 nm,
                                                             AugErase er) {
    __shared__ float tile[2][3 * PLANE];
    const int b = blockIdx.z, ty0 = blockIdx.y * TH, tx0 = blockIdx.x * TW;
    const int pb = b == 0 ? B - 1 : b - 1;
    // the partner is needed by MixUp everywhere and by CutMix in the tiles that meet the box
    const bool partner = mode == 1 || (mode == 2 && ty0 < y2 && ty0 + TH > y1 && tx0 < x2 && tx0 + TW > x1);
    const calm_aug_sample so = samples[b];
    load_tile(tile[0], img, Hs, Ws, so, gray_mean[b], b, ty0, tx0, H, W);
    calm_aug_sample sp = so;
    if (partner) {
        sp = samples[pb];
        load_tile(tile[1], img, Hs, Ws, sp, gray_mean[pb], pb, ty0, tx0, H, W);
    }
    __syncthreads();

    const int ly = threadIdx.x >> 4, lx = (threadIdx.x & 15) * 4;       // a thread: 4 pixels of a row, 3 channels
    const int y = ty0 + ly, x = tx0 + lx;
    if (y >= H || x >= W) return;
    const bool blur_o = (so.flags & CALM_AUG_BLUR) != 0, blur_p = (sp.flags & CALM_AUG_BLUR) != 0;
    float wc_o = 1.0f, we_o = 0.0f, wc_p = 1.0f, we_p = 0.0f;
    if (blur_o) {
        const float w1 = expf(-0.5f / (so.blur_sigma * so.blur_sigma));
        wc_o = 1.0f / (1.0f + 2.0f * w1); we_o = w1 / (1.0f + 2.0f * w1);
    }
    if (partner && blur_p) {
        const float w1 = expf(-0.5f / (sp.blur_sigma * sp.blur_sigma));
        wc_p = 1.0f / (1.0f + 2.0f * w1); we_p = w1 / (1.0f + 2.0f * w1);
    }
    // ERASE: each sample's box replaces its normalised pixels by its fill in front of the mix — the own sample's with
    // the own box, the partner's with the partner's box and the partner's noise
    bool in_o[4], in_p[4];
    float fill_o[3][4], fill_p[3][4];
    if constexpr (ERASE) {
        erase_fill4(er, er.boxes[b], b, y, x, H, W, in_o, fill_o);
        if (partner) erase_fill4(er, er.boxes[pb], pb, y, x, H, W, in_p, fill_p);
    }
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float own[4];
        blur4(tile[0] + c * PLANE, ly, lx, blur_o, wc_o, we_o, own);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[c][k] = (own[k] - nm.mean[c]) * nm.inv[c];
        if constexpr (ERASE) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[c][k] = in_o[k] ? fill_o[c][k] : v[c][k];
        }
        if (partner) {
            float oth[4];
            blur4(tile[1] + c * PLANE, ly, lx, blur_p, wc_p, we_p, oth);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float o = (oth[k] - nm.mean[c]) * nm.inv[c];
                if constexpr (ERASE) o = in_p[k] ? fill_p[c][k] : o;
                if (mode == 1) v[c][k] = v[c][k] * lam + o * (1.0f - lam);          // MixUp: x.roll(1,0)*(1-lam) + x*lam
                else if (y >= y1 && y < y2 && x + k >= x1 && x + k < x2) v[c][k] = o;   // CutMix box
            }
        }
    }
    if (TOKENS) store_quad_tokens<VEC>(out, b, H, W, y, x, v);
    else store_quad_f32<VEC>(out, b, H, W, y, x, v);
}

// Both entry points: the argument checks, the statistics launch and the collate launch; erase: null = ERASE off
int augment_collate(const uint8_t* img_u8, int32_t Hs, int32_t Ws, const calm_aug_sample* samples_dev, float* gray_mean,
                    float* out, int32_t B, int32_t H, int32_t W, int32_t out_tokens, int32_t mode, float lam,
                    const int32_t* box, const float* mean, const float* std, const AugErase* erase, void* stream) {
    if (!img_u8 || !out || !mean || !std || B <= 0 || H <= 0 || W <= 0 || Hs < H || Ws < W || mode < 0 || mode > 2) return CALM_E_INVAL;
    if (!samples_dev || !gray_mean) return CALM_E_INVAL;
    if (mode == 2 && !box) return CALM_E_INVAL;
    const int tiles_y = (H + TH - 1) / TH, tiles_x = (W + TW - 1) / TW;
    if (B > 65535 || tiles_y > 65535 || (int64_t)H * W > (1 << 30)) return CALM_E_UNSUPP;   // grid dimensions y and z; int pixel index
    const int y1 = box ? box[0] : 0, y2 = box ? box[1] : 0, x1 = box ? box[2] : 0, x2 = box ? box[3] : 0;
    const Norm3 nm = norm3(mean, std);
    int rc = calm_launch(augment_stats_kernel, B, NT, 0, stream, img_u8, Hs, Ws, samples_dev, gray_mean, H, W);
    if (rc != 0) return rc;
    const bool vec = W % 4 == 0 && aligned16(out);
    const AugErase er = erase ? *erase : AugErase{};
    return with_bool(out_tokens != 0, [&](auto tokens) {
        return with_bool(vec, [&](auto v) {
            return with_bool(erase != nullptr, [&](auto e) {
                return calm_launch(augment_collate_kernel<decltype(tokens)::value, decltype(v)::value, decltype(e)::value>,
                                   dim3(tiles_x, tiles_y, B), NT, 0, stream, img_u8, Hs, Ws, samples_dev, gray_mean, out, B, H,
                                   W, mode, lam, y1, y2, x1, x2, nm, er);
            });
        });
    });
}

}  // namespace

extern "C" {

int calm_augment_collate(const uint8_t* img_u8, int32_t Hs, int32_t Ws, const calm_aug_sample* samples_dev,
                         float* gray_mean, float* out, int32_t B, int32_t H, int32_t W, int32_t out_tokens, int32_t mode,
                         float lam, const int32_t* box, const float* mean, const float* std, void* stream) {
    return augment_collate(img_u8, Hs, Ws, samples_dev, gray_mean, out, B, H, W, out_tokens, mode, lam, box, mean, std,
                           nullptr, stream);
}

int calm_augment_collate_erase(const uint8_t* img_u8, int32_t Hs, int32_t Ws, const calm_aug_sample* samples_dev,
                               float* gray_mean, float* out, int32_t B, int32_t H, int32_t W, int32_t out_tokens,
                               int32_t mode, float lam, const int32_t* box, const float* mean, const float* std,
                               const calm_erase_box* boxes_dev, int32_t value_mode, const float* value, uint64_t seed,
                               uint64_t offset, void* stream) {
    if (!boxes_dev || value_mode < 0 || value_mode > 1 || (value_mode == 0 && !value)) return CALM_E_INVAL;
    AugErase er{};
    er.boxes = boxes_dev;
    er.noise = value_mode;
    for (int c = 0; c < 3; ++c) er.value[c] = value_mode == 0 ? value[c] : 0.0f;
    er.key = philox_key(seed, offset);
    return augment_collate(img_u8, Hs, Ws, samples_dev, gray_mean, out, B, H, W, out_tokens, mode, lam, box, mean, std, &er,
                           stream);
}

}  // extern "C"
