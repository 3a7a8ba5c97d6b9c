// The generative job on row tokens: the Huber loss between two tensors of one flat layout (the device-collate batch IS the
// target of the model's token output) and the reconstruction tallies of validation — Huber / MAE / MSE in normalised
// space, PSNR and SSIM in pixel space.  Every cross-workgroup sum goes through the caller's `partials` and is added in a
// fixed order: no atomics, results repeat bit for bit.
#include <float.h>
#include <math.h>

#include "common.h"
#include "huber.h"                       // huber_value / huber_slope, huber_rows_final_kernel (shared with mim.hip)

#define RECON_NT HUBER_NT

// ---- Huber on one flat layout ------------------------------------------------------------------------------------------
// n4 groups of four elements go as 16-byte vectors (0 when a base is not 16-byte aligned), the elements behind 4 * n4 one
// by one.  Grid-stride; forward: one block sum per workgroup into partials[blockIdx.x].
template <bool BWD>
static __global__ __launch_bounds__(RECON_NT) void huber_rows_kernel(const float* __restrict__ tokens,
                                                                     const float* __restrict__ target, float delta,
                                                                     const float* __restrict__ dloss,
                                                                     float* __restrict__ out, long n, long n4) {
    __shared__ float red[8];
    const long stride = (long)gridDim.x * RECON_NT;
    const long t0 = (long)blockIdx.x * RECON_NT + threadIdx.x;
    float acc = 0.f, scale = 0.f;
    if (BWD) scale = dloss[0] / (float)n;
    for (long q = t0; q < n4; q += stride) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(tokens + 4 * q);
        const f32x4 b = *reinterpret_cast<const f32x4*>(target + 4 * q);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = a[k] - b[k];
            if (BWD) o[k] = scale * huber_slope(d, delta);
            else acc += huber_value(d, delta);
        }
        if (BWD) *reinterpret_cast<f32x4*>(out + 4 * q) = o;
    }
    for (long e = 4 * n4 + t0; e < n; e += stride) {
        const float d = tokens[e] - target[e];
        if (BWD) out[e] = scale * huber_slope(d, delta);
        else acc += huber_value(d, delta);
    }
    if (!BWD) {
        acc = block_sum_256(acc, red);
        if (threadIdx.x == 0) out[blockIdx.x] = acc;
    }
}

// (the final pass, one workgroup over the block sums: huber_rows_final_kernel of huber.h)
static inline int huber_rows_grid(long n) {
    const long g = (n / 4 + RECON_NT - 1) / RECON_NT + 1;           // ~one vector per thread and turn at the cap
    return g < HUBER_MAX_GRID ? (int)g : HUBER_MAX_GRID;
}

// ---- reconstruction tallies --------------------------------------------------------------------------------------------
// Launch 1.  A workgroup owns one band of R output rows and one strip of RECON_STRIP_OUT output columns of one image.  A
// thread owns three of the strip's 768 row elements (element e = 3 * pixel + channel; consecutive threads, consecutive
// addresses) and walks the band's rows top to bottom, reading both tensors straight from memory, once.  The last eleven
// pixel-space rows of both stay in registers — as (x, y) pairs, so the arithmetic is two-wide packed fp32 — and the
// vertical half of the separable window needs no staging of the inputs at all: from the first row with ten rows above
// it, every row yields the five vertically filtered fields (x, y | x^2, y^2 | xy) of one output row.  They go to LDS as
// two arrays of pairs and one of floats, indexed by element, and after ONE barrier the horizontal half runs: thread t
// takes channel t % 3 of the three neighbouring pixels 3 (t / 3) .. + 2, whose windows share 13 taps (elements
// 9 (t / 3) + t % 3 + 3 m), each read once and added to the up to three outputs it belongs to — 39 LDS reads per thread
// and row instead of 165 for three unrelated outputs.  The channel interleave needs no planar copy: the taps of one
// channel are every third element.  The field rows are double-buffered, so one barrier per row is enough.
// LDS: 2 * 5 * 768 floats = 30 KB, five workgroups per CU by that count (registers allow fewer).
// The moments are taken of (p - 1/2): the variances are shift-invariant, and sum w a^2 - (sum w a)^2 then cancels between
// numbers four times smaller than with p in [0, 1].
// Error sums cover each element once: a band owns the rows [band * R, band * R + R) — the last band to S — and a strip
// the pixels [strip * 246, strip * 246 + 246) — the last strip to S; everything else it reads is halo.
struct ReconGeom {
    int S, R, nb, ns;
    int tok_words;               // bf16 tokens may be read as 32-bit words: 4-byte aligned base, an even element count
    float delta;
    float mean[3], std[3];
    float w[RECON_WIN];
};
#define RECON_STRIP_E (3 * RECON_STRIP_PX)
typedef float f32x2 __attribute__((ext_vector_type(2)));
static_assert(RECON_STRIP_OUT % 3 == 0 && RECON_STRIP_OUT <= RECON_NT - RECON_NT % 3,
              "the horizontal pass hands a thread three neighbouring pixels of one channel");
static_assert(9 * (RECON_STRIP_OUT / 3 - 1) + 2 + 3 * (RECON_WIN + 1) < RECON_STRIP_E, "the last tap stays inside the field row");

template <bool BF16, bool NCHW, bool SSIM>
static __global__ __launch_bounds__(RECON_NT) void recon_band_kernel(const void* __restrict__ tokens,
                                                                     const float* __restrict__ target,
                                                                     float* __restrict__ partials, const ReconGeom g) {
    __shared__ f32x2 Vxy[2][RECON_STRIP_E], Vsq[2][RECON_STRIP_E];   // (sum w x, sum w y), (sum w x^2, sum w y^2)
    __shared__ float Vc[2][RECON_STRIP_E];                           // sum w x y
    __shared__ float red[8];
    const int tid = threadIdx.x;
    const int S = g.S, E = 3 * S;
    const int strip = blockIdx.x % g.ns;
    const int band = (blockIdx.x / g.ns) % g.nb;
    const long b = blockIdx.x / g.ns / g.nb;
    const int px0 = strip * RECON_STRIP_OUT, row0 = band * g.R;
    const int own_row_end = band == g.nb - 1 ? S : row0 + g.R;
    const int own_px_end = strip == g.ns - 1 ? S : px0 + RECON_STRIP_OUT;
    int row_end = own_row_end;
    if (SSIM) row_end = row0 + g.R + RECON_WIN - 1 < S ? row0 + g.R + RECON_WIN - 1 : S;

    bool valid[3], own_col[3];
    int px[3], ch[3];
    float mean[3], std[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int el = tid + RECON_NT * c;
        px[c] = px0 + el / 3;
        ch[c] = el % 3;
        valid[c] = 3 * px0 + el < E;
        own_col[c] = valid[c] && px[c] < own_px_end;
        mean[c] = ch[c] == 0 ? g.mean[0] : ch[c] == 1 ? g.mean[1] : g.mean[2];
        std[c] = ch[c] == 0 ? g.std[0] : ch[c] == 1 ? g.std[1] : g.std[2];
    }
    // the horizontal pass: outputs at the pixels px0 + 3 * (tid / 3) + {0, 1, 2}, channel tid % 3; first tap at element hb
    const int hq = tid / 3, hb = 9 * hq + tid % 3;
    bool out_ok[3];
#pragma unroll
    for (int o = 0; o < 3; ++o) out_ok[o] = SSIM && 3 * hq + o < RECON_STRIP_OUT && px0 + 3 * hq + o <= S - RECON_WIN;
    f32x2 ring[3][RECON_WIN];                                        // the last eleven rows of (x, y) - 1/2, statically indexed
    float s_hub = 0.f, s_abs = 0.f, s_sq = 0.f, s_pix = 0.f, s_ssim = 0.f;
    bool bad = false;
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;

    // The loads run two rows ahead of the arithmetic: a row's iteration ends in a barrier, and nothing else would hide the
    // memory latency of the next row behind it (measured: 318 us -> see DESIGN.md at the Base-224 batch).
    auto load_row = [&](int i, float* gq, float* tq) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            gq[c] = tq[c] = 0.f;
            if (valid[c] && i < row_end) {
                const long at = ((long)b * S + i) * E + 3 * px0 + tid + RECON_NT * c;
                // bf16: the raw bits travel through the queue — widening them here would wait for the load.  Where the base
                // allows it, the aligned 32-bit word that holds the element (its half is picked at use).
                if (BF16 && g.tok_words) {
                    gq[c] = __uint_as_float(reinterpret_cast<const unsigned*>(tokens)[at >> 1]);
                } else if (BF16) {
                    gq[c] = __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(tokens)[at]);
                } else {
                    gq[c] = reinterpret_cast<const float*>(tokens)[at];
                }
                tq[c] = NCHW ? target[(((long)b * 3 + ch[c]) * S + i) * S + px[c]] : target[at];
            }
        }
    };
    float g0[3], t0[3], g1[3], t1[3], g2[3], t2[3];
    load_row(row0, g0, t0);
    load_row(row0 + 1, g1, t1);
    for (int base = row0; base < row_end; base += RECON_WIN) {
#pragma unroll
        for (int u = 0; u < RECON_WIN; ++u) {
            const int i = base + u;
            if (i < row_end) {                                       // (the same for the whole workgroup)
                const bool own_row = i < own_row_end;
                load_row(i + 2, g2, t2);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float gv = g0[c];
                    const float tv = t0[c];
                    if (BF16) {
                        const unsigned raw = __float_as_uint(gv);
                        const long at = ((long)b * S + i) * E + 3 * px0 + tid + RECON_NT * c;
                        gv = __uint_as_float(g.tok_words && (at & 1) ? raw & 0xffff0000u : raw << 16);
                    }
                    g0[c] = g1[c];
                    t0[c] = t1[c];
                    g1[c] = g2[c];
                    t1[c] = t2[c];
                    const float xp = fminf(fmaxf(fmaf(gv, std[c], mean[c]), 0.f), 1.f);
                    const float yp = fminf(fmaxf(fmaf(tv, std[c], mean[c]), 0.f), 1.f);
                    if (own_row && own_col[c]) {
                        bad |= !(fabsf(gv) <= FLT_MAX);
                        const float d = gv - tv, pd = xp - yp;
                        s_hub += huber_value(d, g.delta);
                        s_abs += fabsf(d);
                        s_sq = fmaf(d, d, s_sq);
                        s_pix = fmaf(pd, pd, s_pix);
                    }
                    ring[c][u] = f32x2{xp - 0.5f, yp - 0.5f};
                }
                if (SSIM && i - row0 >= RECON_WIN - 1) {              // output row i - 10: slot u holds its lowest row
                    const int buf = (i - row0) & 1;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        // (a third of the strip that lies outside the image — all of it at S <= 85 — has no taps to feed:
                        // the same for the whole workgroup)
                        if (3 * px0 + RECON_NT * c >= E + 3 * (RECON_WIN + 1)) continue;
                        f32x2 vxy = {0.f, 0.f}, vsq = {0.f, 0.f};
                        float vc = 0.f;
#pragma unroll
                        for (int s = 0; s < RECON_WIN; ++s) {
                            const float wv = g.w[(s - u - 1 + 2 * RECON_WIN) % RECON_WIN];   // (slot u + 1 is the oldest row)
                            const f32x2 p = ring[c][s];
                            const f32x2 wp = wv * p;
                            vxy += wp;
                            vsq = __builtin_elementwise_fma(wp, p, vsq);
                            vc = fmaf(wp.x, p.y, vc);
                        }
                        const int el = tid + RECON_NT * c;
                        Vxy[buf][el] = vxy;
                        Vsq[buf][el] = vsq;
                        Vc[buf][el] = vc;
                    }
                    __syncthreads();
                    if (out_ok[0]) {                                 // (a thread's three outputs are valid from the left)
                        f32x2 mxy[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}}, msq[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
                        float mc[3] = {0.f, 0.f, 0.f};
#pragma unroll
                        for (int m = 0; m < RECON_WIN + 2; ++m) {
                            const f32x2 txy = Vxy[buf][hb + 3 * m], tsq = Vsq[buf][hb + 3 * m];
                            const float tc = Vc[buf][hb + 3 * m];
#pragma unroll
                            for (int o = 0; o < 3; ++o) {
                                if (m - o < 0 || m - o >= RECON_WIN) continue;           // (resolved when unrolled)
                                const float wv = g.w[m - o];
                                mxy[o] = __builtin_elementwise_fma(f32x2{wv, wv}, txy, mxy[o]);
                                msq[o] = __builtin_elementwise_fma(f32x2{wv, wv}, tsq, msq[o]);
                                mc[o] = fmaf(wv, tc, mc[o]);
                            }
                        }
#pragma unroll
                        for (int o = 0; o < 3; ++o) {
                            if (!out_ok[o]) continue;
                            const float mx = mxy[o].x, my = mxy[o].y;
                            const float sxx = msq[o].x - mx * mx, syy = msq[o].y - my * my, sxy = mc[o] - mx * my;
                            const float ux = mx + 0.5f, uy = my + 0.5f;
                            s_ssim += ((2.f * ux * uy + C1) * (2.f * sxy + C2)) / ((ux * ux + uy * uy + C1) * (sxx + syy + C2));
                        }
                    }
                }
            }
        }
    }
    s_hub = block_sum_256(s_hub, red);
    s_abs = block_sum_256(s_abs, red);
    s_sq = block_sum_256(s_sq, red);
    s_pix = block_sum_256(s_pix, red);
    s_ssim = block_sum_256(s_ssim, red);
    const float nbad = block_sum_256(bad ? 1.f : 0.f, red);
    if (tid == 0) {
        float* rec = partials + (long)blockIdx.x * RECON_REC_FLOATS;
        *reinterpret_cast<f32x4*>(rec) = f32x4{s_hub, s_abs, s_sq, s_pix};
        *reinterpret_cast<f32x4*>(rec + 4) = f32x4{s_ssim, nbad, 0.f, 0.f};
    }
}

// Launch 2, one workgroup.  Images are staged 256 at a time: thread t adds the records of image i0 + t in double, in record
// order, and leaves the image's values in LDS; threads 0 .. 7 each own one slot of `sums` and add the staged images to a
// running double in image order.  One plain read-modify-write per slot at the end, ordered by the stream.
static __global__ __launch_bounds__(RECON_NT) void recon_fold_kernel(const float* __restrict__ partials,
                                                                     double* __restrict__ sums, int B, int S, int per_image,
                                                                     int want_ssim) {
    __shared__ double img[8][RECON_NT];
    const int t = threadIdx.x;
    const double elems = 3.0 * (double)S * (double)S;
    const double valid = (double)recon_valid(S);
    double run = 0.0;
    for (int i0 = 0; i0 < B; i0 += RECON_NT) {
        const int n = B - i0 < RECON_NT ? B - i0 : RECON_NT;
        if (t < n) {
            const float* rec = partials + (long)(i0 + t) * per_image * RECON_REC_FLOATS;
            double hub = 0.0, ab = 0.0, sq = 0.0, pix = 0.0, ss = 0.0, bad = 0.0;
            for (int r = 0; r < per_image; ++r) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(rec + (long)r * RECON_REC_FLOATS);
                const f32x4 c = *reinterpret_cast<const f32x4*>(rec + (long)r * RECON_REC_FLOATS + 4);
                hub += (double)a[0];
                ab += (double)a[1];
                sq += (double)a[2];
                pix += (double)a[3];
                ss += (double)c[0];
                bad += (double)c[1];
            }
            const bool finite = bad == 0.0;
            const double mse = pix / elems;
            img[0][t] = 1.0;
            img[1][t] = finite ? 0.0 : 1.0;
            img[2][t] = finite ? hub : 0.0;
            img[3][t] = finite ? ab : 0.0;
            img[4][t] = finite ? sq : 0.0;
            img[5][t] = finite ? elems : 0.0;
            img[6][t] = finite ? 10.0 * log10(1.0 / (mse > 1e-10 ? mse : (mse != mse ? mse : 1e-10))) : 0.0;
            img[7][t] = finite ? ss / (3.0 * valid * valid) : 0.0;
        }
        __syncthreads();
        if (t < 8)
            for (int k = 0; k < n; ++k) run += img[t][k];
        __syncthreads();
    }
    if (t < 7 || (t == 7 && want_ssim)) sums[t] += run;
}

extern "C" {

int calm_recon_huber_rows_fwd(const float* tokens, const float* target, float delta, float* loss, int64_t n,
                              float* partials, void* stream) {
    if (!tokens || !target || !loss || !partials || n <= 0) return CALM_E_INVAL;
    if (n >= (1ll << 31)) return CALM_E_UNSUPP;
    if ((reinterpret_cast<uintptr_t>(tokens) | reinterpret_cast<uintptr_t>(target)) & 3u) return CALM_E_LAYOUT;
    const long n4 = aligned16(tokens) && aligned16(target) ? (long)n / 4 : 0;
    const int grid = huber_rows_grid((long)n);
    if (int e = calm_launch(huber_rows_kernel<false>, grid, RECON_NT, 0, stream, tokens, target, delta, nullptr, partials,
                            (long)n, n4))
        return e;
    return calm_launch(huber_rows_final_kernel, 1, RECON_NT, 0, stream, partials, grid, 1.0f / (float)n, loss);
}

int calm_recon_huber_rows_bwd(const float* tokens, const float* target, float delta, const float* dloss, float* dtokens,
                              int64_t n, void* stream) {
    if (!tokens || !target || !dloss || !dtokens || n <= 0) return CALM_E_INVAL;
    if (n >= (1ll << 31)) return CALM_E_UNSUPP;
    if ((reinterpret_cast<uintptr_t>(tokens) | reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(dtokens)) & 3u)
        return CALM_E_LAYOUT;
    const long n4 = aligned16(tokens) && aligned16(target) && aligned16(dtokens) ? (long)n / 4 : 0;
    return calm_launch(huber_rows_kernel<true>, huber_rows_grid((long)n), RECON_NT, 0, stream, tokens, target, delta, dloss,
                       dtokens, (long)n, n4);
}

int calm_recon_metrics(const void* tokens, int32_t tokens_type, const float* target, int32_t target_layout,
                       const float* mean, const float* std, float delta, int32_t want_ssim, double* sums, int32_t B,
                       int32_t S, float* partials, void* stream) {
    if (!tokens || !target || !mean || !std || !sums || !partials || B <= 0 || S <= 0) return CALM_E_INVAL;
    if (tokens_type != CALM_ST_F32 && tokens_type != CALM_ST_BF16) return CALM_E_INVAL;
    if (target_layout != CALM_RECON_ROWS && target_layout != CALM_RECON_NCHW) return CALM_E_INVAL;
    if (S > 4096 || (want_ssim && S < RECON_WIN)) return CALM_E_UNSUPP;
    ReconGeom g{};
    g.S = S;
    g.R = recon_band_rows(S);
    g.nb = recon_bands(S);
    g.ns = recon_strips(S);
    g.delta = delta;
    const long per_image = (long)g.nb * g.ns;
    if ((long)B * per_image >= (1l << 31)) return CALM_E_UNSUPP;
    const bool bf16 = tokens_type == CALM_ST_BF16;
    g.tok_words = bf16 && (reinterpret_cast<uintptr_t>(tokens) & 3u) == 0 && (((long)B * S * S) & 1) == 0;
    if (!aligned16(partials) || (reinterpret_cast<uintptr_t>(tokens) & (bf16 ? 1u : 3u)) ||
        (reinterpret_cast<uintptr_t>(target) & 3u) || (reinterpret_cast<uintptr_t>(sums) & 7u))
        return CALM_E_LAYOUT;
    double w[RECON_WIN], wsum = 0.0;
    for (int k = 0; k < RECON_WIN; ++k) {
        const double d = k - (RECON_WIN - 1) / 2;
        wsum += w[k] = exp(-d * d / (2.0 * 1.5 * 1.5));
    }
    for (int k = 0; k < RECON_WIN; ++k) g.w[k] = (float)(w[k] / wsum);
    for (int c = 0; c < 3; ++c) {
        g.mean[c] = mean[c];
        g.std[c] = std[c];
    }
    const int grid = (int)((long)B * per_image);
    if (int e = with_bool(bf16, [&](auto b16) {
            return with_bool(target_layout == CALM_RECON_NCHW, [&](auto nchw) {
                return with_bool(want_ssim != 0, [&](auto ssim) {
                    return calm_launch(recon_band_kernel<decltype(b16)::value, decltype(nchw)::value, decltype(ssim)::value>,
                                       grid, RECON_NT, 0, stream, tokens, target, partials, g);
                });
            });
        }))
        return e;
    return calm_launch(recon_fold_kernel, 1, RECON_NT, 0, stream, partials, sums, B, S, (int)per_image, want_ssim != 0);
}

}  // extern "C"
