// Fused cross-axial latent-mask attention, forward (Vi_Tools_CNN_less_V2.py:288-299).
//
//   R      = Q_all K_all^T                      (all heads concatenated, raw, un-scaled)     [Sq,Skv]
//   M      = W2 gelu(W1 R^T + b1) + b2          (2-layer MLP along the KEY axis, W/sigma)    [Sq,Skv]
//   O_h    = softmax_j(Q_h K_h^T / sqrt(hd) + M) V_h                                         per head
//
// One workgroup = NW waves = NW 16-query tiles of one batch element; the wave keeps its 16 queries on
// the MFMA *lane/column* index and the keys on the accumulator rows ("transposed" orientation):
//   R^T[j,i], M^T[j,i], S^T[j,i], P^T[j,i], O^T[d,i]   with i = lane&15.
// With v_mfma_f32_16x16x4_f32 an accumulator tile (rows in registers, column on the lane) is directly the
// B operand of the next product that sums over its ROW index, so the whole chain
//   R^T -> (W1 . R^T) -> gelu -> (W2 . hid) -> + scale K_h Q_h^T -> softmax -> (V_h^T . P^T)
// runs register-to-register: nothing but the streamed operands (K/Q column chunks, W1/W2 row chunks, V
// key chunks) goes through LDS, and the [H,Sq,Skv] probabilities never have to exist in HBM.
// The softmax reduction over keys is 4*NJ in-lane values + two wave shuffles (xor 16, xor 32).
// LDS images are K-major ([k][row]) with row strides chosen so that the 4 lane groups of a b32 read
// land 16 banks apart (conflict-free); global->LDS staging is register-prefetched one chunk ahead.
#include "common.h"

#include <atomic>

#ifndef ATT_TR_ROWFAST
#define ATT_TR_ROWFAST 1   // W1-chunk staging: hidden rows fastest over lanes (16-way LDS write conflict otherwise)
#endif

namespace {

typedef float f32x4v __attribute__((ext_vector_type(4)));

struct AttnFwdP {
    const float* q; const float* k; const float* v;
    const float* w1; const float* b1; const float* s1;
    const float* w2; const float* b2; const float* s2;
    float* out;
    float* R; float* hp; float* hg; float* Mk; float* P;   // saved for backward (P optional)
    int B, Sq, Skv, H, hd;
    float scale;
    float* lse;                  // [B,H,Sq] row log-sum-exp of the logits (optional; calm_attention_fwd_lse)
};

constexpr int NV_Q = 1;   // ... for a [16*NW x 16] query chunk

// ---- staging helpers (all threads of the block cooperate) -------------------------------------
// block of `rows` rows x 16 columns (columns c0..c0+15 of a row-major matrix, row stride `stride`),
// staged K-MAJOR: dst[c][row].  Columns >= cmax are zero-filled.
template <int NV> struct Regs { f32x4v v[NV]; };

template <int NT, int NV>
__device__ __forceinline__ void km_load(Regs<NV>& rg, const float* __restrict__ src, long stride, int rows, int c0,
                                        int cmax) {
    constexpr int nt = NT;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = threadIdx.x + u * nt;
        const int row = f >> 2, c = c0 + 4 * (f & 3);
        f32x4v val = {0.f, 0.f, 0.f, 0.f};
        if (row < rows && c < cmax) val = *reinterpret_cast<const f32x4v*>(src + (long)row * stride + c);
        rg.v[u] = val;
    }
}
template <int NT, int NV>
__device__ __forceinline__ void km_store(const Regs<NV>& rg, float* __restrict__ dst, int ld, int rows) {
    constexpr int nt = NT;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = threadIdx.x + u * nt;
        const int row = f >> 2, cq = 4 * (f & 3);
        if (row < rows) {
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[(cq + e) * ld + row] = rg.v[u][e];
        }
    }
}
// block of 16 rows x `cols` contiguous columns staged TRANSPOSED: dst[col][r] (r = 0..15), ld = row stride of dst
template <int NT, int NV>
__device__ __forceinline__ void tr_load(Regs<NV>& rg, const float* __restrict__ src, long stride, int cols) {
    constexpr int nt = NT;
    const int per_row = cols >> 2;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = threadIdx.x + u * nt;
#if ATT_TR_ROWFAST
        const int r = f & 15, cq = f >> 4;            // 16 rows fastest: LDS writes hit 16 consecutive banks
        f32x4v val = {0.f, 0.f, 0.f, 0.f};
        if (cq < per_row) val = *reinterpret_cast<const f32x4v*>(src + (long)r * stride + 4 * cq);
#else
        const int r = f / per_row, cq = f - r * per_row;
        f32x4v val = {0.f, 0.f, 0.f, 0.f};
        if (r < 16) val = *reinterpret_cast<const f32x4v*>(src + (long)r * stride + 4 * cq);
#endif
        rg.v[u] = val;
    }
}
template <int NT, int NV>
__device__ __forceinline__ void tr_store(const Regs<NV>& rg, float* __restrict__ dst, int ld, int cols) {
    constexpr int nt = NT;
    const int per_row = cols >> 2;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = threadIdx.x + u * nt;
#if ATT_TR_ROWFAST
        const int r = f & 15, cq = f >> 4;
        if (cq < per_row) {
#else
        const int r = f / per_row, cq = f - r * per_row;
        if (r < 16) {
#endif
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[(4 * cq + e) * ld + r] = rg.v[u][e];
        }
    }
}
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// ---- LDS geometry: defined here once; the kernels and the host code that sizes their launches both read it ----------
constexpr size_t LDS_MAX = 160 * 1024;         // LDS of a CU = the most a workgroup can ask for

// row stride (floats) of a K-major [c][row] image: = 16 (mod 32), so the 4 lane groups of a b32 read land 16 banks apart
__host__ __device__ constexpr int ld_km(int rows) { return rows + ((rows % 32 == 16) ? 0 : 16); }

// NJ 16-row tiles on the accumulator rows (forward / query side: the keys; key side: the queries — the model has
// Sq == Skv), NW waves = NW 16-row tiles of the other axis per workgroup.  Offsets and sizes in floats.
template <int NJ_, int NW_>
struct AttGeo {
    static constexpr int NJ = NJ_, NW = NW_;
    static constexpr int SKV = 16 * NJ, TQ = 16 * NW;
    static constexpr int LDJ = ld_km(SKV), LDQ = ld_km(TQ);    // K / Q column-chunk images [c][j], [c][i]
    static constexpr int LDN1 = 20;                            // W1 chunk image [j][nn]
    static constexpr int LDJ2 = SKV + 4;                       // W2 chunk image [nn][j]
    static_assert(LDJ % 32 == 16 && LDQ % 32 == 16, "K-major strides: lane groups 16 banks apart");
    // phases 1 and 3 (and the query-side backward): K and Q chunk double buffers, then the whole head stripe
    static constexpr int Q_OFF = 32 * LDJ, V_OFF = Q_OFF + 32 * LDQ;
    __device__ static float* buf_k(float* smem, int i) { return smem + i * 16 * LDJ; }
    __device__ static float* buf_q(float* smem, int i) { return smem + Q_OFF + i * 16 * LDQ; }
    // phase 2: W1 and W2 chunk double buffers
    static constexpr int W2_OFF = 2 * SKV * LDN1, PH2 = W2_OFF + 32 * LDJ2;
    __device__ static float* buf_w1(float* smem, int i) { return smem + i * SKV * LDN1; }
    __device__ static float* buf_w2(float* smem, int i) { return smem + W2_OFF + i * 16 * LDJ2; }
    // the part that depends on the run-time head dim: the [SKV][LDV] stripe of one head (V_h, K_h, dO_h or Q_h)
    struct Hd { int DT, hdp, LDV, stripe; };
    __host__ __device__ static constexpr Hd at(int hd) {
        const int DT = (hd + 15) / 16;                         // d-tiles (<= 8)
        const int hdp = 16 * DT, LDV = hdp + 4;                // 4*LDV % 32 == 16
        return {DT, hdp, LDV, SKV * LDV};
    }
    // dynamic LDS bytes of the kernels
    static constexpr size_t fwd_bytes(int hd) {
        const int ph13 = V_OFF + at(hd).stripe;
        return sizeof(float) * (size_t)(ph13 > PH2 ? ph13 : PH2);
    }
    static constexpr size_t bwd_q_bytes(int hd) { return sizeof(float) * (size_t)(V_OFF + at(hd).stripe); }
    static constexpr size_t bwd_kv_bytes(int hd) { return sizeof(float) * (size_t)at(hd).stripe; }
    // folded route: the front kernel stages no stripe, the dQ kernel nothing but the K_h stripe
    static constexpr size_t bwd_front_bytes() { return sizeof(float) * (size_t)V_OFF; }
    static constexpr size_t bwd_dq_bytes(int hd) { return sizeof(float) * (size_t)at(hd).stripe; }
    // ring form of the two back kernels: the stripe goes through LDS as [SKV][32]-column slabs (two d-tiles, the unit
    // of the contraction's d loop), two slots — whatever the head dim
    static constexpr int SLAB_COLS = 32, LDS_SLAB = SLAB_COLS + 4, SLAB = SKV * LDS_SLAB;
    static_assert(4 * LDS_SLAB % 32 == 16, "slab row stride: the residue rule of the stripe stride LDV");
    __device__ static float* slab_slot(float* smem, int i) { return smem + (i & 1) * SLAB; }
    static_assert(sizeof(float) * (size_t)(2 * SLAB) <= LDS_MAX, "the slab ring fits at every head dim");
    static constexpr size_t bwd_ring_bytes() { return sizeof(float) * (size_t)(2 * SLAB); }
};

// LEAN (calm_attention_infer): the forward of a model that will run no backward.  R, hp, hg, P and lse are absent — their
// stores, and the address arithmetic that only feeds them, are compiled out; every value that reaches out or Mk goes
// through the same instructions in the same order, so both are bit-identical to the stored form's.
template <int NJ, int NW, bool LEAN>
__global__ __launch_bounds__(64 * NW) void attn_fwd_kernel(const AttnFwdP p) {
    constexpr int NTH = 64 * NW;
    constexpr int NV_K = (NJ + NW - 1) / NW;   // float4 per thread for a [16*NJ x 16] chunk
    extern __shared__ __attribute__((aligned(16))) float smem[];
    typedef AttGeo<NJ, NW> G;
    constexpr int SKV = G::SKV, LDJ = G::LDJ, LDN1 = G::LDN1, LDJ2 = G::LDJ2;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int TQ = G::TQ, LDQ = G::LDQ;
    const int r16 = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * TQ;                            // first query of the workgroup
    const int nq = min(TQ, p.Sq - q0);                         // queries of this workgroup (multiple of 16)
    const bool active = 16 * wave < nq;
    const int iq = q0 + 16 * wave + r16;                       // this lane's query (valid if active)
    const int D = p.H * p.hd;

    const float* qb = p.q + ((long)b * p.Sq + q0) * D;
    const float* kb = p.k + (long)b * p.Skv * D;
    const float* vb = p.v + (long)b * p.Skv * D;

    auto bufK = [&](int i) { return G::buf_k(smem, i); };
    auto bufQ = [&](int i) { return G::buf_q(smem, i); };

    f32x4v accR[NJ];
#pragma unroll
    for (int t = 0; t < NJ; ++t) accR[t] = (f32x4v){0.f, 0.f, 0.f, 0.f};

    // ================= phase 1: R^T[j,i] = sum_c K_all[j,c] Q_all[i,c] =================
    {
        Regs<NV_K> rk; Regs<NV_Q> rq;
        const int nch = (D + 15) / 16;
        km_load<NTH>(rk, kb, D, SKV, 0, D);
        km_load<NTH>(rq, qb, D, nq, 0, D);
        km_store<NTH>(rk, bufK(0), LDJ, SKV);
        km_store<NTH>(rq, bufQ(0), LDQ, nq);
        __syncthreads();
#pragma unroll 1
        for (int c = 0; c < nch; ++c) {
            const int cur = c & 1;
            if (c + 1 < nch) {
                km_load<NTH>(rk, kb, D, SKV, 16 * (c + 1), D);
                km_load<NTH>(rq, qb, D, nq, 16 * (c + 1), D);
            }
            if (active) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float bq = bufQ(cur)[(4 * s + g) * LDQ + 16 * wave + r16];
#pragma unroll
                    for (int t = 0; t < NJ; ++t)
                        accR[t] = MFMA16(bufK(cur)[(4 * s + g) * LDJ + 16 * t + r16], bq, accR[t]);
                    __builtin_amdgcn_sched_barrier(0);       // keep at most NJ operand loads in flight
                }
            }
            if (c + 1 < nch) {
                km_store<NTH>(rk, bufK(cur ^ 1), LDJ, SKV);
                km_store<NTH>(rq, bufQ(cur ^ 1), LDQ, nq);
            }
            __syncthreads();
        }
    }
    if (!LEAN && active) {   // save R[b,i,j] (4 consecutive keys per register group)
        float* Rrow = p.R + ((long)b * p.Sq + iq) * p.Skv;
#pragma unroll
        for (int t = 0; t < NJ; ++t) *reinterpret_cast<f32x4v*>(Rrow + 16 * t + 4 * g) = accR[t];
    }

    // ================= phase 2: M^T = W2 gelu(W1 R^T + b1) + b2 =================
    f32x4v accM[NJ];
#pragma unroll
    for (int t = 0; t < NJ; ++t) accM[t] = (f32x4v){0.f, 0.f, 0.f, 0.f};
    {
        const float inv1 = 1.0f / p.s1[0], inv2 = 1.0f / p.s2[0];
        auto bufW1 = [&](int i) { return G::buf_w1(smem, i); };
        auto bufW2 = [&](int i) { return G::buf_w2(smem, i); };
        const int nch = 2 * NJ;                                 // 2*Skv hidden units, 16 per chunk
        Regs<NV_K> r1, r2;
        tr_load<NTH>(r1, p.w1, SKV, SKV);                            // rows n0..n0+15 of W1 [2Skv, Skv]
        km_load<NTH>(r2, p.w2, 2 * SKV, SKV, 0, 2 * SKV);            // columns n0..n0+15 of W2 [Skv, 2Skv]
        tr_store<NTH>(r1, bufW1(0), LDN1, SKV);
        km_store<NTH>(r2, bufW2(0), LDJ2, SKV);
        __syncthreads();
#pragma unroll 1
        for (int c = 0; c < nch; ++c) {
            const int cur = c & 1, n0 = 16 * c;
            if (c + 1 < nch) {
                tr_load<NTH>(r1, p.w1 + (long)(n0 + 16) * SKV, SKV, SKV);
                km_load<NTH>(r2, p.w2, 2 * SKV, SKV, n0 + 16, 2 * SKV);
            }
            if (active) {
                // two partial accumulators: a single 16x16x4 chain would stall on its 40-cycle dependent latency
                f32x4v hid = {0.f, 0.f, 0.f, 0.f}, hid2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < NJ; ++t) {
#pragma unroll
                    for (int r = 0; r < 4; r += 2) {
                        hid = MFMA16(bufW1(cur)[(16 * t + 4 * g + r) * LDN1 + r16], accR[t][r], hid);
                        hid2 = MFMA16(bufW1(cur)[(16 * t + 4 * g + r + 1) * LDN1 + r16], accR[t][r + 1], hid2);
                    }
                }
                hid = hid + hid2;
                const f32x4v bb = *reinterpret_cast<const f32x4v*>(p.b1 + n0 + 4 * g);
                f32x4v pre, act;
#pragma unroll
                for (int r = 0; r < 4; ++r) { pre[r] = hid[r] * inv1 + bb[r]; act[r] = gelu_erf_f(pre[r]); }
                if constexpr (!LEAN) {
                    const long ho = ((long)b * p.Sq + iq) * (2 * SKV) + n0 + 4 * g;
                    *reinterpret_cast<f32x4v*>(p.hp + ho) = pre;
                    *reinterpret_cast<f32x4v*>(p.hg + ho) = act;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int t = 0; t < NJ; ++t)
                        accM[t] = MFMA16(bufW2(cur)[(4 * g + r) * LDJ2 + 16 * t + r16], act[r], accM[t]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (c + 1 < nch) {
                tr_store<NTH>(r1, bufW1(cur ^ 1), LDN1, SKV);
                km_store<NTH>(r2, bufW2(cur ^ 1), LDJ2, SKV);
            }
            __syncthreads();
        }
        // the mask tile leaves the registers here (it would otherwise stay live across the head loop):
        // Mk[b,i,j] is written once and re-read per head from L2 (NJ float4 per lane)
        if (active) {
            float* Mrow = p.Mk + ((long)b * p.Sq + iq) * p.Skv;
            constexpr int BG = 4;                              // bias chunks requested four at a time (see attn_bwd_q_kernel)
#pragma unroll
            for (int t0 = 0; t0 < NJ; t0 += BG) {
                f32x4v bb[BG];
#pragma unroll
                for (int u = 0; u < BG; ++u)
                    if (t0 + u < NJ) bb[u] = *reinterpret_cast<const f32x4v*>(p.b2 + 16 * (t0 + u) + 4 * g);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < BG; ++u) {
                    if (t0 + u < NJ) {
                        f32x4v m;
#pragma unroll
                        for (int r = 0; r < 4; ++r) m[r] = accM[t0 + u][r] * inv2 + bb[u][r];
                        *reinterpret_cast<f32x4v*>(Mrow + 16 * (t0 + u) + 4 * g) = m;
                    }
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }

    // ================= phase 3: per head  softmax(scale K_h Q_h^T + M^T) , O^T = V_h^T P^T =================
    const int hd = p.hd;
    const auto gh = G::at(hd);
    const int DT = gh.DT, hdp = gh.hdp, LDV = gh.LDV;           // output d-tiles, padded head dim, stripe row stride
    float* bufV = smem + G::V_OFF;                              // the WHOLE V_h [Skv][LDV], filled during the QK loop
    const int v_per_row = hdp >> 2;                             // float4 per V row
    const int v_total = SKV * v_per_row;
    const int nchq = (hd + 15) / 16;                            // QK^T column chunks
    const int v_share = (v_total + nchq - 1) / nchq;            // float4 of V staged per QK chunk (<= NV_K * NTH)
#pragma unroll 1
    for (int h = 0; h < p.H; ++h) {
        const float* qh = qb + h * hd;
        const float* kh = kb + h * hd;
        const float* vh = vb + h * hd;
        f32x4v accS[NJ];
#pragma unroll
        for (int t = 0; t < NJ; ++t) accS[t] = (f32x4v){0.f, 0.f, 0.f, 0.f};
        {
            Regs<NV_K> rk; Regs<NV_Q> rq; Regs<NV_K> rv;
            auto v_load = [&](int c) {
#pragma unroll
                for (int u = 0; u < NV_K; ++u) {
                    const int f = c * v_share + tid + u * NTH;
                    const int row = f / v_per_row, cq = f - row * v_per_row;
                    f32x4v val = {0.f, 0.f, 0.f, 0.f};
                    if (tid + u * NTH < v_share && f < v_total && 4 * cq < hd)
                        val = *reinterpret_cast<const f32x4v*>(vh + (long)row * D + 4 * cq);
                    rv.v[u] = val;
                }
            };
            auto v_store = [&](int c) {
#pragma unroll
                for (int u = 0; u < NV_K; ++u) {
                    const int f = c * v_share + tid + u * NTH;
                    const int row = f / v_per_row, cq = f - row * v_per_row;
                    if (tid + u * NTH < v_share && f < v_total)
                        *reinterpret_cast<f32x4v*>(bufV + row * LDV + 4 * cq) = rv.v[u];
                }
            };
            km_load<NTH>(rk, kh, D, SKV, 0, hd);
            km_load<NTH>(rq, qh, D, nq, 0, hd);
            km_store<NTH>(rk, bufK(0), LDJ, SKV);
            km_store<NTH>(rq, bufQ(0), LDQ, nq);
            __syncthreads();
#pragma unroll 1
            for (int c = 0; c < nchq; ++c) {
                const int cur = c & 1;
                v_load(c);
                if (c + 1 < nchq) {
                    km_load<NTH>(rk, kh, D, SKV, 16 * (c + 1), hd);
                    km_load<NTH>(rq, qh, D, nq, 16 * (c + 1), hd);
                }
                if (active) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const float bq = bufQ(cur)[(4 * s + g) * LDQ + 16 * wave + r16];
#pragma unroll
                        for (int t = 0; t < NJ; ++t)
                            accS[t] = MFMA16(bufK(cur)[(4 * s + g) * LDJ + 16 * t + r16], bq, accS[t]);
                    }
                }
                v_store(c);
                if (c + 1 < nchq) {
                    km_store<NTH>(rk, bufK(cur ^ 1), LDJ, SKV);
                    km_store<NTH>(rq, bufQ(cur ^ 1), LDQ, nq);
                }
                __syncthreads();
            }
        }
        // softmax over the keys: 4*NJ in-lane values, then the 4 lane groups (xor 16, xor 32)
        float mx = -INFINITY;
        {
            // own writes of this thread; the pointer is laundered so that the compiler re-loads the tile per
            // head instead of forwarding the stored values (which would keep 4*NJ registers live)
            const float* Mrow = p.Mk + ((long)b * p.Sq + (active ? iq : q0)) * p.Skv;
            asm volatile("" : "+v"(Mrow));
#pragma unroll
            for (int t = 0; t < NJ; ++t) {
                const f32x4v m = *reinterpret_cast<const f32x4v*>(Mrow + 16 * t + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    accS[t][r] = accS[t][r] * p.scale + m[r];
                    mx = fmaxf(mx, accS[t][r]);
                }
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < NJ; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                accS[t][r] = __expf(accS[t][r] - mx);        // v_exp_f32 form: arguments <= 0, error ~1e-6 relative
                sum += accS[t][r];
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.0f / sum;
        // row-LSE mode: what the backward needs to rebuild this row's probabilities (one lane group per query)
        if (!LEAN && active && p.lse && g == 0) p.lse[((long)b * p.H + h) * p.Sq + iq] = mx + logf(sum);
#pragma unroll
        for (int t = 0; t < NJ; ++t) accS[t] = accS[t] * inv;
        if (!LEAN && active && p.P) {
            float* Prow = p.P + (((long)b * p.H + h) * p.Sq + iq) * p.Skv;
#pragma unroll
            for (int t = 0; t < NJ; ++t) *reinterpret_cast<f32x4v*>(Prow + 16 * t + 4 * g) = accS[t];
        }
        // O^T[d,i] = sum_j V_h[j,d] P^T[j,i]   (V_h complete in LDS since the last barrier of the QK loop)
        if (active) {
            float* orow = p.out + ((long)b * p.Sq + iq) * D + h * hd;
#pragma unroll 1
            for (int d = 0; d < DT; d += 2) {                   // two d-tiles = two independent MFMA chains
                f32x4v accO = {0.f, 0.f, 0.f, 0.f}, accO2 = {0.f, 0.f, 0.f, 0.f};
                const float* vcol = bufV + 16 * d + r16;
                const int d2 = (d + 1 < DT) ? 16 : 0;           // odd DT: the second chain redoes tile d (discarded)
#pragma unroll
                for (int t = 0; t < NJ; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        accO = MFMA16(vcol[(16 * t + 4 * g + r) * LDV], accS[t][r], accO);
                        accO2 = MFMA16(vcol[(16 * t + 4 * g + r) * LDV + d2], accS[t][r], accO2);
                    }
                if (16 * d + 4 * g < hd) *reinterpret_cast<f32x4v*>(orow + 16 * d + 4 * g) = accO;
                if (d + 1 < DT && 16 * (d + 1) + 4 * g < hd)
                    *reinterpret_cast<f32x4v*>(orow + 16 * (d + 1) + 4 * g) = accO2;
            }
        }
        __syncthreads();                                        // bufV / bufK / bufQ are rewritten by the next head
    }
}

// =====================================================================================================
// Backward of the attention core, two kernels with the same tiling/staging as the forward and NO cross-wave
// reductions (the mask-MLP backward stays GEMMs; so do the dR terms, but on the folded route described below):
//   Q side  (queries on the lanes, one wave = 16 queries, all keys on the accumulator rows)
//       dP^T[j,i] = sum_d V_h[j,d] dO_h[i,d]          (same loop as QK^T: V in the K role, dO in the Q role)
//       delta_i   = sum_j P[i,j] dP[i,j]               (in-lane + 2 shuffles)
//       dS        = P o (dP - delta)                   -> written once to HBM for the K/V side
//       dM       += dS                                 (summed over heads in registers)
//       dQ^T[d,i] = scale sum_j K_h[j,d] dS^T[j,i]     (same block as PV: K_h stripe in the V role)
//   KV side (keys on the lanes, one wave = 16 keys, all queries on the accumulator rows)
//       dV^T[d,j] = sum_i dO_h[i,d] P[i,j]             (PV block: dO_h stripe, P tiles as B operand)
//       dK^T[d,j] = scale sum_i Q_h[i,d] dS[i,j]       (PV block: Q_h stripe, dS tiles as B operand)
// Folded route (calm_attention_bwd_front / _back, stored P): dR, the gradient of the raw logits R = Q_all K_all^T shared
// by all heads, enters dQ and dK as dQ_all += dR K_all, dK_all += dR^T Q_all — per head the same contractions as above
// with dR added to the operand:  dQ_h = (scale dS_h + dR) K_h,  dK_h = (scale dS_h + dR)^T Q_h.  dR comes out of the
// caller's mask-MLP backward, which needs dM, so the backward is split around it into three launches:
//   front   attn_bwd_q_kernel<.., DQ = false>   dS, dM                       (the Q side without its dQ block)
//           -- caller: mask-MLP backward, dM -> dR --
//   back    attn_bwd_kv_kernel<.., FOLD = true>  dV; dK^T = sum_i Q_h fmaf(scale, dS, dR)
//           attn_bwd_dq_kernel                   dQ^T = sum_j K_h fmaf(scale, dS, dR)^T   (re-reads dS)
// and the two per-image S x D x S GEMMs of the caller are gone.  No kernel's staging, barriers or loops differ from the
// two-launch form.
// =====================================================================================================
struct AttnBwdP {
    const float* q; const float* k; const float* v; const float* dout;
    const float* P;              // [B,H,Sq,Skv] probabilities saved by the forward
    float* dS;                   // [B,H,Sq,Skv] written by the Q side, read by the KV side
    float* dq; float* dk; float* dv;
    float* dM;                   // [B,Sq,Skv]
    int B, Sq, Skv, H, hd;
    float scale;
    const float* Mk;             // [B,Sq,Skv] mask  } row-LSE mode only (attn_bwd_q_kernel<.., true>): P is then
    const float* lse;            // [B,H,Sq]         } scratch that the Q side fills itself before it reads it
    const float* dR;             // [B,Sq,Skv] gradient of the raw logits R — folded route only (back kernels)
};

// LSE = true: the forward saved no probabilities.  Each head starts by rebuilding its P rows from q, k, the mask and
// the row log-sum-exp — S^T = K_h Q_h^T with the forward's staging and MFMA loop, P = exp(scale S + M - lse): no
// maximum, no sum, no division — and writes them to p.P, where the unchanged body below and the K/V side read them.
// Only accS is live in that prologue (accD does not exist yet), so the body's register budget is the stored-P one.
//
// DQ = false: the front kernel of the folded route.  dR does not exist yet (it comes out of the mask-MLP backward, which
// needs this kernel's dM), so dQ is left to attn_bwd_dq_kernel: the K_h stripe staging and the dQ MFMA block are compiled
// out, q and k are never read and the launch has no stripe in LDS (AttGeo::bwd_front_bytes).  dS and dM go through the
// same instructions in the same order as with DQ = true and are bit-identical to it.
template <int NJ, int NW, bool LSE, bool DQ>
__global__ __launch_bounds__(64 * NW) void attn_bwd_q_kernel(const AttnBwdP p) {
    static_assert(DQ || !LSE, "the row-LSE prologue reads q and k: it has no front-only form");
    constexpr int NTH = 64 * NW;
    constexpr int NV_K = (NJ + NW - 1) / NW;   // float4 per thread for a [16*NJ x 16] chunk
    extern __shared__ __attribute__((aligned(16))) float smem[];
    typedef AttGeo<NJ, NW> G;
    constexpr int SKV = G::SKV, LDJ = G::LDJ, TQ = G::TQ, LDQ = G::LDQ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * TQ;
    const int nq = min(TQ, p.Sq - q0);
    const bool active = 16 * wave < nq;
    const int iq = q0 + 16 * wave + r16;
    const int D = p.H * p.hd;
    const int hd = p.hd;
    const auto gh = G::at(hd);
    const int DT = gh.DT, hdp = gh.hdp, LDV = gh.LDV;
    auto bufK = [&](int i) { return G::buf_k(smem, i); };
    auto bufQ = [&](int i) { return G::buf_q(smem, i); };
    float* bufV = smem + G::V_OFF;                              // whole K_h stripe for the dQ block
    const int v_per_row = hdp >> 2, v_total = SKV * v_per_row;
    const int nchq = (hd + 15) / 16;
    const int v_share = (v_total + nchq - 1) / nchq;

    const float* dob = p.dout + ((long)b * p.Sq + q0) * D;
    const float* qb = p.q + ((long)b * p.Sq + q0) * D;
    const float* kb = p.k + (long)b * p.Skv * D;
    const float* vb = p.v + (long)b * p.Skv * D;

    f32x4v accM[NJ];
#pragma unroll
    for (int t = 0; t < NJ; ++t) accM[t] = (f32x4v){0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int h = 0; h < p.H; ++h) {
        const float* doh = dob + h * hd;
        const float* kh = kb + h * hd;
        const float* vh = vb + h * hd;
        const long prow = (((long)b * p.H + h) * p.Sq + (active ? iq : q0)) * p.Skv;
        if constexpr (LSE) {
            const float* qh = qb + h * hd;
            f32x4v accS[NJ];
#pragma unroll
            for (int t = 0; t < NJ; ++t) accS[t] = (f32x4v){0.f, 0.f, 0.f, 0.f};
            {
                Regs<NV_K> rk; Regs<NV_Q> rq;
                km_load<NTH>(rk, kh, D, SKV, 0, hd);
                km_load<NTH>(rq, qh, D, nq, 0, hd);
                km_store<NTH>(rk, bufK(0), LDJ, SKV);
                km_store<NTH>(rq, bufQ(0), LDQ, nq);
                __syncthreads();
#pragma unroll 1
                for (int c = 0; c < nchq; ++c) {
                    const int cur = c & 1;
                    if (c + 1 < nchq) {
                        km_load<NTH>(rk, kh, D, SKV, 16 * (c + 1), hd);
                        km_load<NTH>(rq, qh, D, nq, 16 * (c + 1), hd);
                    }
                    if (active) {
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const float bq = bufQ(cur)[(4 * s + g) * LDQ + 16 * wave + r16];
#pragma unroll
                            for (int t = 0; t < NJ; ++t)
                                accS[t] = MFMA16(bufK(cur)[(4 * s + g) * LDJ + 16 * t + r16], bq, accS[t]);
                        }
                    }
                    if (c + 1 < nchq) {
                        km_store<NTH>(rk, bufK(cur ^ 1), LDJ, SKV);
                        km_store<NTH>(rq, bufQ(cur ^ 1), LDQ, nq);
                    }
                    __syncthreads();
                }
            }
            // the logits exactly as the forward rounds them (scale S + M), then exp(. - lse) <= 1 up to rounding
            const float* Mrow = p.Mk + ((long)b * p.Sq + (active ? iq : q0)) * p.Skv + 4 * g;
            const float l = p.lse[((long)b * p.H + h) * p.Sq + (active ? iq : q0)];
            float* Pw = const_cast<float*>(p.P) + prow + 4 * g;
            constexpr int MG = 4;                              // mask tiles requested four at a time, as P below
#pragma unroll
            for (int t0 = 0; t0 < NJ; t0 += MG) {
                f32x4v m[MG];
#pragma unroll
                for (int u = 0; u < MG; ++u)
                    if (t0 + u < NJ) m[u] = *reinterpret_cast<const f32x4v*>(Mrow + 16 * (t0 + u));
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < MG; ++u) {
                    if (t0 + u < NJ) {
                        const int t = t0 + u;
#pragma unroll
                        for (int r = 0; r < 4; ++r) accS[t][r] = __expf(accS[t][r] * p.scale + m[u][r] - l);
                        if (active) *reinterpret_cast<f32x4v*>(Pw + 16 * t) = accS[t];
                    }
                }
            }
            // the body re-reads these rows: same lanes, same addresses, so program order is all it takes — the drain
            // (and its "memory" clobber) keeps both the compiler and the __restrict__ loads below behind the stores
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        f32x4v accD[NJ];
#pragma unroll
        for (int t = 0; t < NJ; ++t) accD[t] = (f32x4v){0.f, 0.f, 0.f, 0.f};
        {
            Regs<NV_K> rk; Regs<NV_Q> rq; Regs<NV_K> rv;
            auto s_load = [&](int c) {                         // K_h stripe, a share per chunk iteration
#pragma unroll
                for (int u = 0; u < NV_K; ++u) {
                    const int f = c * v_share + tid + u * NTH;
                    const int row = f / v_per_row, cq = f - row * v_per_row;
                    f32x4v val = {0.f, 0.f, 0.f, 0.f};
                    if (tid + u * NTH < v_share && f < v_total && 4 * cq < hd)
                        val = *reinterpret_cast<const f32x4v*>(kh + (long)row * D + 4 * cq);
                    rv.v[u] = val;
                }
            };
            auto s_store = [&](int c) {
#pragma unroll
                for (int u = 0; u < NV_K; ++u) {
                    const int f = c * v_share + tid + u * NTH;
                    const int row = f / v_per_row, cq = f - row * v_per_row;
                    if (tid + u * NTH < v_share && f < v_total)
                        *reinterpret_cast<f32x4v*>(bufV + row * LDV + 4 * cq) = rv.v[u];
                }
            };
            km_load<NTH>(rk, vh, D, SKV, 0, hd);
            km_load<NTH>(rq, doh, D, nq, 0, hd);
            km_store<NTH>(rk, bufK(0), LDJ, SKV);
            km_store<NTH>(rq, bufQ(0), LDQ, nq);
            __syncthreads();
#pragma unroll 1
            for (int c = 0; c < nchq; ++c) {
                const int cur = c & 1;
                if constexpr (DQ) s_load(c);
                if (c + 1 < nchq) {
                    km_load<NTH>(rk, vh, D, SKV, 16 * (c + 1), hd);
                    km_load<NTH>(rq, doh, D, nq, 16 * (c + 1), hd);
                }
                if (active) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const float bq = bufQ(cur)[(4 * s + g) * LDQ + 16 * wave + r16];
#pragma unroll
                        for (int t = 0; t < NJ; ++t)
                            accD[t] = MFMA16(bufK(cur)[(4 * s + g) * LDJ + 16 * t + r16], bq, accD[t]);
                    }
                }
                if constexpr (DQ) s_store(c);
                if (c + 1 < nchq) {
                    km_store<NTH>(rk, bufK(cur ^ 1), LDJ, SKV);
                    km_store<NTH>(rq, bufQ(cur ^ 1), LDQ, nq);
                }
                __syncthreads();
            }
        }
        // delta, dS = P o (dP - delta); P is read twice (second time from L2) instead of being held in registers.
        // P and dS through __restrict__ locals: with the struct's plain pointers the compiler had to assume that the dS
        // store of tile t may alias the P load of tile t + 1 and put `s_waitcnt vmcnt(0)` between them (ISA, round 4:
        // 18-24 of the kernel's 26-35 global loads were followed by a full drain) — one exposed L2 round trip per key tile
        // and head.
        const float* __restrict__ Prow = p.P + prow + 4 * g;
        float* __restrict__ dSrow = p.dS + prow + 4 * g;
        // ... and in GROUPS of PG tiles requested together: left to itself the compiler reuses one register quad for all
        // NJ loads of a loop — load, s_waitcnt vmcnt(0), use, eleven times over — i.e. 2 NJ exposed round trips per head
        constexpr int PG = 4;
        float part = 0.f;
#pragma unroll
        for (int t0 = 0; t0 < NJ; t0 += PG) {
            f32x4v pv[PG];
#pragma unroll
            for (int u = 0; u < PG; ++u)
                if (t0 + u < NJ) pv[u] = *reinterpret_cast<const f32x4v*>(Prow + 16 * (t0 + u));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < PG; ++u)
                if (t0 + u < NJ)
#pragma unroll
                    for (int r = 0; r < 4; ++r) part += pv[u][r] * accD[t0 + u][r];
        }
        part += __shfl_xor(part, 16, 64);
        part += __shfl_xor(part, 32, 64);
#pragma unroll
        for (int t0 = 0; t0 < NJ; t0 += PG) {
            f32x4v pv[PG];
#pragma unroll
            for (int u = 0; u < PG; ++u)
                if (t0 + u < NJ) pv[u] = *reinterpret_cast<const f32x4v*>(Prow + 16 * (t0 + u));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < PG; ++u) {
                if (t0 + u < NJ) {
                    const int t = t0 + u;
#pragma unroll
                    for (int r = 0; r < 4; ++r) accD[t][r] = pv[u][r] * (accD[t][r] - part);
                    accM[t] = accM[t] + accD[t];
                    if (active) *reinterpret_cast<f32x4v*>(dSrow + 16 * t) = accD[t];
                }
            }
        }
        // dQ^T[d,i] = scale * sum_j K_h[j,d] dS^T[j,i]
        if (DQ && active) {
            float* qrow = p.dq + ((long)b * p.Sq + iq) * D + h * hd;
#pragma unroll 1
            for (int d = 0; d < DT; d += 2) {
                f32x4v accO = {0.f, 0.f, 0.f, 0.f}, accO2 = {0.f, 0.f, 0.f, 0.f};
                const float* kcol = bufV + 16 * d + r16;
                const int d2 = (d + 1 < DT) ? 16 : 0;
#pragma unroll
                for (int t = 0; t < NJ; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        accO = MFMA16(kcol[(16 * t + 4 * g + r) * LDV], accD[t][r], accO);
                        accO2 = MFMA16(kcol[(16 * t + 4 * g + r) * LDV + d2], accD[t][r], accO2);
                    }
                if (16 * d + 4 * g < hd) *reinterpret_cast<f32x4v*>(qrow + 16 * d + 4 * g) = accO * p.scale;
                if (d + 1 < DT && 16 * (d + 1) + 4 * g < hd)
                    *reinterpret_cast<f32x4v*>(qrow + 16 * (d + 1) + 4 * g) = accO2 * p.scale;
            }
        }
        __syncthreads();
    }
    if (active) {
        float* mrow = p.dM + ((long)b * p.Sq + iq) * p.Skv;
#pragma unroll
        for (int t = 0; t < NJ; ++t) *reinterpret_cast<f32x4v*>(mrow + 16 * t + 4 * g) = accM[t];
    }
}

// [rows x hd] stripe of one head (row stride D) -> bufV [rows][LDV], four 16-byte loads in flight per thread and trip: as
// a rolled load -> store loop every trip waited out a full memory round trip (6-8 per stripe, two stripes per head)
// (the geometry by reference, as the kernels' lambdas captured it: by value the key/value side compiles to one VGPR more)
template <int NTH>
__device__ __forceinline__ void stage_stripe(float* const& bufV, const float* src, const int& tid, const int& D,
                                             const int& hd, const int& v_per_row, const int& v_total, const int& LDV) {
    constexpr int SB = 4;
#pragma unroll 1
    for (int f0 = tid; f0 < v_total; f0 += SB * NTH) {
        f32x4v val[SB];
#pragma unroll
        for (int u = 0; u < SB; ++u) {
            const int f = f0 + u * NTH;
            const int row = f / v_per_row, cq = f - row * v_per_row;
            val[u] = (f32x4v){0.f, 0.f, 0.f, 0.f};
            if (f < v_total && 4 * cq < hd) val[u] = *reinterpret_cast<const f32x4v*>(src + (long)row * D + 4 * cq);
        }
#pragma unroll
        for (int u = 0; u < SB; ++u) {
            const int f = f0 + u * NTH;
            const int row = f / v_per_row, cq = f - row * v_per_row;
            if (f < v_total) *reinterpret_cast<f32x4v*>(bufV + row * LDV + 4 * cq) = val[u];
        }
    }
}

// NI = query tiles (accumulator rows), one wave = 16 keys on the lanes.
//
// FOLD = true (folded route, launched after the mask-MLP backward): dK_h = (scale dS_h + dR)^T Q_h — the dR^T Q product
// of the caller rides on the contraction this kernel performs anyway.  The operand tile becomes fmaf(scale, dS, dR) and
// the contraction is stored unscaled.  The dR tile (the dS addressing without the head term) is the same for every head
// and is held in 4 NI registers across the head loop.  VGPRs / scratch bytes / waves per SIMD of the compiler's resource
// report (hipcc -Rpass-analysis=kernel-resource-usage), NI = 2, 3, 5, 8, 11, 14:
//   FOLD = false             70   82  105  141  168  214    scratch 28 at NI = 11    occupancy 5 5 4 3 3 2   (the parent's)
//   FOLD, dR held            60   68   83  107  131  156    no scratch               occupancy 7 6 5 4 3 3
//   FOLD, dR reloaded/head   52   56   66   92  116  144    no scratch               occupancy 8 7 7 5 4 3   (tried, not kept)
// Held: it fits everywhere without scratch and at no fewer waves than the unfolded form, the workgroups per CU are then
// set by the LDS stripe and the workgroup size (NI >= 8: held and reloaded both give 2, 1, 1), and it saves 4 NI L2 loads
// per head whose latency nothing in this kernel's serial phases would cover.
template <int NI, int NW, bool FOLD>
__global__ __launch_bounds__(64 * NW) void attn_bwd_kv_kernel(const AttnBwdP p) {
    constexpr int NTH = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    typedef AttGeo<NI, NW> G;                                   // the same geometry with the axes swapped
    constexpr int SQ = G::SKV, TK = G::TQ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    const int k0 = blockIdx.x * TK;
    const int nk = min(TK, p.Skv - k0);
    const bool active = 16 * wave < nk;
    const int jk = k0 + 16 * wave + r16;                        // this lane's key
    const int D = p.H * p.hd;
    const int hd = p.hd;
    const auto gh = G::at(hd);
    const int DT = gh.DT, hdp = gh.hdp, LDV = gh.LDV;
    float* bufV = smem;                                         // whole dO_h / Q_h stripe [Sq][LDV]
    const int v_per_row = hdp >> 2, v_total = SQ * v_per_row;
    const float* qb = p.q + (long)b * p.Sq * D;
    const float* dob = p.dout + (long)b * p.Sq * D;

    auto stage = [&](const float* src) { stage_stripe<NTH>(bufV, src, tid, D, hd, v_per_row, v_total, LDV); };
    auto contract = [&](const f32x4v (&X)[NI], float* out_row, float scale) {   // out^T[d,j] = sum_i stripe[i,d] X[i,j]
#pragma unroll 1
        for (int d = 0; d < DT; d += 2) {
            f32x4v accO = {0.f, 0.f, 0.f, 0.f}, accO2 = {0.f, 0.f, 0.f, 0.f};
            const float* col = bufV + 16 * d + r16;
            const int d2 = (d + 1 < DT) ? 16 : 0;
#pragma unroll
            for (int t = 0; t < NI; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    accO = MFMA16(col[(16 * t + 4 * g + r) * LDV], X[t][r], accO);
                    accO2 = MFMA16(col[(16 * t + 4 * g + r) * LDV + d2], X[t][r], accO2);
                }
            if (16 * d + 4 * g < hd) *reinterpret_cast<f32x4v*>(out_row + 16 * d + 4 * g) = accO * scale;
            if (d + 1 < DT && 16 * (d + 1) + 4 * g < hd)
                *reinterpret_cast<f32x4v*>(out_row + 16 * (d + 1) + 4 * g) = accO2 * scale;
        }
    };

    // FOLD: the P, dS and dR elements of a lane sit at the same 4 NI offsets from three bases that are uniform over the
    // workgroup.  The offsets do not depend on the head, and left visible the compiler computes them all ahead of the head
    // loop and keeps them live across it as 64-bit values — 8 NI registers, which is why the unfolded form sits at its
    // register ceiling from NI = 11 on.  Here the row index is made opaque at the head of each load phase, so the offsets
    // are rebuilt per load (two integer operations) and their registers are free again once the load has left.
    const unsigned col = active ? jk : k0, skv = p.Skv;
    auto rows = [&]() -> unsigned {
        unsigned g4 = 4 * g;
        asm volatile("" : "+v"(g4));
        return g4;
    };
    auto at = [&](const float* __restrict__ base, int t, int r, unsigned g4) -> float {
        return base[(16 * t + r + g4) * skv + col];
    };
    f32x4v dR[FOLD ? NI : 1];
    if constexpr (FOLD) {
        const float* __restrict__ dRb = p.dR + (long)b * p.Sq * p.Skv;
        const unsigned g4 = rows();
#pragma unroll
        for (int t = 0; t < NI; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) dR[t][r] = at(dRb, t, r, g4);
    }

#pragma unroll 1
    for (int h = 0; h < p.H; ++h) {
        const long base = ((long)b * p.H + h) * p.Sq * p.Skv + (active ? jk : k0);
        const float* __restrict__ Ph = p.P + ((long)b * p.H + h) * p.Sq * p.Skv;
        const float* __restrict__ dSh = p.dS + ((long)b * p.H + h) * p.Sq * p.Skv;
        f32x4v X[NI];
        // P tiles [i rows, key lanes]: 16 consecutive keys = one 64-byte segment per row
        unsigned g4 = FOLD ? rows() : 0;
#pragma unroll
        for (int t = 0; t < NI; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                X[t][r] = FOLD ? at(Ph, t, r, g4) : p.P[base + (long)(16 * t + 4 * g + r) * p.Skv];
        stage(dob + h * hd);
        __syncthreads();
        if (active) contract(X, p.dv + ((long)b * p.Skv + jk) * D + h * hd, 1.0f);
        __syncthreads();
        if constexpr (FOLD) g4 = rows();
#pragma unroll
        for (int t = 0; t < NI; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                X[t][r] = FOLD ? at(dSh, t, r, g4) : p.dS[base + (long)(16 * t + 4 * g + r) * p.Skv];
        stage(qb + h * hd);
        if constexpr (FOLD) {
#pragma unroll
            for (int t = 0; t < NI; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) X[t][r] = fmaf(p.scale, X[t][r], dR[t][r]);
        }
        __syncthreads();
        if (active) contract(X, p.dk + ((long)b * p.Skv + jk) * D + h * hd, FOLD ? 1.0f : p.scale);
        __syncthreads();
    }
}

// dQ of the folded route, launched after the mask-MLP backward: dQ_h = (scale dS_h + dR) K_h — the dR K product of the
// caller rides on the dQ block that used to close attn_bwd_q_kernel.  Query-tiled exactly like the Q side (one wave = 16
// queries on the lanes, rows prow + 4g + 16t): the tile's dR rows are loaded once into NJ register quads, each head
// requests its dS rows (all NJ quads in flight, ahead of the staging), stages the K_h stripe, forms
// accD = fmaf(scale, dS, dR) and runs the Q side's dQ^T MFMA block; dq is stored without the scale.
template <int NJ, int NW>
__global__ __launch_bounds__(64 * NW) void attn_bwd_dq_kernel(const AttnBwdP p) {
    constexpr int NTH = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    typedef AttGeo<NJ, NW> G;
    constexpr int SKV = G::SKV, TQ = G::TQ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * TQ;
    const int nq = min(TQ, p.Sq - q0);
    const bool active = 16 * wave < nq;
    const int iq = q0 + 16 * wave + r16;
    const int D = p.H * p.hd;
    const int hd = p.hd;
    const auto gh = G::at(hd);
    const int DT = gh.DT, hdp = gh.hdp, LDV = gh.LDV;
    float* bufV = smem;                                         // whole K_h stripe [Skv][LDV]
    const int v_per_row = hdp >> 2, v_total = SKV * v_per_row;
    const float* kb = p.k + (long)b * p.Skv * D;

    const float* __restrict__ dRrow = p.dR + ((long)b * p.Sq + (active ? iq : q0)) * p.Skv + 4 * g;
    f32x4v accR[NJ];
#pragma unroll
    for (int t = 0; t < NJ; ++t) accR[t] = *reinterpret_cast<const f32x4v*>(dRrow + 16 * t);

#pragma unroll 1
    for (int h = 0; h < p.H; ++h) {
        const long prow = (((long)b * p.H + h) * p.Sq + (active ? iq : q0)) * p.Skv;
        const float* __restrict__ dSrow = p.dS + prow + 4 * g;
        f32x4v accD[NJ];
#pragma unroll
        for (int t = 0; t < NJ; ++t) accD[t] = *reinterpret_cast<const f32x4v*>(dSrow + 16 * t);
        __builtin_amdgcn_sched_barrier(0);                      // the requests leave before the staging, not after it
        stage_stripe<NTH>(bufV, kb + h * hd, tid, D, hd, v_per_row, v_total, LDV);
#pragma unroll
        for (int t = 0; t < NJ; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) accD[t][r] = fmaf(p.scale, accD[t][r], accR[t][r]);
        __syncthreads();
        // dQ^T[d,i] = sum_j K_h[j,d] (scale dS + dR)^T[j,i]
        if (active) {
            float* qrow = p.dq + ((long)b * p.Sq + iq) * D + h * hd;
#pragma unroll 1
            for (int d = 0; d < DT; d += 2) {
                f32x4v accO = {0.f, 0.f, 0.f, 0.f}, accO2 = {0.f, 0.f, 0.f, 0.f};
                const float* kcol = bufV + 16 * d + r16;
                const int d2 = (d + 1 < DT) ? 16 : 0;
#pragma unroll
                for (int t = 0; t < NJ; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        accO = MFMA16(kcol[(16 * t + 4 * g + r) * LDV], accD[t][r], accO);
                        accO2 = MFMA16(kcol[(16 * t + 4 * g + r) * LDV + d2], accD[t][r], accO2);
                    }
                if (16 * d + 4 * g < hd) *reinterpret_cast<f32x4v*>(qrow + 16 * d + 4 * g) = accO;
                if (d + 1 < DT && 16 * (d + 1) + 4 * g < hd)
                    *reinterpret_cast<f32x4v*>(qrow + 16 * (d + 1) + 4 * g) = accO2;
            }
        }
        __syncthreads();
    }
}

// =====================================================================================================
// Ring form of the two back kernels of the folded route.  In the stripe form above a head's whole [S][hd + 4] stripe sits
// in one LDS buffer that cannot be refilled while the contraction reads it: stage, barrier, contract, barrier — the
// global loads of every stripe are exposed.  Here the stripe goes through LDS in the unit the contraction's d loop consumes
// anyway, a slab of 32 columns (two d-tiles; the last slab of an odd DT holds one, with the stripe form's d2 = 0 for the
// second chain), and the slabs of ALL stripes of the workgroup form one sequence — key side: dO_0, Q_0, dO_1, Q_1, ...;
// dQ side: K_0, K_1, ... — that runs through two slots.  Step s:
//   1. request slab s + 1 from global memory into registers (4 or 2 float4 per thread)
//   2. contract slab s out of slot s & 1
//   3. write the registers to slot (s + 1) & 1
//   4. one barrier
// The slot written in step s was last read in step s - 1, behind that step's barrier, so one barrier per step is enough.
// Each output element is the same chain of MFMAs over the same operands in the same order as in the stripe form: dq, dk
// and dv are bit-identical to it.  The register tiles (P / dS / dR) keep their loads and their place in the head.
// =====================================================================================================
template <int NTH, class G>
struct Slab {
    static constexpr int V_TOTAL = 8 * G::SKV;                 // a slab row is 8 float4: row = f >> 3, cq = f & 7
    static constexpr int NV = V_TOTAL / NTH;
    static_assert(V_TOTAL % NTH == 0, "every thread moves the same number of float4: no bounds test on f");
    f32x4v v[NV];
    // columns c0 .. c0 + 31 of the [SKV x hd] stripe at src (row stride D).  No branch around a load (the compiler
    // drains the whole memory queue where loads sit in conditional blocks): a column >= hd requests column 0 of its row
    // instead, and store() writes the zero
    __device__ __forceinline__ void load(const float* __restrict__ src, int D, int hd, int c0) {
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int f = threadIdx.x + u * NTH;
            const int row = f >> 3, c = c0 + 4 * (f & 7);
            v[u] = *reinterpret_cast<const f32x4v*>(src + (long)row * D + (c < hd ? c : 0));
        }
    }
    __device__ __forceinline__ void store(float* slot, int hd, int c0) const {
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int f = threadIdx.x + u * NTH;
            const int row = f >> 3, cq = f & 7;
            const f32x4v zero = {0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4v*>(slot + row * G::LDS_SLAB + 4 * cq) = c0 + 4 * cq < hd ? v[u] : zero;
        }
    }
};

// out^T[d .. d + 1 tiles, lane] = sum_i slab[i, .] X[i, lane]: the body of the stripe form's d loop on one slab, in two
// halves — the caller writes the next slab to LDS between them, so that the write waits for the slab's loads alone and
// not for the output stores behind them in the memory queue
struct SlabAcc { f32x4v o, o2; };
template <class G>
__device__ __forceinline__ SlabAcc slab_contract(const float* slot, const f32x4v (&X)[G::NJ], int d, int DT, int r16, int g) {
    constexpr int LD = G::LDS_SLAB;
    f32x4v accO = {0.f, 0.f, 0.f, 0.f}, accO2 = {0.f, 0.f, 0.f, 0.f};
    const float* col = slot + r16;
    const int d2 = (d + 1 < DT) ? 16 : 0;
#pragma unroll
    for (int t = 0; t < G::NJ; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            accO = MFMA16(col[(16 * t + 4 * g + r) * LD], X[t][r], accO);
            accO2 = MFMA16(col[(16 * t + 4 * g + r) * LD + d2], X[t][r], accO2);
        }
    return {accO, accO2};
}
__device__ __forceinline__ void slab_out(const SlabAcc& a, float* out_row, int d, int DT, int hd, int g) {
    if (16 * d + 4 * g < hd) *reinterpret_cast<f32x4v*>(out_row + 16 * d + 4 * g) = a.o;
    if (d + 1 < DT && 16 * (d + 1) + 4 * g < hd) *reinterpret_cast<f32x4v*>(out_row + 16 * (d + 1) + 4 * g) = a.o2;
}

// attn_bwd_kv_kernel<NI, NW, FOLD = true> with the dO_h / Q_h stripes through the slab ring
template <int NI, int NW>
__global__ __launch_bounds__(64 * NW) void attn_bwd_kv_ring_kernel(const AttnBwdP p) {
    constexpr int NTH = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    typedef AttGeo<NI, NW> G;                                   // the same geometry with the axes swapped
    static_assert(NI % NW == 0, "Skv = 16 NI keys in whole workgroups: every wave has a key tile");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    const int jk = blockIdx.x * G::TQ + 16 * wave + r16;        // this lane's key
    const int D = p.H * p.hd;
    const int hd = p.hd;
    const int DT = G::at(hd).DT, NS = (DT + 1) >> 1;            // slabs per stripe
    const float* qb = p.q + (long)b * p.Sq * D;
    const float* dob = p.dout + (long)b * p.Sq * D;

    // the opaque row index of the stripe form: the 4 NI tile offsets are rebuilt per load, not held across the head loop
    const unsigned col = jk, skv = p.Skv;
    auto rows = [&]() -> unsigned {
        unsigned g4 = 4 * g;
        asm volatile("" : "+v"(g4));
        return g4;
    };
    auto at = [&](const float* __restrict__ base, int t, int r, unsigned g4) -> float {
        return base[(16 * t + r + g4) * skv + col];
    };
    f32x4v dR[NI];
    {
        const float* __restrict__ dRb = p.dR + (long)b * p.Sq * p.Skv;
        const unsigned g4 = rows();
#pragma unroll
        for (int t = 0; t < NI; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) dR[t][r] = at(dRb, t, r, g4);
    }

    Slab<NTH, G> rs;
    int s = 0;                                                  // step = slab in the workgroup's sequence
    // the NS slabs of the stripe `cur`; the last step requests the first slab of `nxt`.  The very last step of the
    // workgroup has no next stripe and is handed `cur` again: one slab goes to the free slot unread, and the loop keeps a
    // single shape
    auto walk = [&](f32x4v (&X)[NI], const float* cur, const float* nxt, float* out_row, auto fold) {
#pragma unroll 1
        for (int sl = 0; sl < NS; ++sl, ++s) {
            const bool last = sl + 1 == NS;
            const int c0 = last ? 0 : 32 * (sl + 1);
            rs.load(last ? nxt : cur, D, hd, c0);
            __builtin_amdgcn_sched_barrier(0);                  // the requests leave ahead of the contraction ...
            if constexpr (decltype(fold)::value) {
                if (sl == 0) {
#pragma unroll
                    for (int t = 0; t < NI; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) X[t][r] = fmaf(p.scale, X[t][r], dR[t][r]);
                }
            }
            const SlabAcc acc = slab_contract<G>(G::slab_slot(smem, s), X, 2 * sl, DT, r16, g);
            __builtin_amdgcn_sched_barrier(0);                  // ... and are waited for behind it
            rs.store(G::slab_slot(smem, s + 1), hd, c0);
            slab_out(acc, out_row, 2 * sl, DT, hd, g);
            __syncthreads();
        }
    };

    rs.load(dob, D, hd, 0);
    rs.store(G::slab_slot(smem, 0), hd, 0);
    __syncthreads();
#pragma unroll 1
    for (int h = 0; h < p.H; ++h) {
        const float* __restrict__ Ph = p.P + ((long)b * p.H + h) * p.Sq * p.Skv;
        const float* __restrict__ dSh = p.dS + ((long)b * p.H + h) * p.Sq * p.Skv;
        const long orow = ((long)b * p.Skv + jk) * D + h * hd;
        f32x4v X[NI];
        unsigned g4 = rows();
#pragma unroll
        for (int t = 0; t < NI; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) X[t][r] = at(Ph, t, r, g4);
        walk(X, dob + h * hd, qb + h * hd, p.dv + orow, std::false_type{});
        g4 = rows();
#pragma unroll
        for (int t = 0; t < NI; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) X[t][r] = at(dSh, t, r, g4);
        walk(X, qb + h * hd, h + 1 < p.H ? dob + (h + 1) * hd : qb + h * hd, p.dk + orow, std::true_type{});
    }
}

// attn_bwd_dq_kernel<NJ, NW> with the K_h stripes through the slab ring
template <int NJ, int NW>
__global__ __launch_bounds__(64 * NW) void attn_bwd_dq_ring_kernel(const AttnBwdP p) {
    constexpr int NTH = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    typedef AttGeo<NJ, NW> G;
    static_assert(NJ % NW == 0, "Sq = 16 NJ queries in whole workgroups: every wave has a query tile");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    const int iq = blockIdx.x * G::TQ + 16 * wave + r16;
    const int D = p.H * p.hd;
    const int hd = p.hd;
    const int DT = G::at(hd).DT, NS = (DT + 1) >> 1;            // slabs per stripe
    const float* kb = p.k + (long)b * p.Skv * D;

    const float* __restrict__ dRrow = p.dR + ((long)b * p.Sq + iq) * p.Skv + 4 * g;
    f32x4v accR[NJ];
#pragma unroll
    for (int t = 0; t < NJ; ++t) accR[t] = *reinterpret_cast<const f32x4v*>(dRrow + 16 * t);

    Slab<NTH, G> rs;
    rs.load(kb, D, hd, 0);
    rs.store(G::slab_slot(smem, 0), hd, 0);
    __syncthreads();
    int s = 0;                                                  // step = slab in the workgroup's sequence
#pragma unroll 1
    for (int h = 0; h < p.H; ++h) {
        const long prow = (((long)b * p.H + h) * p.Sq + iq) * p.Skv;
        const float* __restrict__ dSrow = p.dS + prow + 4 * g;
        float* qrow = p.dq + ((long)b * p.Sq + iq) * D + h * hd;
        const float* cur = kb + h * hd;
        const float* nxt = h + 1 < p.H ? cur + hd : cur;        // the workgroup's last step: one slab to the free slot, unread
        f32x4v accD[NJ];
#pragma unroll
        for (int t = 0; t < NJ; ++t) accD[t] = *reinterpret_cast<const f32x4v*>(dSrow + 16 * t);
        __builtin_amdgcn_sched_barrier(0);                      // the requests leave before the slab's, not after them
#pragma unroll 1
        for (int sl = 0; sl < NS; ++sl, ++s) {
            const bool last = sl + 1 == NS;
            const int c0 = last ? 0 : 32 * (sl + 1);
            rs.load(last ? nxt : cur, D, hd, c0);
            __builtin_amdgcn_sched_barrier(0);                  // the requests leave ahead of the contraction ...
            if (sl == 0) {
#pragma unroll
                for (int t = 0; t < NJ; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) accD[t][r] = fmaf(p.scale, accD[t][r], accR[t][r]);
            }
            // dQ^T[d,i] = sum_j K_h[j,d] (scale dS + dR)^T[j,i]
            const SlabAcc acc = slab_contract<G>(G::slab_slot(smem, s), accD, 2 * sl, DT, r16, g);
            __builtin_amdgcn_sched_barrier(0);                  // ... and are waited for behind it
            rs.store(G::slab_slot(smem, s + 1), hd, c0);
            slab_out(acc, qrow, 2 * sl, DT, hd, g);
            __syncthreads();
        }
    }
}

// set the dynamic-LDS limit of a kernel, launch it, check the launch
template <class P>
int launch(void (*kernel)(const P), dim3 grid, int threads, size_t lds, hipStream_t s, const P& p) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, s, p);
    CALM_LAUNCH_CHECK();
    return 0;
}

template <class G, bool LSE>
int launch_bwd(const AttnBwdP& p, hipStream_t s) {
    static_assert(G::fwd_bytes(4) <= LDS_MAX, "fits at the smallest head dim; larger ones are checked per launch");
    constexpr int NJ = G::NJ, NW = G::NW;
    const int tiles = p.Sq / 16;
    dim3 grid((tiles + NW - 1) / NW, p.B);
    const int e = launch(&attn_bwd_q_kernel<NJ, NW, LSE, true>, grid, 64 * NW, G::bwd_q_bytes(p.hd), s, p);
    if (e) return e;
    return launch(&attn_bwd_kv_kernel<NJ, NW, false>, grid, 64 * NW, G::bwd_kv_bytes(p.hd), s, p);
}

// the folded route: front (dS, dM) — the caller's mask-MLP backward turns dM into dR — back (dV, folded dK, folded dQ)
template <class G>
int launch_bwd_front(const AttnBwdP& p, hipStream_t s) {
    constexpr int NJ = G::NJ, NW = G::NW;
    dim3 grid((p.Sq / 16 + NW - 1) / NW, p.B);
    return launch(&attn_bwd_q_kernel<NJ, NW, false, false>, grid, 64 * NW, G::bwd_front_bytes(), s, p);
}
// Staging form of the two back kernels (calm_attention_set_option): the table below, or one form forced everywhere.
std::atomic<int>& back_option() {
    static std::atomic<int> opt{CALM_ATTN_BACK_TABLE};
    return opt;
}
// The table: ring where it is measured faster than the stripe at that stage (MI355X, B = 256, kernel trace of both forms in
// one process, us per launch at H = 6; DESIGN.md section 7 "slab ring in the attention backward" has H = 12 as well):
//   key tiles (S, hd)     KV stripe -> ring     dQ stripe -> ring
//   14 (224, 112)            656 -> 473            344 -> 242         ring
//   11 (176, 88)             330 -> 242            172 -> 126         ring
//    8 (128, 64)             114 ->  88             63 ->  50         ring
//    5 (80, 40)               59 ->  44             32 ->  25         ring
//    2, 3 (32, 48)         no stage of a measured model has them: not measured, stripe
template <int NJ> constexpr bool ring_kv_preferred() { return NJ >= 5; }
template <int NJ> constexpr bool ring_dq_preferred() { return NJ >= 5; }

template <class G>
int launch_bwd_back(const AttnBwdP& p, hipStream_t s) {
    constexpr int NJ = G::NJ, NW = G::NW;
    dim3 grid((p.Sq / 16 + NW - 1) / NW, p.B);
    const int mode = back_option().load(std::memory_order_relaxed);
    const bool ring_kv = mode == CALM_ATTN_BACK_TABLE ? ring_kv_preferred<NJ>() : mode == CALM_ATTN_BACK_RING;
    const bool ring_dq = mode == CALM_ATTN_BACK_TABLE ? ring_dq_preferred<NJ>() : mode == CALM_ATTN_BACK_RING;
    const int e = ring_kv ? launch(&attn_bwd_kv_ring_kernel<NJ, NW>, grid, 64 * NW, G::bwd_ring_bytes(), s, p)
                          : launch(&attn_bwd_kv_kernel<NJ, NW, true>, grid, 64 * NW, G::bwd_kv_bytes(p.hd), s, p);
    if (e) return e;
    return ring_dq ? launch(&attn_bwd_dq_ring_kernel<NJ, NW>, grid, 64 * NW, G::bwd_ring_bytes(), s, p)
                   : launch(&attn_bwd_dq_kernel<NJ, NW>, grid, 64 * NW, G::bwd_dq_bytes(p.hd), s, p);
}

template <class G, bool LEAN>
int launch_fwd(const AttnFwdP& p, hipStream_t s) {
    static_assert(G::fwd_bytes(4) <= LDS_MAX, "fits at the smallest head dim; larger ones are checked per launch");
    constexpr int NJ = G::NJ, NW = G::NW;
    const int tiles = p.Sq / 16;
    const size_t lds = G::fwd_bytes(p.hd);
    if (lds > LDS_MAX) return CALM_E_UNSUPP;
    dim3 grid((tiles + NW - 1) / NW, p.B);
    return launch(&attn_fwd_kernel<NJ, NW, LEAN>, grid, 64 * NW, lds, s, p);
}

#ifndef ATT_NW11
#define ATT_NW11 11    // waves per workgroup for the 11-tile (S=176) instantiation: one wave per query tile, a single
#endif                 // pass (A/B: 684 -> 473 us against 6 waves in two passes; 4 waves: slower still)
#ifndef ATT_NW14
#define ATT_NW14 7     // 14-tile (S=224) instantiation
#endif

// THE list of supported shapes: <key tiles, waves per workgroup> (Sq == Skv: the tiles of one image split evenly over
// workgroups of at most 8 waves, but for the two measured exceptions).  f(AttGeo<NJ, NW>{}) for Skv = 16 nj.
template <class F>
int with_geo(int nj, F&& f) {
    switch (nj) {
        case 2: return f(AttGeo<2, 2>{});
        case 3: return f(AttGeo<3, 3>{});
        case 5: return f(AttGeo<5, 5>{});
        case 8: return f(AttGeo<8, 8>{});
        case 11: return f(AttGeo<11, ATT_NW11>{});
        case 14: return f(AttGeo<14, ATT_NW14>{});
    }
    return CALM_E_UNSUPP;
}

int attention_bwd_dispatch(const AttnBwdP& p, bool lse, hipStream_t s) {
    return with_geo(p.Skv / 16, [&](auto g) -> int {
        typedef decltype(g) G;
        return lse ? launch_bwd<G, true>(p, s) : launch_bwd<G, false>(p, s);
    });
}

}  // namespace

extern "C" {

int calm_attention_fwd_supported(int32_t Sq, int32_t Skv, int32_t H, int32_t hd) {
    if (Sq <= 0 || Skv <= 0 || H <= 0 || hd <= 0) return 0;
    if (Sq != Skv || (Sq & 15) || (hd & 3) || hd > 128) return 0;   // every attention of the model has Sq == Skv
    // a listed shape whose whole V_h fits in LDS beside the chunk buffers
    return with_geo(Skv / 16, [&](auto g) -> int { return decltype(g)::fwd_bytes(hd) <= LDS_MAX ? 1 : 0; }) == 1;
}

namespace {
int attention_fwd(const float* q, const float* k, const float* v, const float* w1, const float* b1, const float* s1,
                  const float* w2, const float* b2, const float* s2, float* out, float* R, float* hp, float* hg, float* Mk,
                  float* P, float* lse, int32_t B, int32_t Sq, int32_t Skv, int32_t H, int32_t hd, void* stream) {
    if (!q || !k || !v || !w1 || !b1 || !s1 || !w2 || !b2 || !s2 || !out || !R || !hp || !hg || !Mk || B <= 0)
        return CALM_E_INVAL;
    if (!calm_attention_fwd_supported(Sq, Skv, H, hd)) return CALM_E_UNSUPP;
    if (B > 65535) return CALM_E_UNSUPP;
    AttnFwdP p{q, k, v, w1, b1, s1, w2, b2, s2, out, R, hp, hg, Mk, P, B, Sq, Skv, H, hd, 1.0f / sqrtf((float)hd), lse};
    hipStream_t s = as_stream(stream);
    return with_geo(Skv / 16, [&](auto g) -> int { return launch_fwd<decltype(g), false>(p, s); });
}
}  // namespace

int calm_attention_fwd(const float* q, const float* k, const float* v, const float* w1, const float* b1,
                       const float* s1, const float* w2, const float* b2, const float* s2, float* out, float* R,
                       float* hp, float* hg, float* Mk, float* P, int32_t B, int32_t Sq, int32_t Skv, int32_t H, int32_t hd,
                       void* stream) {
    return attention_fwd(q, k, v, w1, b1, s1, w2, b2, s2, out, R, hp, hg, Mk, P, nullptr, B, Sq, Skv, H, hd, stream);
}

// Row-LSE mode: the same launch with the probabilities left in registers and lse [B,H,Sq] written instead.
int calm_attention_fwd_lse(const float* q, const float* k, const float* v, const float* w1, const float* b1,
                           const float* s1, const float* w2, const float* b2, const float* s2, float* out, float* R,
                           float* hp, float* hg, float* Mk, float* lse, int32_t B, int32_t Sq, int32_t Skv, int32_t H,
                           int32_t hd, void* stream) {
    if (!lse) return CALM_E_INVAL;
    return attention_fwd(q, k, v, w1, b1, s1, w2, b2, s2, out, R, hp, hg, Mk, nullptr, lse, B, Sq, Skv, H, hd, stream);
}

// Lean inference forward: calm_attention_fwd with R, hp, hg, P and lse absent (attn_fwd_kernel<.., LEAN = true>).  Mk stays
// the caller's scratch — the kernel re-reads it per head.  out and Mk are bit-identical to calm_attention_fwd's.
int calm_attention_infer(const float* q, const float* k, const float* v, const float* w1, const float* b1,
                         const float* s1, const float* w2, const float* b2, const float* s2, float* out, float* Mk,
                         int32_t B, int32_t Sq, int32_t Skv, int32_t H, int32_t hd, void* stream) {
    if (!q || !k || !v || !w1 || !b1 || !s1 || !w2 || !b2 || !s2 || !out || !Mk || B <= 0) return CALM_E_INVAL;
    if (!calm_attention_fwd_supported(Sq, Skv, H, hd)) return CALM_E_UNSUPP;
    if (B > 65535) return CALM_E_UNSUPP;
    AttnFwdP p{q, k, v, w1, b1, s1, w2, b2, s2, out, nullptr, nullptr, nullptr, Mk, nullptr, B, Sq, Skv, H, hd,
               1.0f / sqrtf((float)hd), nullptr};
    hipStream_t s = as_stream(stream);
    return with_geo(Skv / 16, [&](auto g) -> int { return launch_fwd<decltype(g), true>(p, s); });
}

// Measured on MI355X (scripts/ab_attn_bwd.py, same process): the two fused launches beat the GEMM composition
// for head dims <= 64 (S=128/80 stages of Small-224, every stage of Base-224: 1.1-1.7x) and tie or lose above
// (hd 112: 1.00x, hd 88: 0.76x), where the per-head GEMMs already fill 128-wide tiles.
int calm_attention_bwd_preferred(int32_t Sq, int32_t Skv, int32_t H, int32_t hd) {
    // measured against the composition of batched GEMMs + softmax_bwd + sum_heads (scripts/ab_attn_bwd.py): faster for
    // head dims <= 64 (1.0-1.6x) and for the 11-tile stage (S=176, hd 88: 0.68 vs 0.77 ms, one wave per key/query
    // tile); at S=224 with hd 112 the composition still wins (1.36 vs 1.43 ms)
    return calm_attention_fwd_supported(Sq, Skv, H, hd) && (hd <= 64 || Skv / 16 == 11);
}

int calm_attention_bwd(const float* q, const float* k, const float* v, const float* dout, const float* P, float* dS,
                       float* dq, float* dk, float* dv, float* dM, int32_t B, int32_t Sq, int32_t Skv, int32_t H,
                       int32_t hd, void* stream) {
    if (!q || !k || !v || !dout || !P || !dS || !dq || !dk || !dv || !dM || B <= 0) return CALM_E_INVAL;
    if (!calm_attention_fwd_supported(Sq, Skv, H, hd)) return CALM_E_UNSUPP;
    if (B > 65535) return CALM_E_UNSUPP;
    AttnBwdP p{q, k, v, dout, P, dS, dq, dk, dv, dM, B, Sq, Skv, H, hd, 1.0f / sqrtf((float)hd), nullptr, nullptr};
    return attention_bwd_dispatch(p, false, as_stream(stream));
}

// The folded route (stored P): calm_attention_bwd split around the caller's mask-MLP backward, so that the two dR
// products ride on the dQ / dK contractions.  front: dS and dM, bit-identical to calm_attention_bwd's.  back, once dR
// [B,Sq,Skv] exists: dV, dK_h = (dS_h / sqrt(hd) + dR)^T Q_h, dQ_h = (dS_h / sqrt(hd) + dR) K_h — written, no atomics.
int calm_attention_bwd_front(const float* v, const float* dout, const float* P, float* dS, float* dM, int32_t B,
                             int32_t Sq, int32_t Skv, int32_t H, int32_t hd, void* stream) {
    if (!v || !dout || !P || !dS || !dM || B <= 0) return CALM_E_INVAL;
    if (!calm_attention_fwd_supported(Sq, Skv, H, hd)) return CALM_E_UNSUPP;
    if (B > 65535) return CALM_E_UNSUPP;
    AttnBwdP p{nullptr, nullptr, v, dout, P, dS, nullptr, nullptr, nullptr, dM, B, Sq, Skv, H, hd,
               1.0f / sqrtf((float)hd), nullptr, nullptr, nullptr};
    hipStream_t s = as_stream(stream);
    return with_geo(Skv / 16, [&](auto g) -> int { return launch_bwd_front<decltype(g)>(p, s); });
}

int calm_attention_bwd_back(const float* q, const float* k, const float* dout, const float* P, const float* dS,
                            const float* dR, float* dq, float* dk, float* dv, int32_t B, int32_t Sq, int32_t Skv,
                            int32_t H, int32_t hd, void* stream) {
    if (!q || !k || !dout || !P || !dS || !dR || !dq || !dk || !dv || B <= 0) return CALM_E_INVAL;
    if (!calm_attention_fwd_supported(Sq, Skv, H, hd)) return CALM_E_UNSUPP;
    if (B > 65535) return CALM_E_UNSUPP;
    AttnBwdP p{q, k, nullptr, dout, P, const_cast<float*>(dS), dq, dk, dv, nullptr, B, Sq, Skv, H, hd,
               1.0f / sqrtf((float)hd), nullptr, nullptr, dR};
    hipStream_t s = as_stream(stream);
    return with_geo(Skv / 16, [&](auto g) -> int { return launch_bwd_back<decltype(g)>(p, s); });
}

// Process-wide switches of the attention launchers, in the style of calm_gemm_set_option: returns the previous value.
int calm_attention_set_option(int32_t option, int32_t value) {
    if (option != CALM_ATTN_OPT_BACK) return CALM_E_INVAL;
    if (value != CALM_ATTN_BACK_TABLE && value != CALM_ATTN_BACK_STRIPE && value != CALM_ATTN_BACK_RING) return CALM_E_INVAL;
    return back_option().exchange(value);
}

// Measured on MI355X (scripts/ab_attn_bwd.py, same process, B = 256; ms per attention block, core + the two dR products,
// the mask-MLP backward between front and back left out as common to both):
//                        today's route + dR GEMMs     front + back    ratio
//   S=224 H=6  hd=112    1.467 (GEMM composition)     1.305           1.12x
//   S=176 H=6  hd=88     0.882 (fused)                0.667           1.32x
//   S=128 H=6  hd=64     0.343 (fused)                0.273           1.26x
//   S=80  H=6  hd=40     0.168 (fused)                0.127           1.33x
//   S=224 H=12 hd=56     1.935 (fused)                1.644           1.18x
//   S=176 H=12 hd=44     1.127 (fused)                0.921           1.22x
//   S=128 H=12 hd=32     0.414 (fused)                0.357           1.16x
//   S=80  H=12 hd=20     0.229 (fused)                0.184           1.25x
// The folded route wins at every measured stage, hd 112 included (there the fused pair + GEMMs takes 1.705), so it is
// preferred wherever the kernels exist.  The key-side-only fold (today's Q side with dQ, folded KV kernel, dR K left a
// GEMM) was not built: even credited with the whole dR^T Q GEMM and no cost at all it would take 1.46 / 0.77 / 0.30 /
// 0.14 ms at the Small-224 stages — behind front + back everywhere.
int calm_attention_bwd_fold_preferred(int32_t Sq, int32_t Skv, int32_t H, int32_t hd) {
    return calm_attention_fwd_supported(Sq, Skv, H, hd) ? 1 : 0;
}

// Row-LSE backward: the caller's scratch holds the two [B,H,Sq,Skv] planes the two launches hand to each other — the
// probabilities rebuilt by the query side, then dS.  Nothing of that size outlives the call.
int64_t calm_attention_bwd_lse_scratch_bytes(int32_t B, int32_t Sq, int32_t Skv, int32_t H, int32_t hd) {
    if (B <= 0 || B > 65535 || !calm_attention_fwd_supported(Sq, Skv, H, hd)) return 0;
    return 2 * (int64_t)sizeof(float) * B * H * Sq * Skv;
}

int calm_attention_bwd_lse(const float* q, const float* k, const float* v, const float* dout, const float* Mk,
                           const float* lse, void* scratch, int64_t scratch_bytes, float* dq, float* dk, float* dv,
                           float* dM, int32_t B, int32_t Sq, int32_t Skv, int32_t H, int32_t hd, void* stream) {
    if (!q || !k || !v || !dout || !Mk || !lse || !scratch || !dq || !dk || !dv || !dM || B <= 0) return CALM_E_INVAL;
    const int64_t need = calm_attention_bwd_lse_scratch_bytes(B, Sq, Skv, H, hd);
    if (need == 0) return CALM_E_UNSUPP;
    if (scratch_bytes < need || (reinterpret_cast<uintptr_t>(scratch) & 15)) return CALM_E_INVAL;
    float* P = static_cast<float*>(scratch);
    float* dS = P + need / (2 * (int64_t)sizeof(float));
    AttnBwdP p{q, k, v, dout, P, dS, dq, dk, dv, dM, B, Sq, Skv, H, hd, 1.0f / sqrtf((float)hd), Mk, lse};
    return attention_bwd_dispatch(p, true, as_stream(stream));
}

}  // extern "C"
