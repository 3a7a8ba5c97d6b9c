// Exact fp32 MFMA kernel family of calm_gemm (dispatcher: gemm.hip; shared pieces: gemm_common.h).
//
// Tile 128x128x16 (4 waves as 2x2, each 64x64 = 2x2 v_mfma_f32_32x32x2_f32 accumulators) or 128x96x16 (4x1 waves,
// 1x3 accumulators) per 256-thread workgroup.  Both operands are staged K-MAJOR in LDS ([k][row], row stride 132 floats): fragment
// reads are then one conflict-free ds_read_b32 per MFMA operand for every source layout, and the
// four source layouts (k- or row-contiguous A and B) only differ in the global->register->LDS
// staging.  fp32 MFMA issues every 64 cycles per SIMD, so LDS/VALU work hides under it; the loop is
// a register-prefetch double buffer (global loads of tile t+1 issued before the MFMAs of tile t).
// Workgroup ids are remapped so that consecutive tiles (n fastest: they share an A panel) land on
// the same XCD / L2.
// A second tile shape, 64 x (16 nb) x 16 on v_mfma_f32_16x16x4_f32 (gemm_f32_t64_kernel, below), serves the launches
// whose dimensions are multiples of 16 but not of 32 / 96 and those with too few 128-row tiles to fill the chip.
#include "gemm_common.h"

namespace calm_gemm_detail {

constexpr int LDT = 132;
constexpr int NREG = BK / 2;     // staging floats per thread per operand (128 rows x BK / 256 threads)

// 16-byte staging with a per-thread cursor: the row part of every address is computed once per (tile, batch entry),
// the k-loop only advances the pointers.  Rows past the tile (edge tiles, and rows 96..127 of the 128-row thread map
// on a 96-row B tile) are CLAMPED to the tile's last row instead of masked: they only feed output rows / columns
// that are never stored, so the loads stay unconditional (no exec masking, no zero fill).  Only a partial last
// k-block (K % BK != 0) takes the masked form.
// RP: rows of the thread map — 128 (the 128-row tiles, and B images of 80..128 columns of the 64-row tiles) or 64;
// ROWS <= RP rows of it are stored.
template <bool KC, int ROWS, int RP = 128>
struct OperandCursor {
    static constexpr int NR = RP * BK / NTHREADS;      // staging floats per thread
    static constexpr int TPR = RP / 4;                 // row-contiguous operands: threads per k-row (16-byte vectors)
    const float* base;               // uniform (SGPR pair): tile origin at the current k-block
    unsigned off[NR / 4];            // per-thread byte offsets from it (constant over the k-loop)
    long step;
    __device__ __forceinline__ void init(const float* origin, long rs, long cs, int row0, int nrows_all, int k0) {
        const int tid = threadIdx.x;
        const int last = min(nrows_all - row0, ROWS) - 1;        // last live row of the tile, tile-local
        if constexpr (KC) {
            constexpr int KQ = BK / 4, RPP = NTHREADS / KQ;
            base = origin + (long)row0 * rs + k0;
#pragma unroll
            for (int i = 0; i < NR / 4; ++i)
                off[i] = (unsigned)(min((tid / KQ) + RPP * i, last) * rs + 4 * (tid % KQ)) * 4u;
            step = BK;
        } else {
            base = origin + (long)k0 * cs + row0;
            const int row = min(4 * (tid % TPR), last & ~3);     // rows come in aligned groups of 4 (M % 4 == 0)
#pragma unroll
            for (int i = 0; i < NR / 4; ++i) off[i] = (unsigned)(((tid / TPR) + (NTHREADS / TPR) * i) * cs + row) * 4u;
            step = BK * cs;
        }
    }
    // k_left = K - k0 (> 0).  FULL: K is a whole number of k-blocks — the loads are unconditional (the kernel holds
    // one copy of its k-loop per case: with a run-time choice in one loop the compiler folds both forms into the
    // masked one, 16 zero fills and 4 exec-mask branches per iteration)
    template <bool FULL>
    __device__ __forceinline__ void load(int k_left, float (&reg)[NR]) {
        const int tid = threadIdx.x;
        const char* b = reinterpret_cast<const char*>(base);
#pragma unroll
        for (int i = 0; i < NR / 4; ++i) {
            f32x4 v;
            if constexpr (FULL) {
                v = *reinterpret_cast<const f32x4*>(b + off[i]);
            } else {
                const int k = KC ? 4 * (tid % (BK / 4)) : (tid / TPR) + (NTHREADS / TPR) * i;
                v = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (k < k_left) v = *reinterpret_cast<const f32x4*>(b + off[i]);
            }
            reg[4 * i + 0] = v[0]; reg[4 * i + 1] = v[1]; reg[4 * i + 2] = v[2]; reg[4 * i + 3] = v[3];
        }
        base += step;
    }
};

template <bool KC, int VEC, int ROWS, int RP = 128>
__device__ __forceinline__ void load_operand(const float* __restrict__ base, long rs, long cs, int row0,
                                             int nrows_all, int k0, int K, float (&reg)[RP * BK / NTHREADS]) {
    constexpr int NR = RP * BK / NTHREADS, TPR = RP / 4;
    const int tid = threadIdx.x;
    const int nrows = min(nrows_all, row0 + ROWS);       // rows of THIS tile only
    if constexpr (VEC == 4) {
        if constexpr (KC) {
            constexpr int KQ = BK / 4, RPP = NTHREADS / KQ;       // float4 per row, rows per pass
            const int k = k0 + 4 * (tid % KQ);
#pragma unroll
            for (int i = 0; i < NR / 4; ++i) {
                const int row = row0 + (tid / KQ) + RPP * i;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (row < nrows && k < K) v = *reinterpret_cast<const f32x4*>(base + (long)row * rs + k);
                reg[4 * i + 0] = v[0]; reg[4 * i + 1] = v[1]; reg[4 * i + 2] = v[2]; reg[4 * i + 3] = v[3];
            }
        } else {
            const int row = row0 + 4 * (tid % TPR);
#pragma unroll
            for (int i = 0; i < NR / 4; ++i) {
                const int k = k0 + (tid / TPR) + (NTHREADS / TPR) * i;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (row < nrows && k < K) v = *reinterpret_cast<const f32x4*>(base + (long)k * cs + row);
                reg[4 * i + 0] = v[0]; reg[4 * i + 1] = v[1]; reg[4 * i + 2] = v[2]; reg[4 * i + 3] = v[3];
            }
        }
    } else {
        if constexpr (KC) {
            const int k = k0 + (tid % BK);
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int row = row0 + (tid / BK) + (NTHREADS / BK) * i;
                reg[i] = (row < nrows && k < K) ? base[(long)row * rs + k] : 0.f;
            }
        } else {
            const int row = row0 + (tid % RP);
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int k = k0 + (tid / RP) + (NTHREADS / RP) * i;
                reg[i] = (row < nrows && k < K) ? base[(long)k * cs + row] : 0.f;
            }
        }
    }
}

// ROWS = rows of the tile this operand stages (128, or 96 for the B side of the 128x96 tile): the RP-row thread
// mapping is shared, rows past ROWS are simply not stored (their image row stride LD may be too short for them).
template <bool KC, int VEC, int LD, int ROWS, int RP = 128>
__device__ __forceinline__ void store_operand(float (*T)[LD], const float (&reg)[RP * BK / NTHREADS]) {
    constexpr int NR = RP * BK / NTHREADS, TPR = RP / 4;
    const int tid = threadIdx.x;
    if constexpr (VEC == 4) {
        if constexpr (KC) {
            constexpr int KQ = BK / 4, RPP = NTHREADS / KQ;
            const int kq = 4 * (tid % KQ);
            // a wave stages 64 / KQ consecutive rows per pass: whether they lie past ROWS is wave-uniform (scalar branch)
            const int wave_row = __builtin_amdgcn_readfirstlane(tid >> 6) * (64 / KQ);
#pragma unroll
            for (int i = 0; i < NR / 4; ++i) {
                const int row = (tid / KQ) + RPP * i;
                if (ROWS < RP && ROWS % (64 / KQ) == 0 && wave_row + RPP * i >= ROWS) continue;
                if (ROWS < RP && ROWS % (64 / KQ) != 0 && row >= ROWS) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) T[kq + j][row] = reg[4 * i + j];
            }
        } else {
            const int row = 4 * (tid % TPR);
            if (ROWS < RP && row >= ROWS) return;
#pragma unroll
            for (int i = 0; i < NR / 4; ++i) {
                const int k = (tid / TPR) + (NTHREADS / TPR) * i;
                f32x4 v = {reg[4 * i + 0], reg[4 * i + 1], reg[4 * i + 2], reg[4 * i + 3]};
                *reinterpret_cast<f32x4*>(&T[k][row]) = v;
            }
        }
    } else {
        if constexpr (KC) {
            const int k = tid % BK;
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int row = (tid / BK) + (NTHREADS / BK) * i;
                if (ROWS < RP && row >= ROWS) continue;
                T[k][row] = reg[i];
            }
        } else {
            const int row = tid % RP;
            if (ROWS < RP && row >= ROWS) return;
#pragma unroll
            for (int i = 0; i < NR; ++i) T[(tid / RP) + (NTHREADS / RP) * i][row] = reg[i];
        }
    }
}

// XCD-aware, bijective tile remap (blocks b and b+8 share an XCD): the linear tile index, n fastest
__device__ __forceinline__ int remap_tile(const GemmP& p) {
    const int tiles = p.tiles_m * p.tiles_n;
    int lin = blockIdx.x;
    if (tiles >= 8) {
        const int q = tiles >> 3, rem = tiles & 7, x = lin & 7, idx = lin >> 3;
        lin = (x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q) + idx;
    }
    return lin;
}

// grid.y: batch entry (plain), k-slice of the concatenated reduction (split-K / reduce_batch), or — batched split-K,
// slices_per_batch > 0 — k-slice `z % spb` of batch entry `z / spb` (entry-local reduction range).  Sets the k-block
// range [kb_begin, kb_end) of this workgroup and z to the epilogue's batch index.
__device__ __forceinline__ void slice_range(const GemmP& p, int& z, int& kb_begin, int& kb_end) {
    z = blockIdx.y;
    kb_begin = z * p.kb_per_z;
    kb_end = min(kb_begin + p.kb_per_z, p.kb_total);
    if (p.slices_per_batch) {
        const int b = z / p.slices_per_batch, sl = z - b * p.slices_per_batch;
        kb_begin = b * p.kpb + sl * p.kb_per_z;
        kb_end = min(kb_begin + p.kb_per_z, (b + 1) * p.kpb);
        z = b;
    }
}

template <bool AKC, bool BKC, int VEC, int BN_>
__global__ __launch_bounds__(NTHREADS, BN_ == 96 ? CALM_GEMM_WAVES96 : CALM_GEMM_WAVES) void gemm_f32_kernel(const GemmP p) {
    constexpr int WN = BN_ == 128 ? 2 : 1;        // wave grid: 2x2 (128x128 tile) or 4x1 (128x96 tile)
    constexpr int MT = BN_ == 128 ? 2 : 1;        // 32x32 MFMA tiles per wave along M
    constexpr int NT = BN_ / (WN * 32);           // ... along N (2 or 3)
    constexpr int LDB = BN_ == 128 ? LDT : 100;   // B image row stride: 96 columns need no more (100 = 4 mod 32 banks too)
    __shared__ __attribute__((aligned(16))) float As[2][BK][LDT];
    __shared__ __attribute__((aligned(16))) float Bs[2][BK][LDB];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave id in an SGPR
    const int wm = WN == 2 ? wave >> 1 : wave, wn = WN == 2 ? wave & 1 : 0;
    const int r = lane & 31, h = lane >> 5;

    const int lin = remap_tile(p);
    const int tn = lin % p.tiles_n, tm = lin / p.tiles_n;
    const int m0 = tm * BM, n0 = tn * BN_;
    int z, kb_begin, kb_end;
    slice_range(p, z, kb_begin, kb_end);
    if (kb_begin >= kb_end && p.atomic) return;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    float ra[NREG], rb[NREG];

    OperandCursor<AKC, BM> ca;
    OperandCursor<BKC, BN_> cb;
    // the 8 k-pairs of one staged k-block: 1 (2) A and 3 (2) B fragments per 3 (4) MFMAs.  A wave whose rows all lie
    // past M (edge tile of a short M: the 40- and 176-row sequence-axis products) stages and synchronises but
    // issues no MFMAs: its accumulators are never stored.
    const bool wave_live = m0 + wm * (32 * MT) < p.M;
    auto multiply = [&](int buf) {
        if (!wave_live) return;
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            const int kk = 2 * s + h;
            float af[MT], bf[NT];
#pragma unroll
            for (int i = 0; i < MT; ++i) af[i] = As[buf][kk][wm * (32 * MT) + 32 * i + r];
#pragma unroll
            for (int j = 0; j < NT; ++j) bf[j] = Bs[buf][kk][wn * (32 * NT) + 32 * j + r];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    };
    auto stash = [&](int buf) {
        store_operand<AKC, VEC, LDT, BM>(As[buf], ra);
        store_operand<BKC, VEC, LDB, BN_>(Bs[buf], rb);
    };

    auto k_loop = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        int cur_b = -1;                       // batch entry the cursors point into
        auto fetch = [&](int kb) {
            const int b = p.kb_total == p.kpb ? 0 : kb / p.kpb;          // single-entry launches skip the divisions
            const int k0 = (kb - b * p.kpb) * BK;
            if constexpr (VEC == 4) {
                if (b != cur_b) {                                         // wave-uniform: first fetch, or a batch boundary
                    const int b0 = b / p.batch1, b1 = b - b0 * p.batch1;
                    ca.init(operand_base(p.A, p.Ag, p.n_group, p.a_b0, p.a_b1, b0, b1), p.a_rs, p.a_cs, m0, p.M, k0);
                    cb.init(operand_base(p.B, p.Bg, p.n_group, p.b_b0, p.b_b1, b0, b1), p.b_rs, p.b_cs, n0, p.N, k0);
                    cur_b = b;
                }
                ca.template load<FULL>(p.K - k0, ra);
                cb.template load<FULL>(p.K - k0, rb);
            } else {
                const int b0 = b / p.batch1, b1 = b - b0 * p.batch1;
                load_operand<AKC, VEC, BM>(operand_base(p.A, p.Ag, p.n_group, p.a_b0, p.a_b1, b0, b1), p.a_rs, p.a_cs,
                                           m0, p.M, k0, p.K, ra);
                load_operand<BKC, VEC, BN_>(operand_base(p.B, p.Bg, p.n_group, p.b_b0, p.b_b1, b0, b1), p.b_rs,
                                            p.b_cs, n0, p.N, k0, p.K, rb);
            }
        };
        if (kb_begin < kb_end) {
            fetch(kb_begin);
            stash(0);
        }
        __syncthreads();
        // two k-blocks per trip: the LDS stage of each half is a compile-time constant (no per-iteration address math)
        auto step = [&](int kb, auto stage_tag) {
            constexpr int ST = decltype(stage_tag)::value;
            const bool more = kb + 1 < kb_end;
            if (p.reduce_group && kb != kb_begin && kb % p.kpb == 0) group_rescale<MT, NT>(p, acc, kb / p.kpb);
            if (more) fetch(kb + 1);
            multiply(ST);
            if (more) stash(ST ^ 1);
            __syncthreads();
        };
        for (int kb = kb_begin; kb < kb_end; kb += 2) {
            step(kb, std::integral_constant<int, 0>{});
            if (kb + 1 < kb_end) step(kb + 1, std::integral_constant<int, 1>{});
        }
    };
    if constexpr (VEC == 4) {
        if (p.K % BK == 0) k_loop(std::true_type{});
        else k_loop(std::false_type{});
    } else {
        k_loop(std::false_type{});
    }
    // (a peeled loop without the per-iteration decisions for single-entry, whole-k-block launches measured +2% on
    // forward / input-gradient shapes, -2% on weight gradients and -0.6% on the training step: not kept)

    static_assert(sizeof(As) >= 4096 * (NTHREADS / 64), "the epilogue's per-wave scratch lives in the A stages");
    gemm_epilogue<MT, NT>(p, acc, m0, n0, wm, wn, r, h, z, (kb_end - 1) / p.kpb, (lds_float*)(&As[0][0][0]) + 1024 * wave);
}

template <bool AKC, bool BKC, int VEC>
int launch(const GemmP& p, dim3 grid, int bn, hipStream_t s) {
    if (bn == 128) hipLaunchKernelGGL((gemm_f32_kernel<AKC, BKC, VEC, 128>), grid, dim3(NTHREADS), 0, s, p);
    else hipLaunchKernelGGL((gemm_f32_kernel<AKC, BKC, VEC, 96>), grid, dim3(NTHREADS), 0, s, p);
    CALM_LAUNCH_CHECK();
    return 0;
}

int launch_f32(const GemmP& p, dim3 grid, int bn, bool akc, bool bkc, bool vec, hipStream_t s) {
    if (vec) {
        if (akc && bkc) return launch<true, true, 4>(p, grid, bn, s);
        if (akc && !bkc) return launch<true, false, 4>(p, grid, bn, s);
        if (!akc && bkc) return launch<false, true, 4>(p, grid, bn, s);
        return launch<false, false, 4>(p, grid, bn, s);
    }
    if (akc && bkc) return launch<true, true, 1>(p, grid, bn, s);
    if (akc && !bkc) return launch<true, false, 1>(p, grid, bn, s);
    if (!akc && bkc) return launch<false, true, 1>(p, grid, bn, s);
    return launch<false, false, 1>(p, grid, bn, s);
}

#if CALM_GEMM_F32_TILE64
// ---- 64-row tiles ------------------------------------------------------------------------------------------------------
// Epilogue of the 64-row tiles: acc[j] is the 16x16 block (rows 16 wave.., columns 16 j..) in the 16x16 MFMA C layout
// (col = lane & 15, row = 4 (lane >> 4) + e).  The same operations in the same order as gemm_epilogue (fp32 tensors
// only: the fp32 pipe takes no bf16 tensor).  Plain launches whose tensors allow it turn each block through 16 x 20
// floats of LDS scratch private to the wave (row stride 20: the 16-lane column groups of a half-wave write 16 banks
// apart) into the row layout — lane = row lane >> 2, columns 4 (lane & 3)..+3 — and move every epilogue tensor as
// 16-byte vectors; atomics, workspace partials and unaligned tensors take the one-element form.
constexpr int EPI16_LD = 20;
template <int NB>
__device__ __forceinline__ void gemm_epilogue16(const GemmP& p, f32x4 (&acc)[NB], int m0, int n0, int wave, int lane,
                                                int z, int sgroup, lds_float* __restrict__ scratch) {
#ifdef CALM_GEMM_NO_EPILOGUE            // timing experiment: everything but the epilogue (alpha is never this value)
    if (p.alpha != 12345.f) return;
#endif
    const int row0 = m0 + 16 * wave;
    if (row0 >= p.M) return;                                    // wave-uniform: a strip past M holds no results
    float scale = p.alpha;
    if (p.inv_scale) scale = scale / p.inv_scale[0];
    const int zc = (p.atomic && !p.slices_per_batch) ? 0 : z;
    const int cb0 = zc / p.batch1, cb1 = zc - cb0 * p.batch1;
    const long coff = cb0 * p.c_b0 + cb1 * p.c_b1;
    float* __restrict__ Cb = reinterpret_cast<float*>(p.C) + coff;
    if (p.n_group) {
        scale = scale / group_sigma(p, p.reduce_group ? sgroup : cb0);
        if (!p.reduce_group && p.Cg[0]) Cb = reinterpret_cast<float*>(p.Cg[cb0]) + cb1 * p.c_b1;
    }
    float* __restrict__ Pb = p.C_pre ? reinterpret_cast<float*>(p.C_pre) + coff : nullptr;
    const float* __restrict__ Xb = p.aux ? reinterpret_cast<const float*>(p.aux) + coff : nullptr;
    const float* __restrict__ Rb =
        p.residual ? reinterpret_cast<const float*>(p.residual) + (cb0 * p.r_b0 + cb1 * p.r_b1) : nullptr;
    // every GemmP field the block loops use, read once (see gemm_epilogue)
    const int pM = p.M, pN = p.N, p_act = p.act, p_accumulate = p.accumulate;
    const long c_rs = p.c_rs, r_rs = p.r_rs;
    const float* __restrict__ p_bias = p.bias;
    const float* __restrict__ p_col_scale = p.col_scale;
    if (p.epi_vec && !p.atomic) {
        const int rl = lane >> 2, c4 = 4 * (lane & 3);
        const int row = row0 + rl;
        const bool row_ok = row < pM;
        const int ro = row_ok ? row : row0;                     // row for loads (rows past M clamped)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int col0 = n0 + 16 * j;
            if (col0 >= pN) continue;                           // wave-uniform
#pragma unroll
            for (int e = 0; e < 4; ++e) scratch[(4 * (lane >> 4) + e) * EPI16_LD + (lane & 15)] = acc[j][e];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int col = col0 + c4;
            const bool col_ok = col < pN;                       // N % 4 == 0: a group is inside or outside
            const int colc = col_ok ? col : col0;
            const bool ok = row_ok && col_ok;
            const long ei = (long)ro * c_rs + colc;
            const f32x4 bj = p_bias ? *reinterpret_cast<const f32x4*>(p_bias + colc) : f32x4{0.f, 0.f, 0.f, 0.f};
            const f32x4 sj = p_col_scale ? *reinterpret_cast<const f32x4*>(p_col_scale + colc) : f32x4{1.f, 1.f, 1.f, 1.f};
            f32x4 v = *(const lds_f32x4*)(scratch + rl * EPI16_LD + c4);
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = v[c] * scale + bj[c];
            if (Pb && ok) *reinterpret_cast<f32x4*>(Pb + ei) = v;
            if (p_act == CALM_ACT_GELU) {
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = gelu_erf_f(v[c]);
            } else if (p_act == CALM_ACT_GELU_BWD) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(Xb + ei);
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] *= gelu_erf_grad_f(t[c]);
            }
            v *= sj;
            if (Rb) v += *reinterpret_cast<const f32x4*>(Rb + (long)ro * r_rs + colc);
            if (p_accumulate) v += *reinterpret_cast<const f32x4*>(Cb + ei);
            if (ok) *reinterpret_cast<f32x4*>(Cb + ei) = v;
            // the next block's scratch writes are issued after these reads: the LDS executes a wave's accesses in order
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        return;
    }
    const int rq = row0 + 4 * (lane >> 4);                      // rows rq .. rq + 3 of column col
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int col = n0 + 16 * j + (lane & 15);
        if (col >= pN) continue;
        if (p.atomic) {
            if (p.ws) {                      // dense [M][N] partial of this k-slice; splitk_reduce sums the slices
                float* __restrict__ Wb = p.ws + (long)blockIdx.y * p.ws_slice;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (rq + e < pM) Wb[(long)(rq + e) * pN + col] = acc[j][e] * scale;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (rq + e < pM) atomicAdd(Cb + (long)(rq + e) * c_rs + col, acc[j][e] * scale);
            }
            continue;
        }
        const float bj = p_bias ? p_bias[col] : 0.f;
        const float sj = p_col_scale ? p_col_scale[col] : 1.f;
        float v[4], t[4];
        long ci[4], ri[4];                                      // element offsets (rows past M clamped to row 0)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int rowc = rq + e < pM ? rq + e : 0;
            ci[e] = (long)rowc * c_rs + col;
            ri[e] = (long)rowc * r_rs + col;
            v[e] = acc[j][e] * scale + bj;
        }
        if (Pb) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (rq + e < pM) Pb[ci[e]] = v[e];
        }
        if (p_act == CALM_ACT_GELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = gelu_erf_f(v[e]);
        } else if (p_act == CALM_ACT_GELU_BWD) {
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] = Xb[ci[e]];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= gelu_erf_grad_f(t[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= sj;
        if (Rb) {
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] = Rb[ri[e]];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += t[e];
        }
        if (p_accumulate) {
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] = Cb[ci[e]];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += t[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (rq + e < pM) Cb[ci[e]] = v[e];
    }
}

// Tile 64 x (16 NB) x 16 per 256-thread workgroup: wave w owns rows 16 w .. 16 w + 15 across the whole tile width —
// NB independent v_mfma_f32_16x16x4_f32 accumulators (4 registers each: their 40-cycle dependent latency hides behind
// the other NB - 1), one A and NB B fragments per k-step.  Multiples of 16 (240, 528, 112, 80, 40 ...) tile N without
// padding, and M pads to 16 rows: a wave whose strip lies past M stages and synchronises but issues no MFMAs.
// k-steps in k order (lane group g = lane >> 4 feeds k = 4 s + g at step s): the two column groups of a ds_read_b32
// half-wave lie one image row apart, so the image row strides are = 16 mod 32 (A 80, B 48 / 80 / 112 / 144) and every
// half-wave touches 32 distinct banks.  Staging (64-row thread map for A and for B tiles of at most 64 columns, the 128-row map with the
// rows past the tile skipped for wider ones), k-loop and tile remap are the 128-row kernel's.
template <bool AKC, bool BKC, int VEC, int NB>
__global__ __launch_bounds__(NTHREADS, waves64(NB)) void gemm_f32_t64_kernel(const GemmP p) {
    constexpr int TM = 64, BN_ = 16 * NB;
    constexpr int RB = BN_ <= 64 ? 64 : 128;      // thread map of the B staging
    constexpr int LDA = 80, LDB = (BN_ + 15) / 32 * 32 + 16;      // image row strides (= 16 mod 32, >= the tile's rows)
    constexpr int NRA = TM * BK / NTHREADS, NRB = RB * BK / NTHREADS;
    __shared__ __attribute__((aligned(16))) float As[2][BK][LDA];
    __shared__ __attribute__((aligned(16))) float Bs[2][BK][LDB];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;

    const int lin = remap_tile(p);
    const int tn = lin % p.tiles_n, tm = lin / p.tiles_n;
    const int m0 = tm * TM, n0 = tn * BN_;
    int z, kb_begin, kb_end;
    slice_range(p, z, kb_begin, kb_end);
    if (kb_begin >= kb_end && p.atomic) return;

    f32x4 acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    float ra[NRA], rb[NRB];

    OperandCursor<AKC, TM, TM> ca;
    OperandCursor<BKC, BN_, RB> cb;
    const bool wave_live = m0 + 16 * wave < p.M;
    auto multiply = [&](int buf) {
        if (!wave_live) return;
#pragma unroll
        for (int s = 0; s < BK / 4; ++s) {
            const int kk = 4 * s + g;
            const float af = As[buf][kk][16 * wave + r];
            float bf[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) bf[j] = Bs[buf][kk][16 * j + r];
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf[j], acc[j], 0, 0, 0);
        }
    };
    auto stash = [&](int buf) {
        store_operand<AKC, VEC, LDA, TM, TM>(As[buf], ra);
        store_operand<BKC, VEC, LDB, BN_, RB>(Bs[buf], rb);
    };

    auto k_loop = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        int cur_b = -1;                       // batch entry the cursors point into
        auto fetch = [&](int kb) {
            const int b = p.kb_total == p.kpb ? 0 : kb / p.kpb;
            const int k0 = (kb - b * p.kpb) * BK;
            if constexpr (VEC == 4) {
                if (b != cur_b) {
                    const int b0 = b / p.batch1, b1 = b - b0 * p.batch1;
                    ca.init(operand_base(p.A, p.Ag, p.n_group, p.a_b0, p.a_b1, b0, b1), p.a_rs, p.a_cs, m0, p.M, k0);
                    cb.init(operand_base(p.B, p.Bg, p.n_group, p.b_b0, p.b_b1, b0, b1), p.b_rs, p.b_cs, n0, p.N, k0);
                    cur_b = b;
                }
                ca.template load<FULL>(p.K - k0, ra);
                cb.template load<FULL>(p.K - k0, rb);
            } else {
                const int b0 = b / p.batch1, b1 = b - b0 * p.batch1;
                load_operand<AKC, VEC, TM, TM>(operand_base(p.A, p.Ag, p.n_group, p.a_b0, p.a_b1, b0, b1), p.a_rs,
                                               p.a_cs, m0, p.M, k0, p.K, ra);
                load_operand<BKC, VEC, BN_, RB>(operand_base(p.B, p.Bg, p.n_group, p.b_b0, p.b_b1, b0, b1), p.b_rs,
                                                p.b_cs, n0, p.N, k0, p.K, rb);
            }
        };
        if (kb_begin < kb_end) {
            fetch(kb_begin);
            stash(0);
        }
        __syncthreads();
        auto step = [&](int kb, auto stage_tag) {
            constexpr int ST = decltype(stage_tag)::value;
            const bool more = kb + 1 < kb_end;
            if (p.reduce_group && kb != kb_begin && kb % p.kpb == 0) {
                const float ratio = group_sigma(p, kb / p.kpb) / group_sigma(p, kb / p.kpb - 1);
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[j] *= ratio;
            }
            if (more) fetch(kb + 1);
            multiply(ST);
            if (more) stash(ST ^ 1);
            __syncthreads();
        };
        for (int kb = kb_begin; kb < kb_end; kb += 2) {
            step(kb, std::integral_constant<int, 0>{});
            if (kb + 1 < kb_end) step(kb + 1, std::integral_constant<int, 1>{});
        }
    };
    if constexpr (VEC == 4) {
        if (p.K % BK == 0) k_loop(std::true_type{});
        else k_loop(std::false_type{});
    } else {
        k_loop(std::false_type{});
    }

    static_assert(sizeof(As) >= sizeof(float) * 16 * EPI16_LD * (NTHREADS / 64), "the epilogue's scratch lives in the A stages");
    gemm_epilogue16<NB>(p, acc, m0, n0, wave, lane, z, (kb_end - 1) / p.kpb,
                        (lds_float*)(&As[0][0][0]) + 16 * EPI16_LD * wave);
}

template <bool AKC, bool BKC, int VEC>
int launch_t64(const GemmP& p, dim3 grid, int nb, hipStream_t s) {
    switch (nb) {
    case 3: hipLaunchKernelGGL((gemm_f32_t64_kernel<AKC, BKC, VEC, 3>), grid, dim3(NTHREADS), 0, s, p); break;
    case 4: hipLaunchKernelGGL((gemm_f32_t64_kernel<AKC, BKC, VEC, 4>), grid, dim3(NTHREADS), 0, s, p); break;
    case 5: hipLaunchKernelGGL((gemm_f32_t64_kernel<AKC, BKC, VEC, 5>), grid, dim3(NTHREADS), 0, s, p); break;
    case 6: hipLaunchKernelGGL((gemm_f32_t64_kernel<AKC, BKC, VEC, 6>), grid, dim3(NTHREADS), 0, s, p); break;
    case 7: hipLaunchKernelGGL((gemm_f32_t64_kernel<AKC, BKC, VEC, 7>), grid, dim3(NTHREADS), 0, s, p); break;
    case 8: hipLaunchKernelGGL((gemm_f32_t64_kernel<AKC, BKC, VEC, 8>), grid, dim3(NTHREADS), 0, s, p); break;
    default: return CALM_E_INVAL;
    }
    CALM_LAUNCH_CHECK();
    return 0;
}

int launch_f32_t64(const GemmP& p, dim3 grid, int nb, bool akc, bool bkc, bool vec, hipStream_t s) {
    if (vec) {
        if (akc && bkc) return launch_t64<true, true, 4>(p, grid, nb, s);
        if (akc && !bkc) return launch_t64<true, false, 4>(p, grid, nb, s);
        if (!akc && bkc) return launch_t64<false, true, 4>(p, grid, nb, s);
        return launch_t64<false, false, 4>(p, grid, nb, s);
    }
    if (akc && bkc) return launch_t64<true, true, 1>(p, grid, nb, s);
    if (akc && !bkc) return launch_t64<true, false, 1>(p, grid, nb, s);
    if (!akc && bkc) return launch_t64<false, true, 1>(p, grid, nb, s);
    return launch_t64<false, false, 1>(p, grid, nb, s);
}
#else
int launch_f32_t64(const GemmP&, dim3, int, bool, bool, bool, hipStream_t) { return CALM_E_UNSUPP; }
#endif

}  // namespace calm_gemm_detail
