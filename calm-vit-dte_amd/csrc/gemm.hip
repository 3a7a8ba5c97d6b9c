// calm_gemm: strided / batched / grouped / split-K GEMM with fused epilogue for gfx950 — the dispatcher.
// Six kernel families, numbered as calm_gemm_plan::family in include/calm_vit.h:
//   0 exact fp32 MFMA, 128- or 64-row tiles (gemm_f32.hip)    3 bf16 pipelined persistent (gemm_bf16p.h)
//   1 bf16-operand, 128-row tiles (gemm_bf16.hip)             4 fp32 pipelined persistent (gemm_bf16p.h; opt-in)
//   2 bf16-operand, 256x128 tiles (gemm_bf16.hip)             5 fp8 operands (gemm_fp8.hip)
// Families 0-2 share tiling, remap, split logic and epilogue (gemm_common.h).  plan_gemm() decides a launch once and has
// no side effects; calm_gemm_workspace_bytes, calm_gemm_describe and calm_gemm report or launch that one decision.
#include <atomic>
#include "gemm_common.h"
#include "gemm_lane.h"
#include <stdlib.h>

using namespace calm_gemm_detail;

namespace {

// Second pass of a split launch with a workspace: C[m][n] (+= if accumulate) sum over the slices' partial tiles.
// grid.y = output (group); outputs are Cg[y] when given, else C + y * c_b0.
struct ReduceP {
    const float* ws; long ws_slice; int nslices;
    float* C; float* Cg[4]; long c_b0, c_rs;
    int M, N, accumulate;
};
__global__ __launch_bounds__(256) void splitk_reduce(const ReduceP q) {
    const long total = (long)q.M * q.N;
    const float* w = q.ws + (long)blockIdx.y * q.nslices * q.ws_slice;
    float* out = q.Cg[0] ? q.Cg[blockIdx.y] : q.C + blockIdx.y * q.c_b0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        float s0 = 0.f, s1 = 0.f;
        int sl = 0;
        for (; sl + 1 < q.nslices; sl += 2) {
            s0 += w[(long)sl * q.ws_slice + i];
            s1 += w[(long)(sl + 1) * q.ws_slice + i];
        }
        if (sl < q.nslices) s0 += w[(long)sl * q.ws_slice + i];
        const unsigned m = (unsigned)i / (unsigned)q.N, n = (unsigned)i - m * (unsigned)q.N;
        float* dst = out + (long)m * q.c_rs + n;
        *dst = (q.accumulate ? *dst : 0.f) + s0 + s1;
    }
}

// The same on 16-byte vectors with four slices in flight (N, the output's row stride and the slice size multiples of 4,
// 16-byte aligned bases): the scalar form above moved 3.2 TB/s of mostly cache-resident partial tiles (PMC, round 4:
// 96 calls, 0.78 ms per fp32 step).  Fixed order: slice sl goes to running sum sl % 4, combined (s0 + s1) + (s2 + s3).
__global__ __launch_bounds__(256) void splitk_reduce_vec(const ReduceP q) {
    const long total4 = ((long)q.M * q.N) >> 2;
    const f32x4* w = reinterpret_cast<const f32x4*>(q.ws + (long)blockIdx.y * q.nslices * q.ws_slice);
    const long slice4 = q.ws_slice >> 2;
    float* out = q.Cg[0] ? q.Cg[blockIdx.y] : q.C + blockIdx.y * q.c_b0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
        int sl = 0;
        for (; sl + 3 < q.nslices; sl += 4) {
            s0 += w[(long)sl * slice4 + i];
            s1 += w[(long)(sl + 1) * slice4 + i];
            s2 += w[(long)(sl + 2) * slice4 + i];
            s3 += w[(long)(sl + 3) * slice4 + i];
        }
        if (sl < q.nslices) s0 += w[(long)sl * slice4 + i];
        if (sl + 1 < q.nslices) s1 += w[(long)(sl + 1) * slice4 + i];
        if (sl + 2 < q.nslices) s2 += w[(long)(sl + 2) * slice4 + i];
        const unsigned e = (unsigned)(4 * i);
        const unsigned m = e / (unsigned)q.N, n = e - m * (unsigned)q.N;
        f32x4* dst = reinterpret_cast<f32x4*>(out + (long)m * q.c_rs + n);
        const f32x4 sum = (s0 + s1) + (s2 + s3);
        *dst = q.accumulate ? *dst + sum : sum;
    }
}

static void launch_splitk_reduce(const ReduceP& q, int n_out, hipStream_t s) {
    const long total = (long)q.M * q.N;
    bool vec = (q.N & 3) == 0 && (q.c_rs & 3) == 0 && (q.c_b0 & 3) == 0 && (q.ws_slice & 3) == 0 && aligned16(q.ws) &&
               total < (1l << 31);
    for (int g = 0; g < 4; ++g) vec = vec && (!q.Cg[g] || aligned16(q.Cg[g]));
    vec = vec && (q.Cg[0] || aligned16(q.C));
    if (vec) {
        const long t4 = total >> 2;
        const int gx = (int)((t4 + 255) / 256 < 2048 ? (t4 + 255) / 256 : 2048);
        hipLaunchKernelGGL(splitk_reduce_vec, dim3(gx, n_out), dim3(256), 0, s, q);
    } else {
        const int gx = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
        hipLaunchKernelGGL(splitk_reduce, dim3(gx, n_out), dim3(256), 0, s, q);
    }
}

#ifndef CALM_GEMM_WS_MIN_SLICES
#define CALM_GEMM_WS_MIN_SLICES 48     // per-slice partial tiles + one reduction instead of atomics from this many k-slices
#endif                                 // per output (A/B with plain stores in place of the atomics: outputs of 528 rows and
                                       // more, <= 42 slices, do not change; 384x768 ... 240x240, 53-106 slices, -15..-30%)

// calm_gemm_plan::family (include/calm_vit.h; backend.py and tests/locate.py compare against FAM_PIPE / FAM_PIPE32)
enum : int { FAM_F32 = 0, FAM_BF16 = 1, FAM_BF16_WIDE = 2, FAM_PIPE = 3, FAM_PIPE32 = 4, FAM_FP8 = 5 };

// What a launch decomposes into beyond its GemmP: decided once by plan_gemm, read by every entry point.
struct Decomp {
    int family = FAM_F32;
    int mt = 0, nt = 0;              // pipelined families: (64 mt) x (32 nt) tiles
    int bn = 0;                      // 128-row and 256x128 tiles: N tile (96 / 128); 64-row tiles: 16 nb
    int nb64 = 0;                    // fp32 64-row tiles: N tile / 16 (0: 128-row tiles)
    int npass = 1;                   // bf16-operand 128-row tiles: MFMA passes (3: CALM_BF16X3)
    bool vec = false;                // fp32 128-row tiles: 16-byte operand staging
    long items = 0;                  // tiles x (batch entries or k-slices)
    dim3 grid;                       // workgroups of the main launch
    int n_out = 1;                   // outputs the k-slices are combined into
    int slices_per_out = 1;          // k-slices per output (1: not split)
    int64_t ws_need = 0;             // workspace for one partial tile per slice (0: atomics, or not split)
};

// ---- pipelined persistent family (gemm_bf16p.h) -----------------------------------------------------------------------
// Takes the launches whose operands are both bf16 tensors: activation x weight (forward), gradient x weight^T (data
// gradient), gradient^T x activation (weight gradient, k-split over the chip), plain batches and independent groups.
// Declines (the 256-thread / 256x128 kernels keep them): batch-reduced and group-reduced sums, scalar epilogues, tiny
// problems.  CALM_GEMM_PIPE=0 in the environment switches the family off (A/B runs).
constexpr int PIPE_DECLINED = -1000;

std::atomic<int>& pipe_option(int which) {
    static std::atomic<int> opt[4] = {
        [] { const char* e = getenv("CALM_GEMM_PIPE"); return (e && e[0] == '0') ? 0 : 1; }(),
        [] { const char* e = getenv("CALM_GEMM_PIPE32"); return e ? atoi(e) : 0; }(),
        [] { const char* e = getenv("CALM_GEMM_DETERMINISTIC"); return (e && e[0] == '1') ? 1 : 0; }(),
        0};                                  // CALM_GEMM_OPT_LANE: the caller switches the side lane on (backend.set_wgrad_lane)
    return opt[which];
}
// every k-split / batch-reduced launch through the workspace + fixed-order reduction (no fp32 atomics)
bool deterministic() { return pipe_option(CALM_GEMM_OPT_DETERMINISTIC).load(std::memory_order_relaxed) != 0; }
bool lane_enabled() { return pipe_option(CALM_GEMM_OPT_LANE).load(std::memory_order_relaxed) != 0; }
bool pipe_enabled() { return pipe_option(CALM_GEMM_OPT_PIPE).load(std::memory_order_relaxed) != 0; }
// fp32 instantiation: 0 off (default), 1 every eligible launch, 2 k-contiguous operand pairs only
int pipe32_mode() { return pipe_enabled() ? pipe_option(CALM_GEMM_OPT_PIPE32).load(std::memory_order_relaxed) : 0; }

// How the k-slices of a split launch are combined: fp32 atomics onto a zeroed (or accumulated-into) C, or — in
// deterministic mode, or many slices per output and a caller-provided workspace — one dense partial tile per slice and a
// reduction pass.  `slices`: k-slices over all outputs (grid.y / work items per tile).
void plan_combine(const calm_gemm_args* a, GemmP& p, Decomp& d, int slices) {
    d.n_out = p.slices_per_batch ? a->batch0 * a->batch1 : 1;
    d.slices_per_out = p.atomic ? slices / d.n_out : 1;
    p.ws_slice = (long)a->M * a->N;
    if (p.atomic && (deterministic() || (d.slices_per_out >= CALM_GEMM_WS_MIN_SLICES && p.ws_slice >= 100000)))     // tiny outputs: the second launch costs more than their atomics
        d.ws_need = (int64_t)sizeof(float) * slices * p.ws_slice;
}

bool uses_workspace(const calm_gemm_args* a, const Decomp& d) {
    return d.ws_need > 0 && a->workspace && a->workspace_bytes >= d.ws_need && aligned16(a->workspace);
}

// modelled duration of a launch (cycles of one CU, up to a common factor): `rounds` items per persistent workgroup, each
// nk k-tiles of a (64 mt) x (32 nt) tile; a k-tile is bound by its MFMAs (64 mt nt cycles per SIMD at two waves) or by
// staging its (64 mt + 32 nt) x 128 bytes at ~40 B per cycle; the epilogue costs about one extra k-tile per tile row set
// (fp32: eight 32-cycle v_mfma_f32_16x16x4_f32 per tile, k-tile and wave instead of two 16-cycle bf16 ones)
double pipe_cost(long items, int mt, int nt, int nk, bool split, bool f32) {
    const long rounds = (items + 255) / 256;
    const double mfma = (f32 ? 512.0 : 64.0) * mt * nt, stage = (64.0 * mt + 32.0 * nt) * 128.0 / 40.0;
    const double ktile = (mfma > stage ? mfma : stage) + 120.0;
    const double epi = (split ? 90.0 : f32 ? 70.0 : 45.0) * mt * nt + 600.0;
    return rounds * (nk * ktile + epi);
}

// families 3 (bf16) and 4 (fp32): 0 or PIPE_DECLINED
int plan_pipe(const calm_gemm_args* a, GemmP& p, Decomp& d, bool f32) {
    const bool akc = a->a_cs == 1, bkc = a->b_cs == 1;
    if (!akc && bkc) return PIPE_DECLINED;                      // row-contiguous A with k-contiguous B: not instantiated
    if (a->reduce_batch || !p.epi_vec) return PIPE_DECLINED;
    if ((a->act == CALM_ACT_GELU_BWD) + (a->residual != nullptr) + (a->accumulate != 0) > 1) return PIPE_DECLINED;   // one C-shaped epilogue operand
    const int kt = f32 ? 32 : 64;                               // k per k-tile (128 bytes)
    if (a->M < 128 || a->N < 64 || a->K < kt) return PIPE_DECLINED;
    const int batch = a->batch0 * a->batch1;
    // per-lane staging offsets are 32-bit byte offsets from the batch entry's base
    const int64_t span_a = akc ? (int64_t)a->M * a->a_rs : 64 * a->a_cs + a->M;
    const int64_t span_b = bkc ? (int64_t)a->N * a->b_rs : 64 * a->b_cs + a->N;
    const int64_t span_max = f32 ? (1ll << 29) : (1ll << 30);
    if (span_a >= span_max || span_b >= span_max) return PIPE_DECLINED;
    if ((int64_t)a->M * a->c_rs >= (1ll << 29)) return PIPE_DECLINED;        // the epilogue's 32-bit byte offsets into C
    const bool trivial_epi = !a->bias && !a->col_scale && !a->residual && !a->C_pre && a->act == CALM_ACT_NONE;
    const int kpb = (a->K + kt - 1) / kt;

    // k-split: the same decisions as the 256-thread families (weight gradients: one problem, or independent groups,
    // whose tiles alone cannot fill the chip)
    const int tiles_min = ((a->M + 255) / 256) * ((a->N + 255) / 256);
    const bool group_split = a->n_group && a->split_k == 0 && trivial_epi && a->C_group[0] && tiles_min * batch < 128 && kpb >= 32;
    const bool k_split = group_split || a->split_k > 1 ||
                         (a->split_k == 0 && batch == 1 && trivial_epi && tiles_min < 128 && kpb >= 32);
    if (k_split && !group_split && batch != 1) return PIPE_DECLINED;
    // where the 256-thread kernels measured faster inside the training step (Base-224, same box): narrow k-split outputs,
    // small grouped weight gradients, reductions of two or three k-tiles
    if (!f32) {
        if (k_split && (a->M < 200 || a->N < 200)) return PIPE_DECLINED;
        if (group_split && (int64_t)a->M * a->N < 100000) return PIPE_DECLINED;
        if (!k_split && a->K < 160) return PIPE_DECLINED;
    }
    if (k_split && (!trivial_epi || a->c_type != CALM_ST_F32)) return PIPE_DECLINED;

    int best_mt = 0, best_nt = 0, best_split = 1;
    double best = 1e300;
    for (int mt = 2; mt <= 4; ++mt)
        for (int nt = 4; nt <= 8; ++nt) {
            if (f32 && mt == 4 && nt == 8) continue;            // 128 accumulators + fp32 fragments: spills
            const long tiles = (long)((a->M + 64 * mt - 1) / (64 * mt)) * ((a->N + 32 * nt - 1) / (32 * nt));
            if (!k_split) {
                const double c = pipe_cost(tiles * batch, mt, nt, kpb, false, f32);
                if (c < best) { best = c; best_mt = mt; best_nt = nt; best_split = 1; }
                continue;
            }
            const long per = tiles * (group_split ? batch : 1);
            for (int rounds = 1; rounds <= 4; ++rounds) {
                int ns = a->split_k > 1 ? a->split_k : (int)(256L * rounds / per);
                if (ns < 1) ns = 1;
                if (ns > kpb / 4) ns = kpb / 4 > 0 ? kpb / 4 : 1;
                const int nk = (kpb + ns - 1) / ns;
                ns = (kpb + nk - 1) / nk;
                // the slices' partial tiles are combined through atomics / the workspace: M x N x 4 bytes each through a
                // CHIP-WIDE resource at ~2 TB/s (scripts/ab_wgrad_split.py: 240 x 480 x 20480 takes 23.9 us with 16 slices,
                // 31.3 with 64, 38.3 with 128 — 0.13 us per 460 KB slice), in cycles of the launch like pipe_cost
                const double comb = ns > 1 ? (double)a->M * a->N * 4.0 * ns * (group_split ? batch : 1) / 2.0e12 * 2.0e9 : 0.0;
                const double c = pipe_cost(per * ns, mt, nt, nk, ns > 1, f32) + comb;
                if (c < best) { best = c; best_mt = mt; best_nt = nt; best_split = ns; }
            }
        }
    const int mt = best_mt, nt = best_nt, nsplit = best_split;
    p.tiles_m = (a->M + 64 * mt - 1) / (64 * mt);
    p.tiles_n = (a->N + 32 * nt - 1) / (32 * nt);
    p.kpb = kpb;
    p.kb_total = kpb;
    p.reduce_group = 0;
    p.atomic = nsplit > 1;
    p.slices_per_batch = 0;
    if (p.atomic) {
        p.kb_per_z = (kpb + nsplit - 1) / nsplit;
        const int ns = (kpb + p.kb_per_z - 1) / p.kb_per_z;
        if (group_split) {
            p.slices_per_batch = ns;
            p.nz = ns * batch;
        } else {
            p.nz = ns;
        }
    } else {
        p.kb_per_z = kpb;
        p.nz = batch;
    }
    d.family = f32 ? FAM_PIPE32 : FAM_PIPE;
    d.mt = mt;
    d.nt = nt;
    d.items = (long)p.tiles_m * p.tiles_n * p.nz;
    d.grid = dim3((int)(d.items < 256 ? d.items : 256));
    static const int stagger = [] { const char* e = getenv("CALM_PIPE_STAGGER"); return e ? atoi(e) : 0; }();
    p.stagger = d.items > 256 ? stagger : 0;
    {   // 8 columns per lane in the epilogue when every tensor it touches is bf16 and addressable in aligned groups of 8
        auto m8 = [](int64_t x) { return (x & 7) == 0; };
        const bool u8 = !p.atomic && a->c_type == CALM_ST_BF16 && (!a->aux || a->aux_type == CALM_ST_BF16) &&
                        (!a->residual || (a->r_type == CALM_ST_BF16 && m8(a->r_rs) && m8(a->r_b0) && m8(a->r_b1))) &&
                        m8(a->N) && m8(a->c_rs) && m8(a->c_b0) && m8(a->c_b1);
        p.epi_unit = u8 ? 8 : 4;
    }
    plan_combine(a, p, d, p.nz);
    return 0;
}

// modelled duration of a 256-thread fp32 launch (cycles of one CU, up to a common factor; the pattern of pipe_cost):
// `items` workgroups of nk k-blocks, each k-block `rows` live rows (strips past M skip their MFMAs) x `width` columns
// of MFMA work (x BK x 2 FLOP at 256 FLOP per CU cycle) plus a fixed share (staging, barrier, fragment reads), served
// ceil(items / 256) deep on the busiest CU at the matrix-pipe efficiency of its resident workgroups (min(slots, items
// per CU) of them: 0.89 at 4, 0.84 at 3 measured) — or, with too few of them to cover a k-block's memory latency, one
// exposed latency per k-block and resident round — plus one epilogue per resident round and the combine of the k-slices
// (atomics or the workspace: `combine` bytes through a chip-wide resource at ~2 TB/s, as in plan_pipe)
double f32_tile_cost(long items, int nk, double rows, int width, int slots, double combine) {
    constexpr double KB_FIXED = 192.0, KB_LATENCY = 1100.0, EPILOGUE = 1500.0;
    const long per_cu = (items + 255) / 256;
    const double resident = (double)(per_cu < slots ? per_cu : slots);
    const double kb = rows * width * BK * 2.0 / 256.0 + KB_FIXED;
    const double mfma = (double)per_cu * nk * kb * (resident + 0.5) / resident;
    const double rounds = (double)((items + 256L * slots - 1) / (256L * slots));
    const double lat = rounds * nk * KB_LATENCY;
    return (mfma > lat ? mfma : lat) + rounds * EPILOGUE + combine / 1000.0;
}

// ---- 256-thread families: 128-row tiles (0, 1) and 256x128 tiles (2) ----------------------------------------------------
// dtype: the matrix pipe the kernels run (CALM_F32 for a launch that cannot be vectorised)
int plan_tiles(const calm_gemm_args* a, GemmP& p, Decomp& d, int dtype, bool vec) {
    const int batch = a->batch0 * a->batch1;
    const int bk = dtype == CALM_F32 ? BK : CK;
    p.kpb = (a->K + bk - 1) / bk;
    const bool trivial_epi = !a->bias && !a->col_scale && !a->residual && !a->C_pre && a->act == CALM_ACT_NONE;

    // N tile: 128 (2x2 waves) or 96 (4x1 waves).  k-split launches (work spread evenly whatever the tile count) take
    // the width that pads N less (672, 528, 1344, 1056, 480 ... are multiples of 96 or nearly so), ties to 128 for
    // the better A-panel reuse.  Data-parallel launches take the width with the lower estimated time: the
    // workgroups resident on a CU share its matrix pipe, so a launch lasts about ceil(work items / CUs) x width
    // (A/B over the model's shapes: N=240 and N=352 are 12-20% faster on 96 although 128 pads less).
    p.tiles_m = (a->M + BM - 1) / BM;
    const int pad128 = (a->N + 127) / 128 * 128, pad96 = (a->N + 95) / 96 * 96;
    int bn = pad96 < pad128 ? 96 : 128;
    const bool grouped_reduce_unsplit = a->n_group && a->reduce_batch && a->split_k <= 1;
    // grouped weight gradients (dW_g = dY_g^T X of the projections that share X): every group gets its own k-slices
    const bool group_split = a->n_group && !a->reduce_batch && a->split_k == 0 && trivial_epi && a->C_group[0] &&
                             p.tiles_m * ((a->N + bn - 1) / bn) * batch < 256 && p.kpb >= 64;
    const bool k_split = group_split || (a->reduce_batch && !grouped_reduce_unsplit) || a->split_k > 1 ||
                         (a->split_k == 0 && batch == 1 && trivial_epi && p.tiles_m * ((a->N + bn - 1) / bn) < 256 &&
                          p.kpb >= 64);
    if (!k_split) {
        const long cus = 256;
        const long nb = grouped_reduce_unsplit ? 1 : batch;     // launches of the y grid dimension
        const long items96 = (long)p.tiles_m * (pad96 / 96) * nb, items128 = (long)p.tiles_m * (pad128 / 128) * nb;
        const long cost96 = (items96 + cus - 1) / cus * 96, cost128 = (items128 + cus - 1) / cus * 128;
        bn = cost96 < cost128 ? 96 : 128;
    }
    // bf16 operands, data-parallel launch with at least a full resident round (2 per CU) of 256x128 tiles: wide kernel
    bool wide = false;
    if (dtype == CALM_BF16 && !k_split) {
        const long nb = grouped_reduce_unsplit ? 1 : batch;
        const long rows_w = (long)(a->M + WBM - 1) / WBM * WBM;             // at most 1/8 of the rows padded
        wide = 8 * rows_w <= 9 * (long)a->M &&
               rows_w / WBM * ((a->N + WBN - 1) / WBN) * nb >= CALM_GEMM_WIDE_MIN_TILES;
    }
    // ... and the split-K weight gradients (plain or grouped) whose output pads by at most 1/4 in 256-row tiles (672,
    // 768, 1056, 1344 rows): with bf16 operands they are bound by re-reading the fp32 panels from L2, not by padded MFMAs
    wide = wide || (dtype == CALM_BF16 && k_split && !a->reduce_batch && (group_split || batch == 1) &&
                    4 * ((long)(a->M + WBM - 1) / WBM * WBM) <= 5 * (long)a->M);
    if (wide) {
        bn = WBN;
        p.tiles_m = (a->M + WBM - 1) / WBM;
    }
    p.tiles_n = (a->N + bn - 1) / bn;
    const int tiles = p.tiles_m * p.tiles_n;

    // k-slices of a split launch: one resident round of workgroups (256 CUs x 5 for the 96-wide tile, x 4 for the
    // 128-wide one; A/B over the weight-gradient shapes: -3% time against 768, -12% on 1344x672)
    const int split_slots = wide ? 256 * 2 : bn == 96 ? 256 * CALM_GEMM_WAVES96 : 256 * CALM_GEMM_WAVES;
    if (k_split && !group_split && !a->reduce_batch && batch != 1) return CALM_E_UNSUPP;
    // k-slices per output for `ntiles` output tiles and `slots` workgroup slots; min_kb: fewest k-blocks per slice
    auto split_count = [&](int ntiles, int slots, int min_kb) {
        int nsplit = 1;
        if (group_split) {
            nsplit = slots / (ntiles * batch);
            const int max_split = (p.kpb + min_kb - 1) / min_kb;
            if (nsplit > max_split) nsplit = max_split;
        } else if (a->reduce_batch && !grouped_reduce_unsplit) {
            nsplit = a->split_k > 1 ? a->split_k : slots / ntiles;
            const int max_split = (batch * p.kpb + 7) / 8;
            if (nsplit > max_split) nsplit = max_split;
            // every slice adds its whole tile onto the SAME output with atomics: beyond about one workgroup per CU the
            // contention costs more than the shorter slices save (scripts/ab_reduce_split.py, 256 images: 80x176x528 51.6 us
            // at 512 slices, 33.4 at 128; 224x176x528 69.7 -> 56.5; 128x80x240 24.4 -> 19.7)
            // (measured on the bf16-operand kernels; the fp32 kernels, 16x slower per k-block, keep their full round of slices)
            if (a->split_k <= 1 && dtype == CALM_BF16) {
                const int cap = ntiles == 1 ? 128 : 256 / ntiles;
                if (nsplit > cap) nsplit = cap;
            }
        } else if (k_split) {
            nsplit = a->split_k > 1 ? a->split_k : slots / ntiles;
            const int max_split = (p.kpb + min_kb - 1) / min_kb;
            if (nsplit > max_split) nsplit = max_split;
            // small outputs (the 128-row kernels' share of the weight gradients): every slice adds its tiles onto the same
            // output — about one workgroup per CU is the optimum (264 x 240 x 45056: 41.9 us at 88 slices, 29.7 at 32)
            // (bf16-operand kernels only: as above)
            if (a->split_k <= 1 && dtype == CALM_BF16 && !wide && nsplit > 256 / ntiles) nsplit = 256 / ntiles;
        }
        return nsplit < 1 ? 1 : nsplit;
    };
    // p.atomic, p.slices_per_batch, p.kb_total and p.kb_per_z of `nsplit` k-slices per output; returns grid.y
    auto apply_split = [&](int nsplit) {
        p.atomic = 0;
        p.slices_per_batch = 0;
        if (group_split) {
            p.kb_total = batch * p.kpb;
            if (nsplit > 1) {
                p.atomic = 1;
                p.slices_per_batch = nsplit;
            }
        } else if (grouped_reduce_unsplit) {
            p.kb_total = batch * p.kpb;                     // one k-range over all groups, plain epilogue
        } else if (a->reduce_batch) {
            p.atomic = 1;
            p.kb_total = batch * p.kpb;
        } else if (k_split) {
            p.kb_total = p.kpb;
            p.atomic = nsplit > 1;
        } else {
            p.kb_total = batch * p.kpb;
        }
        if (p.slices_per_batch) {
            p.kb_per_z = (p.kpb + nsplit - 1) / nsplit;
            p.slices_per_batch = (p.kpb + p.kb_per_z - 1) / p.kb_per_z;      // no empty trailing slices
        } else if (p.atomic) {
            p.kb_per_z = (p.kb_total + nsplit - 1) / nsplit;
        } else if (grouped_reduce_unsplit) {
            p.kb_per_z = p.kb_total;                        // grid.y == 1
        } else {
            p.kb_per_z = p.kpb;   // grid.y == batch
        }
        return p.slices_per_batch ? batch * p.slices_per_batch : (p.kb_total + p.kb_per_z - 1) / p.kb_per_z;
    };
    int nsplit = split_count(tiles, split_slots, 16);
    int gy = apply_split(nsplit);
    int nb64 = 0;
#if CALM_GEMM_F32_TILE64
    // fp32 pipe: the 128-row plan above against 64 x (16 nb) tiles, nb = 3..8, by modelled launch time (f32_tile_cost);
    // a k-split launch recomputes its slice count for the smaller tile (one or two resident rounds, >= 4 k-blocks each).
    // Launches whose 128-row plan combines its slices through the workspace (plan_combine) keep that plan.
    const int per_out = p.slices_per_batch ? p.slices_per_batch : gy;
    const bool ws_plan = p.atomic && per_out >= CALM_GEMM_WS_MIN_SLICES && (long)a->M * a->N >= 100000;
    if (dtype == CALM_F32 && (!ws_plan || CALM_GEMM_F32_TILE64 == 2)) {
        const bool auto_split = (group_split || (a->reduce_batch && !grouped_reduce_unsplit) || k_split) && a->split_k <= 1;
        auto cost_of = [&](int tiles_m, int tiles_n, int rows_live, int width, int slots, int y) {
            const long items = (long)tiles_m * tiles_n * y;
            const double comb = p.atomic ? 4.0 * a->M * a->N * y : 0.0;
            return f32_tile_cost(items, p.kb_per_z, (double)rows_live / tiles_m, width, slots, comb);
        };
        const int gran = bn == 128 ? 64 : 32;               // the 128-row tiles skip the MFMAs of whole wave strips
        double best = CALM_GEMM_F32_TILE64 == 2 ? 1e300 :
                      cost_of(p.tiles_m, p.tiles_n, (a->M + gran - 1) / gran * gran, bn,
                              bn == 96 ? CALM_GEMM_WAVES96 : CALM_GEMM_WAVES, gy);
        int best_split = nsplit;
        const int tm64 = (a->M + 63) / 64, rows64 = (a->M + 15) / 16 * 16;
        for (int nb = 3; nb <= 8; ++nb) {
            const int tn64 = (a->N + 16 * nb - 1) / (16 * nb);
            const int slots = waves64(nb);
            int cand[3] = {split_count(tm64 * tn64, 256 * slots, 16), 0, 0};
            if (auto_split) {
                cand[1] = split_count(tm64 * tn64, 256 * slots, 4);
                cand[2] = split_count(tm64 * tn64, 2 * 256 * slots, 4);
            }
            for (int ns : cand) {
                if (ns < 1) continue;
                const int y = apply_split(ns);
                const double c = cost_of(tm64, tn64, rows64, 16 * nb, slots, y);
                if (y <= 65535 && c < best) {
                    best = c;
                    nb64 = nb;
                    best_split = ns;
                }
            }
        }
        if (nb64) {
            bn = 16 * nb64;
            p.tiles_m = tm64;
            p.tiles_n = (a->N + bn - 1) / bn;
        }
        nsplit = best_split;
        gy = apply_split(nsplit);
    }
#endif
    if (p.atomic && a->c_type != CALM_ST_F32) return CALM_E_UNSUPP;            // k-slices combine in fp32
    if (p.atomic && !p.slices_per_batch && !trivial_epi) return CALM_E_UNSUPP;
    if (gy > 65535) return CALM_E_UNSUPP;
    d.family = wide ? FAM_BF16_WIDE : dtype == CALM_F32 ? FAM_F32 : FAM_BF16;
    d.bn = bn;
    d.nb64 = nb64;
    d.npass = dtype == CALM_BF16X3 ? 3 : 1;
    d.vec = vec;
    d.items = (long)p.tiles_m * p.tiles_n * gy;
    d.grid = dim3(p.tiles_m * p.tiles_n, gy);
    plan_combine(a, p, d, gy);
    return 0;
}

// ---- fp8 family (gemm_fp8.hip) ----------------------------------------------------------------------------------------
// both operands fp8 (B e4m3; A e4m3 or e5m2), k-contiguous, K and row strides multiples of 16 bytes, one launch per call
// (no k-split, no groups), dequantisation factors on the device
int plan_fp8(const calm_gemm_args* a, GemmP& p, Decomp& d) {
    if (a->b_type != CALM_ST_FP8_E4M3 || a->a_type < CALM_ST_FP8_E4M3 || !a->a_dq || !a->b_dq) return CALM_E_INVAL;
    if (a->dtype != CALM_BF16 || a->a_cs != 1 || a->b_cs != 1 || a->n_group || a->reduce_batch || a->split_k > 1) return CALM_E_UNSUPP;
    if ((a->K & 15) || (a->a_rs & 15) || (a->b_rs & 15) || (a->a_b0 & 15) || (a->a_b1 & 15) || (a->b_b0 & 15) ||
        (a->b_b1 & 15) || !aligned16(a->A) || !aligned16(a->B))
        return CALM_E_LAYOUT;
    const int batch = a->batch0 * a->batch1;
    if (batch > 65535) return CALM_E_UNSUPP;
    p.dq_a = a->a_dq;
    p.dq_b = a->b_dq;
    p.tiles_m = (a->M + WBM - 1) / WBM;
    p.tiles_n = (a->N + WBN - 1) / WBN;
    d.family = FAM_FP8;
    d.items = p.tiles_m * p.tiles_n * batch;
    d.grid = dim3(p.tiles_m * p.tiles_n, batch);
    return 0;
}

// Validates the arguments and decides the whole launch: GemmP (p value-initialised by the caller) and Decomp.  No side
// effects: calm_gemm_workspace_bytes, calm_gemm_describe and calm_gemm all report or launch this one decision.
int plan_gemm(const calm_gemm_args* a, GemmP& p, Decomp& d) {
    if (!a || !a->A || !a->B || !a->C) return CALM_E_INVAL;
    if (a->M <= 0 || a->N <= 0 || a->K <= 0 || a->batch0 <= 0 || a->batch1 <= 0) return CALM_E_INVAL;
    if (a->dtype != CALM_F32 && a->dtype != CALM_BF16 && a->dtype != CALM_BF16X3) return CALM_E_UNSUPP;
    for (int t : {a->c_type, a->aux_type, a->r_type})
        if (t != CALM_ST_F32 && t != CALM_ST_BF16) return CALM_E_INVAL;
    for (int t : {a->a_type, a->b_type})
        if (t < CALM_ST_F32 || t > CALM_ST_FP8_E5M2) return CALM_E_INVAL;
    const bool fp8 = a->a_type >= CALM_ST_FP8_E4M3 || a->b_type >= CALM_ST_FP8_E4M3;
    const bool any_bf16_tensor = a->a_type || a->b_type || a->c_type || a->aux_type || a->r_type;      // (or fp8)
    if (any_bf16_tensor && a->dtype != CALM_BF16) return CALM_E_UNSUPP;       // bf16 tensors: bf16 matrix pipe only
    if (a->a_rs != 1 && a->a_cs != 1) return CALM_E_LAYOUT;
    if (a->b_rs != 1 && a->b_cs != 1) return CALM_E_LAYOUT;
    // the staging cursors address a tile with 32-bit byte offsets from a per-tile base: 255 rows x stride x 4 B < 2^32
    if (a->a_rs >= (1 << 21) || a->a_cs >= (1 << 21) || a->b_rs >= (1 << 21) || a->b_cs >= (1 << 21)) return CALM_E_UNSUPP;
    if (a->act == CALM_ACT_GELU_BWD && !a->aux) return CALM_E_INVAL;
    if (a->act < 0 || a->act > CALM_ACT_GELU_BWD) return CALM_E_INVAL;
    if (a->n_group < 0 || a->n_group > CALM_GEMM_MAX_GROUP) return CALM_E_INVAL;
    if (a->n_group) {
        if (a->batch0 != a->n_group || a->batch1 != 1) return CALM_E_INVAL;
        if (a->C_pre || a->aux || a->residual || a->inv_scale) return CALM_E_UNSUPP;
        for (int g = 0; g < a->n_group; ++g) {
            if ((a->A_group[0] && !a->A_group[g]) || (a->B_group[0] && !a->B_group[g])) return CALM_E_INVAL;
            if (!a->reduce_batch && a->C_group[0] && !a->C_group[g]) return CALM_E_INVAL;
        }
    }

    p.A = a->A; p.B = a->B; p.C = a->C;
    p.a_type = a->a_type; p.b_type = a->b_type; p.c_type = a->c_type; p.aux_type = a->aux_type; p.r_type = a->r_type;
    p.M = a->M; p.N = a->N; p.K = a->K;
    p.batch1 = a->batch1;
    p.a_rs = a->a_rs; p.a_cs = a->a_cs; p.a_b0 = a->a_b0; p.a_b1 = a->a_b1;
    p.b_rs = a->b_rs; p.b_cs = a->b_cs; p.b_b0 = a->b_b0; p.b_b1 = a->b_b1;
    p.c_rs = a->c_rs; p.c_b0 = a->c_b0; p.c_b1 = a->c_b1;
    p.alpha = a->alpha; p.inv_scale = a->inv_scale; p.bias = a->bias; p.col_scale = a->col_scale;
    p.residual = a->residual; p.r_rs = a->r_rs; p.r_b0 = a->r_b0; p.r_b1 = a->r_b1;
    p.C_pre = a->C_pre; p.aux = a->aux;
    p.act = a->act; p.accumulate = a->accumulate;
    p.n_group = a->n_group;
    p.reduce_group = a->n_group && a->reduce_batch;
    for (int g = 0; g < a->n_group; ++g) {
        p.Ag[g] = a->A_group[g];
        p.Bg[g] = a->B_group[g];
        p.Cg[g] = a->C_group[g];
        p.Sg[g] = a->inv_scale_group[g];
    }
    {   // vector epilogue: every tensor the epilogue touches addressable in aligned groups of 4 columns
        auto m4 = [](int64_t x) { return (x & 3) == 0; };
        bool ev = m4(a->N) && m4(a->c_rs) && m4(a->c_b0) && m4(a->c_b1) && aligned16(a->C) &&
                  (!a->C_pre || aligned16(a->C_pre)) && (!a->aux || aligned16(a->aux)) &&
                  (!a->bias || aligned16(a->bias)) && (!a->col_scale || aligned16(a->col_scale)) &&
                  (!a->residual || (aligned16(a->residual) && m4(a->r_rs) && m4(a->r_b0) && m4(a->r_b1)));
        for (int g = 0; g < a->n_group; ++g) ev = ev && (!a->C_group[g] || aligned16(a->C_group[g]));
        p.epi_vec = ev && CALM_GEMM_VEC_EPILOGUE;
    }
    if (fp8) return plan_fp8(a, p, d);

    const bool akc = a->a_cs == 1, bkc = a->b_cs == 1;
    // 16-byte staging vectors hold 4 fp32 or 8 bf16 elements: sizes / strides of an operand must be multiples of that
    const int64_t ea = a->a_type == CALM_ST_BF16 ? 7 : 3, eb = a->b_type == CALM_ST_BF16 ? 7 : 3;
    auto mult = [](int64_t x, int64_t mask) { return (x & mask) == 0; };
    bool vec = aligned16(a->A) && aligned16(a->B) && mult(a->a_b0, ea) && mult(a->a_b1, ea) && mult(a->b_b0, eb) &&
               mult(a->b_b1, eb);
    for (int g = 0; g < a->n_group; ++g) vec = vec && aligned16(a->A_group[g]) && aligned16(a->B_group[g]);
    vec = vec && (akc ? (mult(a->K, ea) && mult(a->a_rs, ea)) : (mult(a->M, ea) && mult(a->a_cs, ea)));
    vec = vec && (bkc ? (mult(a->K, eb) && mult(a->b_rs, eb)) : (mult(a->N, eb) && mult(a->b_cs, eb)));
    // bf16-operand kernels need the 16-byte staging path; anything else runs on the exact fp32 kernels — which
    // only read fp32 tensors: a bf16 tensor in a launch that cannot be vectorised is the caller's layout error
    if (!vec && any_bf16_tensor) return CALM_E_LAYOUT;
    const int dtype = vec ? a->dtype : CALM_F32;
    if (dtype == CALM_BF16 && a->a_type == CALM_ST_BF16 && a->b_type == CALM_ST_BF16 && pipe_enabled()) {
        const int rc = plan_pipe(a, p, d, false);
        if (rc != PIPE_DECLINED) return rc;
    }
    if (vec && a->dtype == CALM_F32 && !any_bf16_tensor && (pipe32_mode() == 1 || (pipe32_mode() == 2 && akc && bkc))) {
        const int rc = plan_pipe(a, p, d, true);
        if (rc != PIPE_DECLINED) return rc;
    }
    return plan_tiles(a, p, d, dtype, vec);
}

// The only place a calm_gemm_plan is built.
calm_gemm_plan to_plan(const GemmP& p, const Decomp& d, bool use_ws) {
    calm_gemm_plan r{d.family, 0, 0, 0, p.tiles_m, p.tiles_n, d.slices_per_out, (int32_t)d.items,
                     (int32_t)(d.grid.x * d.grid.y), 0, use_ws ? 1 : 0, 0};
    switch (d.family) {
    case FAM_F32:       r.tile_m = d.nb64 ? 64 : BM; r.tile_n = d.bn; r.tile_k = BK; r.threads = NTHREADS; break;
    case FAM_BF16:      r.tile_m = BM;  r.tile_n = d.bn; r.tile_k = CK; r.threads = NTHREADS; break;
    case FAM_BF16_WIDE: r.tile_m = WBM; r.tile_n = WBN;  r.tile_k = CK; r.threads = WTHREADS; break;
    case FAM_FP8:       r.tile_m = WBM; r.tile_n = WBN;  r.tile_k = 64; r.threads = WTHREADS; break;
    default:            // FAM_PIPE, FAM_PIPE32
        r.tile_m = 64 * d.mt; r.tile_n = 32 * d.nt; r.tile_k = d.family == FAM_PIPE32 ? 32 : 64; r.threads = 512;
        r.epi_unit = p.epi_unit;
    }
    return r;
}

int launch_main(const GemmP& p, const Decomp& d, hipStream_t s) {
    const bool akc = p.a_cs == 1, bkc = p.b_cs == 1;
    switch (d.family) {
    case FAM_F32:
        return d.nb64 ? launch_f32_t64(p, d.grid, d.nb64, akc, bkc, d.vec, s) : launch_f32(p, d.grid, d.bn, akc, bkc, d.vec, s);
    case FAM_BF16:      return launch_bf16(p, d.grid, d.bn, akc, bkc, d.npass, s);
    case FAM_BF16_WIDE: return launch_bf16_wide(p, d.grid, akc, bkc, s);
    case FAM_FP8:       return launch_fp8(p, d.grid, s);
    case FAM_PIPE:
        return (akc && bkc ? launch_pipe_kk : akc ? launch_pipe_km : launch_pipe_mm)(p, d.mt, d.nt, d.grid.x, s);
    default:            // FAM_PIPE32
        return (akc && bkc ? launch_pipe32_kk : akc ? launch_pipe32_km : launch_pipe32_mm)(p, d.mt, d.nt, d.grid.x, s);
    }
}

// ---- the side lane (gemm_lane.h) -----------------------------------------------------------------------------------------
struct HipLaneRt {
    using Stream = hipStream_t;
    using Event = hipEvent_t;
    static int device(int* d) { return (int)hipGetDevice(d); }
    static int capturing(Stream s, bool* c) {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        const hipError_t e = hipStreamIsCapturing(s, &st);
        *c = st != hipStreamCaptureStatusNone;
        return (int)e;
    }
    static int stream_create(Stream* s) {       // non-blocking, the lowest priority the device offers
        int least = 0, greatest = 0;
        const hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (e != hipSuccess) return (int)e;
        return (int)hipStreamCreateWithPriority(s, hipStreamNonBlocking, least);
    }
    static int event_create(Event* e) { return (int)hipEventCreateWithFlags(e, hipEventDisableTiming); }
    static int record(Event e, Stream s) { return (int)hipEventRecord(e, s); }
    static int wait(Stream s, Event e) { return (int)hipStreamWaitEvent(s, e, 0); }
};

calm_lane::Book<HipLaneRt>& lane_book() {
    static calm_lane::Book<HipLaneRt> book;
    return book;
}

// One planned launch on stream `s`, or — `lane` — on the side lane of the current device (on `s` itself while the lane is
// off or `s` is capturing).  Plan, kernels, split and combine do not depend on the stream.
int gemm_launch(const calm_gemm_args* a, hipStream_t s, bool lane) {
    GemmP p{};
    Decomp d;
    int rc = plan_gemm(a, p, d);
    if (rc) return rc;
    if (lane) {
        rc = lane_book().launch_stream(lane_enabled(), s, &s);
        if (rc) return rc;
    }
    const bool use_ws = uses_workspace(a, d);
    if (use_ws) {
        p.ws = (float*)a->workspace;
    } else if (p.atomic && !a->accumulate) {
        for (int g = 0; g < d.n_out; ++g) {
            float* out = (float*)(p.slices_per_batch ? p.Cg[g] : p.C);
            hipError_t e;
            if (a->c_rs == a->N) e = hipMemsetAsync(out, 0, sizeof(float) * (size_t)a->M * a->N, s);
            else e = hipMemset2DAsync(out, sizeof(float) * a->c_rs, 0, sizeof(float) * a->N, a->M, s);
            if (e != hipSuccess) return (int)e;
        }
    }
#ifdef CALM_PIPE_STAMP
    if ((d.family == FAM_PIPE || d.family == FAM_PIPE32) && !p.atomic && a->workspace &&
        a->workspace_bytes >= 256 * 2 * 8 * 4 * 8)
        p.ws = (float*)a->workspace;                    // diagnostic build: stamps
#endif
    rc = launch_main(p, d, s);
    if (rc || !use_ws) return rc;
    ReduceP q;
    q.ws = p.ws; q.ws_slice = p.ws_slice; q.nslices = d.slices_per_out;
    q.C = (float*)p.C; q.c_b0 = a->c_b0; q.c_rs = a->c_rs;
    for (int g = 0; g < 4; ++g) q.Cg[g] = p.slices_per_batch ? (float*)p.Cg[g] : nullptr;
    q.M = a->M; q.N = a->N; q.accumulate = a->accumulate;
    launch_splitk_reduce(q, d.n_out, s);
    CALM_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int calm_gemm(const calm_gemm_args* a, void* stream) { return gemm_launch(a, as_stream(stream), false); }

extern "C" int calm_gemm_lane(const calm_gemm_args* a, void* main_stream) {
    return gemm_launch(a, as_stream(main_stream), true);
}

extern "C" int calm_gemm_lane_fork(void* main_stream) { return lane_book().fork(lane_enabled(), as_stream(main_stream)); }

extern "C" int calm_gemm_lane_join(void* main_stream) { return lane_book().join(as_stream(main_stream)); }

extern "C" int calm_gemm_lane_stats(int64_t out[4]) {
    if (!out) return CALM_E_INVAL;
    const calm_lane::Stats st = lane_book().stats();
    out[0] = st.forks; out[1] = st.launches; out[2] = st.joins; out[3] = st.events;
    return 0;
}

extern "C" int calm_gemm_set_option(int32_t option, int32_t value) {
    if (option != CALM_GEMM_OPT_PIPE && option != CALM_GEMM_OPT_PIPE32 && option != CALM_GEMM_OPT_DETERMINISTIC &&
        option != CALM_GEMM_OPT_LANE)
        return CALM_E_INVAL;
    if (value < 0 || value > (option == CALM_GEMM_OPT_PIPE32 ? 2 : 1)) return CALM_E_INVAL;
    return pipe_option(option).exchange(value);
}

extern "C" int calm_gemm_describe(const calm_gemm_args* a, calm_gemm_plan* plan) {
    if (!plan) return CALM_E_INVAL;
    GemmP p{};
    Decomp d;
    const int rc = plan_gemm(a, p, d);
    if (rc == 0) *plan = to_plan(p, d, uses_workspace(a, d));
    return rc;
}

extern "C" int64_t calm_gemm_workspace_bytes(const calm_gemm_args* a) {
    GemmP p{};
    Decomp d;
    return plan_gemm(a, p, d) == 0 ? d.ws_need : 0;
}
