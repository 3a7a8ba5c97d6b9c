/*
 * calm_vit.h — C-ABI of libcalmvit_hip.so, the MI355X (gfx950) kernel library behind the
 * CALM-ViT cross-axial latent-masking attention path.
 *
 * The reference (focegueda1998/CALM-ViT-DTE) is pure Python: its "FFI" for this path is the
 * set of ATen ops that CALM-ViT/Vi_Tools_CNN_less_V2.py and CALM-ViT/CALM_ViT_V2.py call.
 * Each entry point below replaces one such call site (cited as file:line into
 * /root/reference/CALM-ViT/) and is bound from Python with ctypes
 * (calm-vit-dte_amd/_lib.py; see INTEGRATION.md for the reference-side stub).
 *
 * Conventions
 *  - plain device pointers + sizes; element strides unless stated; no torch types.
 *  - every call only ENQUEUES work on `stream` (hipStream_t passed as void*): no allocation,
 *    no host synchronisation, re-entrant, hipGraph-capturable.
 *  - return value: 0 = ok, <0 = invalid argument / unsupported shape (CALM_E_*),
 *    >0 = hipError_t of the failed launch.  No C++ exceptions cross the boundary.
 *  - NaN/Inf propagate (GradScaler's inf check relies on it, distributed_trainer_cls.py:88,93).
 *  - tensors are fp32 unless an entry point takes a storage-type argument (CALM_ST_*; ABI v4: the bf16 pipeline).
 */
#ifndef CALM_VIT_H
#define CALM_VIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CALM_ABI_VERSION 7

#define CALM_E_INVAL   (-1)   /* null pointer / negative size                 */
#define CALM_E_LAYOUT  (-2)   /* stride pattern the kernel cannot address     */
#define CALM_E_UNSUPP  (-3)   /* combination of options not implemented       */

/* calm_gemm_args.dtype — tensors are fp32 in memory in every mode; the mode selects the matrix pipe:
 *   CALM_F32    exact fp32 MFMA (v_mfma_f32_32x32x2_f32), bit-for-bit an fmaf chain
 *   CALM_BF16   operands rounded to bf16 in LDS, fp32 accumulate (what autocast(bfloat16) computes)
 *   CALM_BF16X3 operands split hi+lo bf16, 3 MFMA passes, fp32 accumulate: ~2^-17 relative product error */
enum { CALM_F32 = 0, CALM_BF16 = 1, CALM_BF16X3 = 2 };
enum { CALM_ST_F32 = 0, CALM_ST_BF16 = 1, CALM_ST_FP8_E4M3 = 2, CALM_ST_FP8_E5M2 = 3 };   /* storage type of a tensor in HBM
                                                          (fp8: OCP e4m3fn / e5m2 as gfx950 implements them) */
enum { CALM_ACT_NONE = 0, CALM_ACT_GELU = 1, CALM_ACT_GELU_BWD = 2 };

int         calm_abi_version(void);
const char* calm_build_info(void);     /* "gfx950 ..." */

/* ---------------------------------------------------------------------------------------
 * Strided, batched GEMM with fused epilogue on the matrix cores (v_mfma_f32_32x32x2_f32).
 *
 *   acc(m,n)  = sum_k A(m,k) * B(n,k)                 A(m,k) = A[m*a_rs + k*a_cs + b0*a_b0 + b1*a_b1]
 *   z         = acc * alpha / (inv_scale ? *inv_scale : 1) + (bias ? bias[n] : 0)
 *   C_pre(m,n)= z                                      (optional second output, C's layout)
 *   y         = act == GELU      ? gelu_erf(z)
 *             : act == GELU_BWD  ? z * gelu_erf'(aux(m,n))   (aux: C's layout)
 *             : z
 *   C(m,n)    = y * (col_scale ? col_scale[n] : 1) + (residual ? residual(m,n) : 0) [+ C(m,n) if accumulate]
 *
 * One of (a_rs, a_cs) must be 1, likewise (b_rs, b_cs); C is n-contiguous.
 * Operand row / column strides must be below 2^21 elements (CALM_E_UNSUPP otherwise): a tile is addressed with
 * 32-bit byte offsets from a per-tile base.
 * batch = batch0*batch1 independent problems (b0,b1 strides per operand; 0 = broadcast).
 * reduce_batch: all batches are summed into ONE C (c_b0/c_b1 ignored) — the weight gradient of
 * the sequence-axis linears.  split_k: 0 = library picks, 1 = off, >1 = that many K-slices; slices
 * and reduce_batch combine through fp32 atomics and then allow alpha/inv_scale only.
 *
 * Grouped form (n_group = batch0 in 1..CALM_GEMM_MAX_GROUP; batch1 must be 1): the b0 entries are separate
 * allocations — entry g uses A_group[g], B_group[g], C_group[g] (a table whose first entry is NULL falls back to
 * base + g*stride) and its own spectral-norm scale inv_scale_group[g] (a NULL table entry = 1).
 *   without reduce_batch: n_group independent products in ONE launch (the q/k/v projections of a block read one
 *     activation: Vi_Tools_CNN_less_V2.py:265-267), each divided by its sigma in the epilogue;
 *   with reduce_batch:    C = sum_g A_g B_g^T / sigma_g in one pass over the concatenated reduction (their
 *     input gradient); runs unsplit — deterministic, full epilogue — unless split_k > 1.
 * Grouped launches take no C_pre / aux / residual.
 *
 * Replaces: nn.Linear / matmul / bmm call sites Vi_Tools_CNN_less_V2.py:226-231, 251-267, 276-277,
 * 288-290 (raw QK^T + linear_mask), 293-298 (QK^T, PV of SDPA), 300, 305-308, 312;
 * CALM_ViT_V2.py:76 (head), 1x1 convs Vi_Tools:380,384 — and all their autograd backward GEMMs.
 * ------------------------------------------------------------------------------------- */
typedef struct calm_gemm_args {
    const void* A; const void* B; void* C;
    int32_t M, N, K;
    int32_t batch0, batch1;
    int64_t a_rs, a_cs, a_b0, a_b1;
    int64_t b_rs, b_cs, b_b0, b_b1;
    int64_t c_rs, c_b0, c_b1;
    float        alpha;
    const float* inv_scale;      /* device scalar (spectral-norm sigma) or NULL */
    const float* bias;           /* [N] or NULL */
    const float* col_scale;      /* [N] or NULL (LayerScale ls_att / ls_mlp) */
    const void*  residual; int64_t r_rs, r_b0, r_b1;
    void*        C_pre;          /* optional pre-activation output */
    const void*  aux;            /* GELU_BWD: saved pre-activation */
    int32_t act;
    int32_t accumulate;
    int32_t reduce_batch;
    int32_t split_k;
    int32_t dtype;
    int32_t n_group;             /* 0 = plain strided batches */
    const void*  A_group[4];
    const void*  B_group[4];
    void*        C_group[4];
    const float* inv_scale_group[4];
    void*        workspace;      /* optional (ABI v3): device scratch for split launches, see calm_gemm_workspace_bytes */
    int64_t      workspace_bytes;
    /* ABI v4 — storage type of each tensor in HBM (CALM_ST_F32 / CALM_ST_BF16; strides stay in ELEMENTS of the tensor).
     * bf16 tensors are accepted by the bf16 matrix pipe only (dtype == CALM_BF16): the bf16 pipeline keeps the
     * activations that only GEMMs consume (LayerNorm outputs, MLP hidden states, attention outputs, their
     * gradients) and a per-step copy of the weights as bf16 — rounding an operand when it is stored instead of
     * every time a tile of it is staged: identical products, half the operand bytes.  A bf16 operand needs its
     * contiguous extent (K if k-contiguous, else its M / N), its other stride and its batch strides to be
     * multiples of 8 elements and a 16-byte aligned base (CALM_E_LAYOUT otherwise).  C_pre has C's type.
     * Split / batch-reduced outputs (fp32 atomics or workspace) must be fp32. */
    int32_t      a_type, b_type, c_type, aux_type, r_type;
    int32_t      reserved_;
    /* fp8 operands (BASELINE configs[4], "bf16 + fp8 MFMA GEMMs"): a_type in {FP8_E4M3, FP8_E5M2}, b_type FP8_E4M3, both
     * k-contiguous with K and row strides multiples of 16, dtype == CALM_BF16, no groups / k-split; a_dq / b_dq are the
     * DEVICE dequantisation factors written by calm_quantize_fp8 (amax / FP8_MAX): the epilogue multiplies the fp32
     * accumulator by a_dq * b_dq before alpha, sigma, bias ...  Products run on v_mfma_f32_32x32x16_{fp8,bf8}_fp8. */
    const float* a_dq; const float* b_dq;
} calm_gemm_args;
#define CALM_GEMM_MAX_GROUP 4

int calm_gemm(const calm_gemm_args* args, void* stream);
/* Bytes of `workspace` with which this launch would combine its k-slices through per-slice partial tiles and one
 * reduction pass instead of fp32 atomics (0: the launch is not split, or atomics are as fast — large outputs).
 * Passing less (or NULL) is always valid: the launch then uses atomics.  The caller owns the buffer; it is only used
 * until the launch's kernels have run on `stream`. */
int64_t calm_gemm_workspace_bytes(const calm_gemm_args* args);

/* ABI v6 — kernel-family switches of calm_gemm (process-wide tuning knobs, not part of the reference's interface: every
 * setting computes the same products to rounding).  Returns the previous value, CALM_E_INVAL for an unknown option.
 *   CALM_GEMM_OPT_PIPE    1 (default; env CALM_GEMM_PIPE):  bf16-tensor launches on the pipelined persistent family
 *   CALM_GEMM_OPT_PIPE32  0 (default; env CALM_GEMM_PIPE32): fp32-tensor launches on the same pipeline
 *                         (gemm_f32p_kernel) — 1: every eligible launch, 2: k-contiguous operand pairs only.  Off by
 *                         default: the fp32 matrix pipe is clock-limited under sustained load and both families end
 *                         at the same rate. */
/*   CALM_GEMM_OPT_DETERMINISTIC (ABI v7) 0 (default; env CALM_GEMM_DETERMINISTIC): 1 = EVERY k-split / batch-reduced
 *                         launch asks for a workspace (calm_gemm_workspace_bytes) and combines its slices through
 *                         per-slice partial tiles and one fixed-order reduction pass — no fp32 atomics, the weight
 *                         gradients repeat bit for bit (a launch that is handed no workspace still uses atomics).
 *                         Off by default: below ~48 slices per output the atomics are faster (the partial tiles
 *                         are written and read back once more).  The forward and input-gradient products never split:
 *                         they are reproducible in either mode. */
#define CALM_GEMM_OPT_PIPE   0
#define CALM_GEMM_OPT_PIPE32 1
/*   CALM_GEMM_OPT_LANE (an addition to ABI v7) 0 (default): 1 = calm_gemm_lane launches go to the side lane, see below. */
#define CALM_GEMM_OPT_DETERMINISTIC 2
#define CALM_GEMM_OPT_LANE 3
int calm_gemm_set_option(int32_t option, int32_t value);

/* The side lane (an addition to ABI v7): one non-blocking stream of the lowest priority per device, owned by the
 * library, for launches whose result nothing reads soon — the weight-gradient GEMMs of a backward, which are MFMA-bound
 * and can fill the CUs while the caller's stream runs kernels that leave the matrix pipe idle.
 *   calm_gemm_lane_fork(main)   an event recorded on `main`, the lane waits for it.  Call it immediately before each
 *                               lane launch: the lane then sees the launch's operands (and a zeroed C) finished.
 *   calm_gemm_lane(args, main)  calm_gemm(args, .) on the lane: same plan, same kernels, same split and combine.  The
 *                               caller keeps A, B, C and the workspace alive, and unused by other streams, until the
 *                               join — the lane is not the stream their allocator knows.
 *   calm_gemm_lane_join(main)   an event recorded on the lane, `main` waits for it: every lane launch so far is ordered
 *                               before what `main` is given next.  Does nothing if no launch went to the lane since the
 *                               last join.
 * With CALM_GEMM_OPT_LANE = 0, and while `main` is capturing a graph, fork and join do nothing and calm_gemm_lane
 * launches on `main`: it is then exactly calm_gemm, and a captured graph has the shape it has without the lane.
 * calm_gemm_lane_stats: counts since the library was loaded — out[0] forks that recorded an event, out[1] launches that
 * went to a lane, out[2] joins that recorded an event, out[3] events recorded. */
int calm_gemm_lane(const calm_gemm_args* args, void* main_stream);
int calm_gemm_lane_fork(void* main_stream);
int calm_gemm_lane_join(void* main_stream);
int calm_gemm_lane_stats(int64_t out[4]);

/* ABI v7 — what calm_gemm would launch for `args` (nothing is enqueued): kernel family, tile, work decomposition.
 * Diagnostic surface: tests use it to map a wrong output element back to (tile, persistent workgroup, XCD, wave,
 * 16-row strip) — see tests/locate.py — and the bench to label its per-shape table.
 *   family  0 fp32 tiles, 128-row or 64-row               3 bf16 pipelined persistent (gemm_bf16p_kernel)
 *             (gemm_f32_kernel / gemm_f32_t64_kernel)
 *           1 bf16-operand 128-row tiles                   4 fp32 pipelined persistent (gemm_f32p_kernel)
 *           2 bf16-operand 256x128 tiles                   5 fp8
 *   items = tiles_m * tiles_n * (batch entries or k-slices); the persistent families launch min(items, 256) workgroups
 *   that walk items in the XCD-aware order of gemm_bf16p.h::decode, the others one workgroup per (tile, y). */
typedef struct calm_gemm_plan {
    int32_t family;
    int32_t tile_m, tile_n, tile_k;
    int32_t tiles_m, tiles_n;
    int32_t k_slices;          /* k-slices per output (1: not split) */
    int32_t items;
    int32_t grid;              /* workgroups of the main launch */
    int32_t epi_unit;          /* pipelined families: columns per lane of the row-layout epilogue (4 / 8); else 0 */
    int32_t uses_workspace;    /* slices combined through args->workspace (1) or fp32 atomics (0) */
    int32_t threads;           /* threads per workgroup */
} calm_gemm_plan;
int calm_gemm_describe(const calm_gemm_args* args, calm_gemm_plan* plan);

/* ---------------------------------------------------------------------------------------
 * ABI v7 — fixed-order cross-workgroup reductions.  Every entry point whose result sums over workgroups (LayerNorm dw,
 * RoPE d_inv_freq, bias column sums, the latent KL sum, the CNN tail's weight gradients) takes `partials`: device
 * scratch of at least calm_reduce_scratch_floats(op, rows, cols) floats (16-byte aligned).  Workgroup g writes one
 * row of partial sums; a second launch of the same call adds the rows in workgroup order.  No atomics remain outside
 * calm_gemm's optional k-split (CALM_GEMM_OPT_DETERMINISTIC) and the standalone calm_dwconv3x3_bwd helper: forward and
 * backward of the path repeat bit for bit.  The scratch is only used until the call's kernels have run on `stream`.
 *   op                        rows                 cols
 *   CALM_RED_LAYERNORM_BWD    rows                 D
 *   CALM_RED_ROPE_BWD         B*S*H                dr
 *   CALM_RED_LATENT_FWD       rows                 mvh
 *   CALM_RED_COLSUM           rows                 cols
 *   CALM_RED_CNN_BWD          B                    S
 *   CALM_RED_SOFT_CE          B                    C            (the loss entry points, additions to ABI v7)
 *   CALM_RED_HUBER            B*S                  3S
 *   CALM_RED_EVAL             B                    C            (calm_eval_metrics: one 16-byte record per row)
 *   CALM_RED_RECON            B                    S            (calm_recon_metrics: one 32-byte record per workgroup)
 *   CALM_RED_DISTILL          B                    C            (calm_distill_fwd: five sums per row)
 *   CALM_RED_BCE              B                    C            (calm_bce_fwd: 2 * B floats, row sums and agreement flags)
 *   CALM_RED_MIM              B                    S            (calm_mim_huber_fwd: one block sum per workgroup)
 * ------------------------------------------------------------------------------------- */
enum { CALM_RED_LAYERNORM_BWD = 0, CALM_RED_ROPE_BWD = 1, CALM_RED_LATENT_FWD = 2, CALM_RED_COLSUM = 3, CALM_RED_CNN_BWD = 4,
       CALM_RED_SOFT_CE = 5, CALM_RED_HUBER = 6, CALM_RED_EVAL = 7, CALM_RED_RECON = 8, CALM_RED_DISTILL = 9,
       CALM_RED_BCE = 10, CALM_RED_MIM = 11 };
int64_t calm_reduce_scratch_floats(int32_t op, int64_t rows, int32_t cols);

/* ---------------------------------------------------------------------------------------
 * Deferred reductions (additions to ABI v7 — no existing signature or struct changes, so the version number stays).
 * The second launch of the entry points above is pure latency (a few microseconds for at most a megabyte or two), and
 * its outputs are leaf gradients that nothing reads before the backward ends.  A caller may therefore run the FIRST
 * launch alone — calm_part_layernorm_bwd, calm_part_rope_bwd, calm_part_colsum, calm_part_cnn_residual_bwd: the
 * siblings of calm_layernorm_bwd / calm_rope_bwd / calm_colsum / calm_cnn_residual_bwd without the output of the sum
 * — keep each call's `partials` alive (one buffer per call, sized by calm_reduce_scratch_floats as before), and combine
 * many of them later with calm_reduce_partials_batch.  Each sibling reports the rows of partials it wrote through
 * calm_reduce_shape; the batch runs, per entry, exactly the additions of the single form in the same order (one shared
 * device function), so the results are bit-identical.
 *
 * calm_reduce_entry: G rows of n partials, `stride` floats apart; columns [begin[k], begin[k+1]) are ADDED to out[k]
 * (nseg <= 6 outputs side by side, begin[0] = 0, begin[nseg] = n).  The entries travel by value in the kernel arguments
 * (no device table, no host-to-device copy: safe under stream capture), calm_reduce_batch_max() per launch; a longer
 * list is split into several launches.  `entries` is host memory and is not read after the call returns.
 * ------------------------------------------------------------------------------------- */
typedef struct calm_reduce_shape {
    int32_t G, n, stride, nseg;
    int32_t begin[7];
    int32_t reserved;
} calm_reduce_shape;
typedef struct calm_reduce_entry {
    const float* partials;
    int32_t G, n, stride, nseg;
    float* out[6];
    int32_t begin[7];
    int32_t reserved;
} calm_reduce_entry;
int32_t calm_reduce_batch_max(void);
int calm_reduce_partials_batch(const calm_reduce_entry* entries, int32_t n_entries, void* stream);
int calm_part_layernorm_bwd(const void* dy, const float* x, const float* w, const float* mean, const float* rstd,
                            float* dx, const float* dx_add, int64_t rows, int32_t D, int32_t dy_type, float* partials,
                            calm_reduce_shape* shape, void* stream);
int calm_part_rope_bwd(const void* d_out, const void* xr, const float* table, void* d_content, void* d_xr, int32_t B,
                       int32_t S, int32_t H, int32_t dc, int32_t dr, int32_t dout_type, int32_t xr_type,
                       int32_t dcontent_type, int32_t dxr_type, float* partials, calm_reduce_shape* shape, void* stream);
int calm_part_colsum(const void* x, int64_t rows, int32_t cols, int32_t x_type /* CALM_ST_* */, float* partials,
                     calm_reduce_shape* shape, void* stream);
/* (shape->begin: the six segments g0 | gb0 | g2 | gb2 | g4 | gb4 of a partial row) */
int calm_part_cnn_residual_bwd(const float* dy, const float* x, const float* w0, const float* s0, const float* b0,
                               const float* w2, const float* s2, const float* b2, const float* w4, const float* s4,
                               const float* b4, float* dx, int32_t B, int32_t S, int32_t hidden, int32_t residual,
                               float* partials, calm_reduce_shape* shape, void* stream);

/* ---------------------------------------------------------------------------------------
 * LayerNorm(D, eps, bias=False) over the last axis (Vi_Tools:131-132,197,494; fwd 211-215,311,523).
 * x,y: [rows, D] contiguous.  mean,rstd: [rows] saved for backward.
 * bwd: dx = rstd*(w*dy - mean_D(w*dy) - xhat*mean_D(w*dy*xhat)) [+ dx_add]; dw[D] += sum_rows dy*xhat
 * (added onto the caller's dw in a fixed order through `partials`, see calm_reduce_scratch_floats).  dx_add (nullable, x's layout): gradient arriving
 * through the skip connection that bypasses the norm (x feeds LN and the block's residual add, Vi_Tools:209-211,
 * 309-315), summed into dx here instead of by a separate elementwise pass.
 * y_type / dy_type (CALM_ST_*, ABI v4): the normalised output and the gradient arriving for it may be bf16 tensors
 * (bf16 pipeline: the output only feeds GEMMs; statistics, x and dx stay fp32).
 * ------------------------------------------------------------------------------------- */
int calm_layernorm_fwd(const float* x, const float* w, void* y, float* mean, float* rstd,
                       int64_t rows, int32_t D, float eps, int32_t y_type, void* stream);
int calm_layernorm_bwd(const void* dy, const float* x, const float* w, const float* mean,
                       const float* rstd, float* dx, float* dw, const float* dx_add, int64_t rows, int32_t D,
                       int32_t dy_type, float* partials /* ABI v7 */, void* stream);

/* ---------------------------------------------------------------------------------------
 * Learned-frequency NeoX RoPE + head assembly (Vi_Tools:80-95 applied at 275-285).
 * out[b,s,h, 0:dc]      = content[b,s,h,:]               (dc may be 0: plain blocks)
 * out[b,s,h, dc:dc+dr]  = rope(xr[b,s,h,:], t=s, inv_freq[dr/2])
 * content: [B,S,H,dc], xr: [B,S,H,dr], out: [B,S,H,dc+dr], all contiguous.
 * table: [2, S, dr/2] workspace; fwd fills it with cos|sin(t * inv_freq) (rebuilt every forward
 * because inv_freq is a learned parameter, Vi_Tools:70-71,86-91) and bwd reads it back.
 * bwd: d_content, d_xr from d_out; d_inv_freq[dr/2] += ... (fixed order through `partials`; dr/2 <= 256 and tensors
 * below 2^31 elements, CALM_E_UNSUPP otherwise).
 * Each tensor may be fp32 or bf16 (type arguments): in the bf16 pipeline the projections write bf16 and the
 * attention reads bf16 q / k; the rotation itself, the table and d_inv_freq are fp32.
 * ------------------------------------------------------------------------------------- */
int calm_rope_fwd(const void* content, const void* xr, const float* inv_freq, float* table, void* out,
                  int32_t B, int32_t S, int32_t H, int32_t dc, int32_t dr,
                  int32_t content_type, int32_t xr_type, int32_t out_type /* CALM_ST_*, ABI v4 */, void* stream);
int calm_rope_bwd(const void* d_out, const void* xr, const float* table,
                  void* d_content, void* d_xr, float* d_inv_freq,
                  int32_t B, int32_t S, int32_t H, int32_t dc, int32_t dr,
                  int32_t dout_type, int32_t xr_type, int32_t dcontent_type, int32_t dxr_type,
                  float* partials /* ABI v7 */, void* stream);

/* ---------------------------------------------------------------------------------------
 * Row softmax of the masked logits and its backward (the softmax inside
 * F.scaled_dot_product_attention, Vi_Tools:293-298).  In place.  rows x cols contiguous.
 * bwd: dp <- p * (dp - sum_j p*dp).
 * calm_sum_heads: dm[b,i,j] = sum_h dl[b,h,i,j]  (gradient of the head-broadcast mask, :291).
 * ------------------------------------------------------------------------------------- */
int calm_softmax_fwd(float* x, int64_t rows, int32_t cols, void* stream);
int calm_softmax_bwd(const float* p, float* dp, int64_t rows, int32_t cols, void* stream);
/* the two steps above in one pass for P, dP: [B,H,Sq,cols]: dP <- softmax backward, dm[b,i,j] = sum_h dP[b,h,i,j] */
int calm_softmax_bwd_heads(const float* p, float* dp, float* dm, int32_t B, int32_t H, int32_t Sq, int32_t cols,
                           void* stream);
int calm_sum_heads(const float* dl, float* dm, int32_t B, int32_t H, int64_t per_head, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused cross-axial latent-mask attention, forward (Vi_Tools:288-299):
 *   R = Q_all K_all^T;  M = W2 gelu(W1 R^T + b1) + b2 (along the key axis, weights divided by their
 *   sigmas);  out_h = softmax(Q_h K_h^T / sqrt(hd) + M) V_h  — the mask is produced and applied in-kernel.
 * q:[B,Sq,H*hd]  k,v:[B,Skv,H*hd]  w1:[2Skv,Skv] b1:[2Skv]  w2:[Skv,2Skv] b2:[Skv]  out:[B,Sq,H*hd].
 * Saved for backward: R:[B,Sq,Skv], hp/hg:[B,Sq,2Skv] (mask-MLP hidden before/after GELU), the mask
 * Mk:[B,Sq,Skv] and, if P != NULL, the probabilities P:[B,H,Sq,Skv].
 * calm_attention_fwd_supported() tells whether the shape has a fused instantiation
 * (Sq,Skv multiples of 16 with Skv/16 in {2,3,5,8,11,14}, hd%4==0, hd<=128); otherwise the caller
 * composes the same result from calm_gemm + calm_softmax_fwd.
 * ------------------------------------------------------------------------------------- */
int calm_attention_fwd_supported(int32_t Sq, int32_t Skv, int32_t H, int32_t hd);
int calm_attention_fwd(const float* q, const float* k, const float* v, const float* w1, const float* b1,
                       const float* s1, const float* w2, const float* b2, const float* s2, float* out, float* R,
                       float* hp, float* hg, float* Mk, float* P, int32_t B, int32_t Sq, int32_t Skv, int32_t H, int32_t hd,
                       void* stream);

/* Backward of the attention core for the same shapes (two launches: query side, key/value side):
 *   dP = dO_h V_h^T; dS = P o (dP - rowsum(P o dP)); dM = sum_h dS; dQ_h = dS K_h / sqrt(hd);
 *   dV_h = P^T dO_h; dK_h = dS^T Q_h / sqrt(hd).
 * dS:[B,H,Sq,Skv] is scratch written and re-read by the call; dq,dk,dv,dM are written (not accumulated).
 * The mask-MLP backward (through dM) and the dR = dM-path terms are calm_gemm calls of the caller. */
int calm_attention_bwd_preferred(int32_t Sq, int32_t Skv, int32_t H, int32_t hd);   /* supported AND measured faster */
int calm_attention_bwd(const float* q, const float* k, const float* v, const float* dout, const float* P, float* dS,
                       float* dq, float* dk, float* dv, float* dM, int32_t B, int32_t Sq, int32_t Skv, int32_t H,
                       int32_t hd, void* stream);

/* The same backward split around the caller's mask-MLP backward, so that the two dR products (the gradient of
 * R = Q_all K_all^T, Vi_Tools:288-289: dQ_all += dR K_all, dK_all += dR^T Q_all) ride on the per-head contractions
 * instead of being calm_gemm calls (additions to ABI v7 — no existing signature or struct changes, so the version
 * number stays).  Same shapes, same argument checks and return codes as calm_attention_bwd.
 *   calm_attention_bwd_front: the query side without dQ.  Writes dS and dM, bit-identical to calm_attention_bwd's;
 *     reads neither q nor k.  The caller then runs the mask-MLP backward from dM, which yields dR [B,Sq,Skv].
 *   calm_attention_bwd_back: dV_h = P^T dO_h; dK_h = (dS_h / sqrt(hd) + dR)^T Q_h; dQ_h = (dS_h / sqrt(hd) + dR) K_h.
 *     dq, dk, dv are written (not accumulated) and are complete: nothing is left for the caller to add.  No atomics:
 *     results repeat bit for bit.  dS is the tensor calm_attention_bwd_front wrote.
 *   calm_attention_bwd_fold_preferred: supported AND front + back measured faster than the caller's present route
 *     (calm_attention_bwd or the calm_gemm composition) followed by the two dR products. */
int calm_attention_bwd_front(const float* v, const float* dout, const float* P, float* dS, float* dM, int32_t B,
                             int32_t Sq, int32_t Skv, int32_t H, int32_t hd, void* stream);
int calm_attention_bwd_back(const float* q, const float* k, const float* dout, const float* P, const float* dS,
                            const float* dR, float* dq, float* dk, float* dv, int32_t B, int32_t Sq, int32_t Skv,
                            int32_t H, int32_t hd, void* stream);
int calm_attention_bwd_fold_preferred(int32_t Sq, int32_t Skv, int32_t H, int32_t hd);

/* Process-wide switches of the attention launchers, in the style of calm_gemm_set_option (addition to ABI v7 — no
 * existing signature or struct changes, so the version number stays).  Returns the previous value, CALM_E_INVAL for an
 * unknown option or value.
 *   CALM_ATTN_OPT_BACK  how the two kernels of calm_attention_bwd_back bring a head's dO_h / Q_h / K_h stripe into LDS:
 *       CALM_ATTN_BACK_TABLE  (default) per compiled geometry, whichever form is measured faster on MI355X
 *       CALM_ATTN_BACK_STRIPE the whole [S][hd] stripe at once: stage, barrier, contract, barrier
 *       CALM_ATTN_BACK_RING   32-column slabs through a two-slot ring, the next slab requested under the contraction
 *     Both forms run the same MFMA chains in the same order: dq, dk and dv are bit-identical (tests, same-process A/B). */
#define CALM_ATTN_OPT_BACK    0
#define CALM_ATTN_BACK_TABLE  0
#define CALM_ATTN_BACK_STRIPE 1
#define CALM_ATTN_BACK_RING   2
int calm_attention_set_option(int32_t option, int32_t value);

/* Row-LSE mode of the fp32 attention (Vi_Tools:288-299; additions to ABI v7 — no existing signature or struct
 * changes, so the version number stays): train without the saved probabilities.
 *   calm_attention_fwd_lse: calm_attention_fwd with P left out and lse [B,H,Sq] written instead,
 *     lse[b,h,i] = log sum_j exp(q_i.k_j / sqrt(hd) + M[i,j]) (natural log).  out, R, hp, hg, Mk are bit-identical
 *     to calm_attention_fwd's.
 *   calm_attention_bwd_lse: calm_attention_bwd without P.  The query-side launch first rebuilds each head's
 *     probabilities, P = exp(Q_h K_h^T / sqrt(hd) + Mk - lse), into the caller's scratch and continues as the
 *     stored-P kernel; dq, dk, dv, dM are written (not accumulated).  No atomics: results repeat bit for bit.
 *   calm_attention_bwd_lse_scratch_bytes: host only, no launch.  Bytes of device scratch (16-byte aligned, contents
 *     undefined before and after) that calm_attention_bwd_lse needs for the shape; 0 = no fused instantiation
 *     (exactly the shapes calm_attention_fwd_supported refuses, or B outside 1..65535).  A smaller scratch_bytes is
 *     CALM_E_INVAL.  Served for every supported shape, whatever calm_attention_bwd_preferred answers. */
int calm_attention_fwd_lse(const float* q, const float* k, const float* v, const float* w1, const float* b1,
                           const float* s1, const float* w2, const float* b2, const float* s2, float* out, float* R,
                           float* hp, float* hg, float* Mk, float* lse, int32_t B, int32_t Sq, int32_t Skv, int32_t H,
                           int32_t hd, void* stream);
int64_t calm_attention_bwd_lse_scratch_bytes(int32_t B, int32_t Sq, int32_t Skv, int32_t H, int32_t hd);
int calm_attention_bwd_lse(const float* q, const float* k, const float* v, const float* dout, const float* Mk,
                           const float* lse, void* scratch, int64_t scratch_bytes, float* dq, float* dk, float* dv,
                           float* dM, int32_t B, int32_t Sq, int32_t Skv, int32_t H, int32_t hd, void* stream);

/* Lean inference forward of the fp32 attention (addition to ABI v7, as the row-LSE entries were): calm_attention_fwd
 * with R, hp, hg, P and lse absent — the forward of a model that will run no backward.  Mk [B,Sq,Skv] stays: it is the
 * caller's scratch, written once and re-read by the kernel per head.  Same kernel, same supported shapes
 * (calm_attention_fwd_supported), same launch geometry; the stores of the absent tensors are compiled out.  out and Mk
 * are bit-identical to calm_attention_fwd's. */
int calm_attention_infer(const float* q, const float* k, const float* v, const float* w1, const float* b1,
                         const float* s1, const float* w2, const float* b2, const float* s2, float* out, float* Mk,
                         int32_t B, int32_t Sq, int32_t Skv, int32_t H, int32_t hd, void* stream);

/* ---------------------------------------------------------------------------------------
 * The same attention on the bf16 matrix pipe (ABI v4; the bf16 pipeline — what autocast(bfloat16) makes of
 * Vi_Tools:288-299): q, k, v, out and the saved R / hp / hg / Mk are bf16 tensors; w1 [2S,S] / w2 [S,2S] are the
 * step's bf16 weight copies; biases, sigmas and the row log-sum-exp lse [B,H,S] are fp32.  Accumulation and softmax
 * are fp32 (v_mfma_f32_16x16x32_bf16).  Every shape with S % 8 == 0, S <= 384, hd % 4 == 0, hd <= 128 is
 * supported (keys padded to 32 in-kernel with mask -inf, head dims to 32 with zero columns).  The probabilities are
 * NOT stored: the backward recomputes them from q, k, the mask and lse.  The mask is saved twice, Mk [B,query,key]
 * and MkT [B,key,query] (the query-side / key-side backward passes keep queries / keys on the MFMA lanes).
 *   calm_attention16_bwd: dq, dk, dv (bf16, written), dM [B,S,S] (bf16, written; the caller's mask-MLP backward
 *   continues from it); delta [B,H,S] fp32 scratch (rowsum(dO o O) = rowsum(P o dP), written by the query-side
 *   pass, read by the key-side pass); out = the forward's output.
 * Two kernel generations sit behind these entry points, chosen by shape (same arithmetic, same rounding points):
 * S <= 224 with hd <= 64 (every stage of Base-224) runs the LDS-DMA pipelined kernels of round 3
 * (csrc/attention_bf16_fwd2.h, csrc/attention_bf16_bwd2.h; the forward only when H * hd % 8 == 0, i.e. rows of q / k
 * are whole 16-byte chunks), everything else the register-staged ones.  No entry point
 * uses atomics: results repeat bit for bit.  With B % 8 == 0 the workgroups of one image are dealt to one XCD (L2 reuse
 * of its K / V); any B is valid.
 * ------------------------------------------------------------------------------------- */
int calm_attention16_supported(int32_t S, int32_t H, int32_t hd);
int calm_attention16_fwd(const void* q, const void* k, const void* v, const void* w1, const float* b1, const float* s1,
                         const void* w2, const float* b2, const float* s2, void* out, void* R, void* hp, void* hg,
                         void* Mk, void* MkT, float* lse, int32_t B, int32_t S, int32_t H, int32_t hd, void* stream);
int calm_attention16_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout, const void* Mk,
                         const void* MkT, const float* lse, float* delta, void* dq, void* dk, void* dv, void* dM,
                         int32_t B, int32_t S, int32_t H, int32_t hd, void* stream);
/* Lean inference forward of the bf16 attention (addition to ABI v7): calm_attention16_fwd without R, hp, hg, MkT and lse
 * and without the transpose pass that writes MkT.  Mk [B,S,S] (bf16) stays as the caller's scratch.  Both kernel
 * generations, chosen by the same rule as in calm_attention16_fwd; never the experimental CALM_ATTN16_V3 pair.  out and
 * Mk are bit-identical to calm_attention16_fwd's. */
int calm_attention16_infer(const void* q, const void* k, const void* v, const void* w1, const float* b1, const float* s1,
                           const void* w2, const float* b2, const float* s2, void* out, void* Mk, int32_t B, int32_t S,
                           int32_t H, int32_t hd, void* stream);

/* ---------------------------------------------------------------------------------------
 * Latent bottleneck sampling (Vi_Tools:232-242) + KL partial sum (Vi_Tools:24-25).
 * mv: [rows, 2*mvh] (mean | raw).  std = softplus(raw)+1e-6;  z = mean + noise*std (noise NULL
 * in eval: z = mean).  kl_sum (device scalar) += sum(1 + 2 log std - mean^2 - std^2) — block partials through
 * `partials`, added in block order (ABI v7: reproducible; rounds 1-3 used fp32 atomics).
 * bwd: dmv from dz and the scalar d(kl_sum) (device pointer).
 * ------------------------------------------------------------------------------------- */
int calm_latent_fwd(const float* mv, const float* noise, float* z, float* std_out, float* kl_sum,
                    int64_t rows, int32_t mvh, float* partials /* ABI v7 */, void* stream);
int calm_latent_bwd(const float* dz, const float* d_kl_sum, const float* mv, const float* noise,
                    const float* std_in, float* dmv, int64_t rows, int32_t mvh, void* stream);

/* ---------------------------------------------------------------------------------------
 * Spectral norm (hook-based torch.nn.utils.spectral_norm wrapped around every Linear/Conv:
 * Vi_Tools:137-205,380-384; CALM_ViT_V2.py:50-52,62-66), batched over a table of layers.
 * training!=0: v <- normalize(W^T u); u <- normalize(W v); sigma = u.(W v)   (in place on u,v)
 * training==0: sigma = u.(W v) with the stored u,v.
 * Every reduction has a fixed order (no atomics): u, v, sigma are bit-reproducible, hence identical on every
 * data-parallel rank that holds the same weights (what DDP's per-forward buffer broadcast guarantees in the reference).
 * Three launches cover ALL layers of the model (the reference issues 882 mv + 883 div per forward).
 *
 * Usage: fill a host array of calm_sn_layer (device pointers inside), call calm_sn_plan() to get
 * the size of / fill a host "plan" blob, copy the blob to device memory once (pointers must stay
 * valid), then call calm_sn_power_iter(plan_dev, ...) every step with `scratch` of
 * plan_info.scratch_floats floats.
 * ------------------------------------------------------------------------------------- */
typedef struct calm_sn_layer {
    const float* w;      /* [rows, cols] row-major (conv weights flattened over dim 0) */
    float* u;            /* [rows] */
    float* v;            /* [cols] */
    float* sigma;        /* [1] */
    int32_t rows, cols;
} calm_sn_layer;

typedef struct calm_sn_plan_info {
    int64_t blob_bytes;      /* size of the plan blob */
    int64_t scratch_floats;  /* size of the per-call scratch */
    int32_t n_layers, n_work;
    int32_t n_work_a, reserved;   /* ABI v4: work items of the column-owning W^T u pass */
} calm_sn_plan_info;

/* blob_host == NULL: only fills *info.  Otherwise writes blob_bytes bytes to blob_host. */
int calm_sn_plan(const calm_sn_layer* layers, int32_t n, void* blob_host, calm_sn_plan_info* info);
int calm_sn_power_iter(const void* plan_dev, const calm_sn_plan_info* info, int32_t training,
                       float eps, float* scratch, void* stream);

/* ---------------------------------------------------------------------------------------
 * bf16 copies of many fp32 tensors in ONE launch (ABI v4): the bf16 pipeline refreshes the bf16 copy of every weight
 * once per forward (W_orig itself, not W_orig/sigma: the GEMM epilogues keep dividing by sigma in fp32), next to the
 * power iteration.  entries_dev: table in device memory; work items are chunks of calm_cast_chunk_elems() consecutive
 * elements of one entry: chunk_entry_dev[k] = entry of chunk k, entry.chunk0 = its first chunk.  Round to nearest even
 * (what autocast's weight cast does inside `with autocast(device_type="cuda", dtype=torch.bfloat16)`,
 * distributed_trainer_cls.py:84-85: torch `.to(bfloat16)` of every Linear weight per forward).
 * ------------------------------------------------------------------------------------- */
typedef struct calm_cast_entry {
    const float* src;
    void*        dst;          /* bf16[numel] */
    int64_t      numel;
    int32_t      chunk0, reserved;
} calm_cast_entry;
int32_t calm_cast_chunk_elems(void);
int calm_cast_bf16(const calm_cast_entry* entries_dev, const int32_t* chunk_entry_dev, int32_t n_chunks, void* stream);
/* Per-tensor fp8 quantisation (ABI v4): q[i] = fp8(x[i] * FP8_MAX / amax(|x|)) with FP8_MAX = 448 (e4m3) / 57344 (e5m2),
 * state[0] <- amax, state[1] <- amax / FP8_MAX (the dequantisation factor calm_gemm takes as a_dq / b_dq); x fp32 or
 * bf16, n % 4 == 0.  Two launches (amax, then convert: just-in-time scaling, no history).
 * calm_transpose_u8: out[c][r] = in[r][c] on bytes — the transposed fp8 weight copy of the input-gradient product. */
int calm_quantize_fp8(const void* x, int32_t x_type, int64_t n, void* q, int32_t q_type, float* state, void* stream);
int calm_transpose_u8(const void* in, void* out, int32_t rows, int32_t cols, void* stream);
/* one tensor: dst[i] = bf16(src[i]) — the fp32 residual-stream gradient that two backward GEMMs are about to read */
int calm_cast_bf16_one(const float* src, void* dst, int64_t n, void* stream);
/* ABI v7 — dst[i] = (float)src[i] for a bf16 tensor: the fp32 copies of the rare bf16 launch whose strides rule out
 * 16-byte staging (10-class head, 36-token stage of the fixture models) — rounds 1-3 used torch casts there */
int calm_cast_f32_one(const void* src, float* dst, int64_t n, void* stream);

/* Weight gradient through W = W_orig / sigma (and an optional LayerScale on the output):
 *   d_ls[c]  = sum_k G[c,k] * W_orig[c,k] / sigma            (only if ls != NULL; written)
 *   G0       = (ls ? ls[c] : 1) * G
 *   dW_orig  = (G0 - <G0, W_orig/sigma> u v^T) / sigma       (written)
 * G: [rows, cols] = dY^T X.  scratch: >= rows+2 floats. */
int calm_sn_weight_bwd(const float* G, const float* w_orig, const float* u, const float* v,
                       const float* sigma, const float* ls, float* d_w_orig, float* d_ls,
                       int32_t rows, int32_t cols, float* scratch, void* stream);
/* The same correction for many layers in two launches per calm_sn_bwd_batch_max() layers (an addition to ABI v7): the
 * row-dot pass over work items (layer, row) and the apply pass over (layer, row chunk), entries by value in the kernel
 * arguments as for calm_reduce_partials_batch.  Per layer the arithmetic and the summation order are those of
 * calm_sn_weight_bwd (shared device functions): bit-identical results, with and without ls.  rowdot: >= rows floats of
 * scratch per entry, alive until the launches have run on `stream`.  `entries` is host memory. */
typedef struct calm_sn_bwd_entry {
    const float *G, *w_orig, *u, *v, *sigma, *ls;   /* ls nullable */
    float *d_w_orig, *d_ls, *rowdot;                /* d_ls nullable */
    int32_t rows, cols;
} calm_sn_bwd_entry;
int32_t calm_sn_bwd_batch_max(void);
int calm_sn_weight_bwd_batch(const calm_sn_bwd_entry* entries, int32_t n_entries, void* stream);

/* ---------------------------------------------------------------------------------------
 * Optimizer-side step over ALL parameters in three launches (distributed_trainer_cls.py:88-96,158):
 * GradScaler.unscale_ + inf/NaN check, clip_grad_norm_(max_norm), AdamW — torch.optim.AdamW's update exactly:
 *   p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * with g = grad * min(1, max_norm/(||grad||+1e-6)) / grad_scale; the whole update is skipped when a gradient is
 * inf/NaN (what scaler.step() does).  A tensor with sn_sigma != NULL carries the gradient w.r.t. its NORMALISED
 * weight (backward deferred the correction): dW_orig = (G - <G, W_orig/sigma> u v^T)/sigma is applied on the fly
 * and is what enters the norm.
 *
 * tensors_dev: table in device memory.  Work items are chunks of calm_optim_chunk_elems() consecutive elements of one
 * tensor: chunk_tensor_dev[k] = tensor index of chunk k, tensor.chunk0 = its first chunk.
 * scratch: 6*n_tensors + 4 + 3*n_chunks floats.  stats_out[2] (device): total gradient norm, found_inf.
 * Every reduction of the call has a fixed order (per-chunk partials, summed per tensor in chunk order): given equal
 * gradients — what the all-reduce leaves on every rank — all ranks apply bit-identical updates.
 * step_dev (nullable, device int32, ABI v4): the bias-correction step count kept on the device; it advances by one
 * per call EXCEPT when the update is skipped for inf/NaN gradients (torch's fused AdamW under a GradScaler), and then
 * replaces hparams->step.
 * ------------------------------------------------------------------------------------- */
typedef struct calm_optim_tensor {
    float*       param;
    const float* grad;
    float*       exp_avg;
    float*       exp_avg_sq;
    const float* sn_u;        /* [rows]  NULL for plain tensors */
    const float* sn_v;        /* [cols] */
    const float* sn_sigma;    /* [1] */
    int64_t numel;
    int32_t rows, cols;       /* rows*cols == numel for deferred spectral-norm weights */
    int32_t chunk0;
    int32_t group;            /* parameter group, read by calm_optim_step_groups only (0 from a zeroed table) */
} calm_optim_tensor;

typedef struct calm_optim_hparams {
    float lr, beta1, beta2, eps, weight_decay, max_norm;   /* max_norm <= 0: no clipping */
    int32_t step;                                           /* 1-based */
} calm_optim_hparams;

int32_t calm_optim_chunk_elems(void);
int calm_optim_step(const calm_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev,
                    int32_t n_chunks, float* scratch, const calm_optim_hparams* hparams,
                    const float* grad_scale /* device scalar or NULL */, float* stats_out, int32_t* step_dev,
                    const float* lr_dev /* ABI v7: device scalar overriding hparams->lr, or NULL — lets a captured
                                           (hipGraph) step follow an LR schedule without re-capture */,
                    void* stream);

/* ---------------------------------------------------------------------------------------
 * calm_optim_step with parameter groups (addition to ABI v7): tensor t is updated with the learning rate and the weight
 * decay of groups_dev[tensors_dev[t].group]; hparams->lr and hparams->weight_decay are ignored, beta1, beta2, eps,
 * max_norm and step / step_dev mean what they mean to calm_optim_step.  Passes 1 and 2 are calm_optim_step's own
 * kernels on the same scratch layout: the norm, the clip coefficient, found_inf and the step counter are taken over ALL
 * tensors of the table, whatever their group (clip_grad_norm_(model.parameters()) and torch's fused AdamW with several
 * param groups).  Pass 3 reads its group once per workgroup and then performs calm_optim_step's fp32 operations in
 * calm_optim_step's order: equal (lr, weight_decay) give equal bits.  An lr of 0 freezes a group's parameters while
 * its moments keep moving.
 * groups_dev: n_groups records in DEVICE memory, always — there is no lr_dev: a captured (hipGraph) step follows a
 * schedule of every group by the host rewriting this table between replays.
 * The entry point cannot see the device tables: the caller guarantees 0 <= group < n_groups for every tensor and
 * lr >= 0 for every group (backend.OptimPlan checks both on the host).
 * Three launches, no atomics, a fixed result per element; does not allocate or synchronise; captures into a hipGraph.
 * CALM_E_INVAL, before any launch: everything calm_optim_step refuses (hparams->lr aside), a null groups_dev,
 * n_groups <= 0.
 * ------------------------------------------------------------------------------------- */
typedef struct calm_optim_group { float lr, weight_decay; } calm_optim_group;   /* 8 bytes */
int calm_optim_step_groups(const calm_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev,
                           int32_t n_chunks, float* scratch, const calm_optim_hparams* hparams,
                           const calm_optim_group* groups_dev, int32_t n_groups,
                           const float* grad_scale /* device scalar or NULL */, float* stats_out, int32_t* step_dev,
                           void* stream);

/* ---------------------------------------------------------------------------------------
 * LAMB over calm_optim_step's table (addition to ABI v7): Adam's direction plus decoupled weight decay, rescaled per TENSOR
 * by the trust ratio ||w|| / ||update|| (You et al. 2020; which tensors adapt is timm's rule).  Four launches.  Tensor t
 * uses lr_t, wd_t = those of groups_dev[tensors_dev[t].group] when groups_dev != NULL (lr_dev is then ignored), else
 * hparams->lr (lr_dev[0] when lr_dev != NULL) and hparams->weight_decay.  All arithmetic in fp32, in this order:
 *   passes 1, 2  calm_optim_step's own kernels on its scratch layout (the first 6*n_tensors + 4 + 3*n_chunks floats): the
 *                gradient norm, the clip coefficient, found_inf and step_dev have the bits calm_optim_step gives them
 *   pass 3       g' = ((G - c u_i v_j) * (1/sigma)) * (clip / grad_scale)    (the first factor only with sn_sigma)
 *                m = m + (g' - m) * (1 - b1);   v = v * b2 + g'^2 * (1 - b2);   both stored
 *                r = (m / (sqrt(v) * (1 / sqrt(1 - b2^t)) + eps)) / (1 - b1^t)
 *                u = r + wd_t * w                                 (three roundings, never contracted into an fma)
 *                per chunk: sum w^2 and sum u^2, a thread's elements added serially, then the workgroup's tree; w is read only
 *   pass 4       W2, U2 = the tensor's chunk sums added in chunk order;  wn = sqrt(W2), un = sqrt(U2)
 *                trust = (adapt_t && wn > 0 && un > 0) ? wn / un : 1,   adapt_t = always_adapt || wd_t != 0
 *                trust_clip > 0:  trust = min(trust, trust_clip)
 *                lr_t != 0:  u recomputed from the stored m, v and the untouched w (the same bits as in pass 3),
 *                            w = w - (lr_t * trust) * u;    lr_t == 0: w keeps its bits, its moments have moved
 * found_inf: nothing is written — not w, m, v, not trust_out — and step_dev does not advance.
 * scratch: calm_optim_lamb_scratch_floats(n_tensors, n_chunks) floats (calm_optim_step's plus 2 per chunk).
 * trust_out (nullable, device): 3*n_tensors floats, (wn, un, trust) of every tensor on an applied step.
 * hparams->beta1, beta2, eps, max_norm, step / step_dev and stats_out mean what they mean to calm_optim_step.  As for
 * calm_optim_step_groups the caller guarantees 0 <= group < n_groups and lr >= 0 for every group.
 * No atomics, every sum in a fixed order, no result depends on the grid; does not allocate or synchronise; captures into a
 * hipGraph.  CALM_E_INVAL, before any launch: everything calm_optim_step (without groups_dev) / calm_optim_step_groups (with
 * it) refuse, a null lamb_hparams, a trust_clip that is NaN or negative, always_adapt outside {0, 1}, groups_dev with
 * n_groups <= 0.
 * ------------------------------------------------------------------------------------- */
typedef struct calm_lamb_hparams {
    float trust_clip;         /* 0: no upper limit on the trust ratio */
    int32_t always_adapt;     /* 1: tensors with wd_t == 0 get a trust ratio too */
} calm_lamb_hparams;
int64_t calm_optim_lamb_scratch_floats(int32_t n_tensors, int32_t n_chunks);   /* CALM_E_INVAL for a count <= 0 */
int calm_optim_step_lamb(const calm_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev,
                         int32_t n_chunks, float* scratch, const calm_optim_hparams* hparams,
                         const calm_lamb_hparams* lamb_hparams, const calm_optim_group* groups_dev /* nullable */,
                         int32_t n_groups, const float* grad_scale /* device scalar or NULL */, float* stats_out,
                         float* trust_out /* nullable */, int32_t* step_dev,
                         const float* lr_dev /* nullable, ignored with groups_dev */, void* stream);

/* ---------------------------------------------------------------------------------------
 * Gradient accumulation over micro-batches (addition to ABI v7), between a backward and calm_optim_step:
 *   acc[t][i] = first ? g'[i] : acc[t][i] + g'[i]
 * for every tensor t of calm_optim_step's table (tensors_dev / chunk_tensor_dev exactly as handed to it, gradient
 * pointers of THIS micro-batch), with g' = grad for a plain tensor and, for one with sn_sigma != NULL,
 *   g' = (G - <G, W_orig/sigma> u v^T) / sigma
 * evaluated with the u, v, sigma the table points at NOW: the deferred spectral-norm correction is applied per
 * micro-batch, because the power iteration advances u, v, sigma at every training forward.  The accumulators then hold
 * finished gradients; the window's optimizer step runs calm_optim_step over a table with sn_* = NULL and grad = acc, and
 * passes grad_scale * (number of micro-batches) as its grad_scale to average.
 * acc_dev: device array of n_tensors accumulator pointers (fp32, 4-byte aligned, numel elements each, overlapping
 * nothing else of the call).  scratch: n_chunks floats.  first = 1: the accumulators are written without being read
 * (they may hold anything, NaN included).  No unscale, no clip, no inf/NaN flag: a non-finite gradient stays non-finite
 * in the accumulator, where calm_optim_step's own check finds it.
 * Two launches, no atomics, <G, W_orig> summed per chunk and then in chunk order: a fixed result per element, bit-identical
 * on all data-parallel ranks given equal inputs.  Does not allocate or synchronise.
 * CALM_E_INVAL, before any launch: a null tensors_dev / chunk_tensor_dev / acc_dev / scratch, n_tensors <= 0,
 * n_chunks <= 0, first other than 0 or 1.
 * ------------------------------------------------------------------------------------- */
int calm_grad_accum(const calm_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev,
                    int32_t n_chunks, float* const* acc_dev, float* scratch, int32_t first, void* stream);

/* ---------------------------------------------------------------------------------------
 * Gradient monitor (addition to ABI v7), in front of calm_optim_step over the same table (tensors_dev / chunk_tensor_dev
 * exactly as handed to it, gradient pointers of THIS step): one calm_grad_stat per tensor, of the gradient the step is
 * about to apply before clipping, of the weights and of the Adam direction of the moments as they are now.  All in fp32:
 *   inv = grad_scale ? 1.0f / grad_scale[0] : 1.0f
 *   plain tensor:               g' = G[i] * inv
 *   tensor with sn_sigma != 0:  c = (sum over chunks of <G, W_orig>) / sigma, the per-chunk partials summed in the
 *                               thread / block order of calm_optim_step's first pass and then in chunk order (the bits
 *                               calm_optim_step and calm_grad_accum give c);
 *                               g' = ((G[i] - c * u[r] * v[col]) * (1.0f / sigma)) * inv
 *   grad_sq, param_sq, dir_sq:  a thread's serial sum over its (at most 64) elements of a chunk, the block sum (six
 *                               shuffle levels, three adds of the wave sums), then the tensor's chunks in chunk order.
 *                               g'^2 is summed element by element, never in the expanded |G|^2 - 2 c u^T G v + ... form
 *   grad_absmax, param_absmax:  exact maxima of the fp32 values
 *   nonfinite:                  the number of RAW G[i] with !(fabsf(G[i]) <= FLT_MAX).  An element whose g' is not finite is
 *                               left out of grad_sq and grad_absmax; a spectral-norm tensor with a non-finite G has a
 *                               non-finite c, so all of its elements are left out (grad_sq = grad_absmax = 0)
 *   dir_sq:                     t = step_dev ? step_dev[0] : hparams->step.  t < 1: 0, and the moments are not read.
 *                               Otherwise bc1 = 1.0f - powf(beta1, (float)t), bc2 likewise, and
 *                               d = (1.0f / bc1) * (m / (sqrtf(v) * (1.0f / sqrtf(bc2)) + eps)):
 *                               the AdamW update of the last applied step divided by its learning rate, without the
 *                               weight-decay term.  lr * sqrt(dir_sq / param_sq) is a tensor's update-to-weight ratio.
 * A chunk whose four operand addresses are 16-byte aligned is read as 16-byte vectors, any other as single words; the
 * thread that owns an element differs between the two, the summation depth does not.
 * Sticky fields and summary_dev[4] = {calls, bad_calls, first_bad_call, first_bad_tensor}: the last launch is one
 * workgroup.  calls += 1; if any tensor has nonfinite > 0, bad_calls += 1 and, the first time, first_bad_call = this
 * call's 0-based index and first_bad_tensor = the lowest such tensor; each such tensor's own bad_calls / first_bad_call
 * likewise.  The HOST initialises and resets them: counts 0, firsts -1 (in out_dev and in summary_dev).
 * Reads param, grad, exp_avg, exp_avg_sq, sn_*; writes out_dev, summary_dev and scratch
 * (calm_grad_stats_scratch_floats(n_tensors, n_chunks) floats, host-only query) and nothing else.  Three launches, no
 * atomics, no result depends on the grid; does not allocate or synchronise (capturable).  hparams: beta1, beta2, eps and
 * step are read.
 * CALM_E_INVAL, before any launch: a null tensors_dev / chunk_tensor_dev / hparams / out_dev / summary_dev / scratch,
 * n_tensors <= 0, n_chunks <= 0, a beta outside [0, 1).
 * ------------------------------------------------------------------------------------- */
typedef struct calm_grad_stat {      /* 32 bytes, one per tensor of the table */
    float   grad_sq;        /* sum g'^2 over the elements whose g' is finite                      (this call) */
    float   grad_absmax;    /* max |g'| over the same elements, 0 if none                         (this call) */
    float   param_sq;       /* sum p^2                                                            (this call) */
    float   param_absmax;   /* max |p|                                                            (this call) */
    float   dir_sq;         /* sum d^2, d = Adam direction of the moments as they are now         (this call) */
    int32_t nonfinite;      /* elements of the RAW gradient G that are inf / NaN                  (this call) */
    int32_t bad_calls;      /* calls so far in which nonfinite > 0                                (sticky)    */
    int32_t first_bad_call; /* 0-based index of the first such call, -1 until then                (sticky)    */
} calm_grad_stat;
int64_t calm_grad_stats_scratch_floats(int32_t n_tensors, int32_t n_chunks);
int calm_grad_stats(const calm_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev,
                    int32_t n_chunks, const calm_optim_hparams* hparams, const int32_t* step_dev, const float* grad_scale,
                    calm_grad_stat* out_dev, int32_t* summary_dev, float* scratch, void* stream);

/* ---------------------------------------------------------------------------------------
 * Sharpness-aware minimisation (additions to ABI v7): between the first backward of a step and its second forward,
 * calm_sam_perturb moves every parameter of calm_optim_step's table (tensors_dev / chunk_tensor_dev exactly as handed to
 * it, gradient pointers of the FIRST pass) by rho along the normalised TRUE gradient — corrected for the deferred
 * spectral-norm layers and unscaled, as calm_grad_stats documents it — IN PLACE, after saving its bits; behind the second
 * backward calm_sam_restore moves the saved bits back.  exp_avg and exp_avg_sq are not read.  All in fp32:
 *   inv = grad_scale ? 1.0f / grad_scale[0] : 1.0f
 *   plain tensor:               g' = G[i] * inv
 *   tensor with sn_sigma != 0:  c = (sum over chunks of <G, W_orig>) / sigma, the per-chunk partials summed in the
 *                               thread / block order of calm_optim_step's first pass and then in chunk order (the bits
 *                               calm_optim_step, calm_grad_accum and calm_grad_stats give c);
 *                               g' = ((G[i] - c * u[r] * v[col]) * (1.0f / sigma)) * inv
 *   s:                          adaptive == 0: s = g'.   adaptive == 1 (ASAM): t = fabsf(w[i]) + eta, s = t * g'
 *   norm = sqrtf(total):        per tensor, s^2 summed by a thread's serial sum over its (at most 64) elements of a chunk,
 *                               the block sum (six shuffle levels, three adds of the wave sums), then the tensor's chunks in
 *                               chunk order; then the tensors: 256 running sums, sum k adding tensors k, k + 256, k + 512,
 *                               ... in rising order, and the block sum over the 256
 *   found_inf:                  1 when any RAW G[i] has !(fabsf(G[i]) <= FLT_MAX), or when !(fabsf(norm) <= FLT_MAX); else 0
 *   scale:                      found_inf ? 0 : rho / (norm + eps)
 *   stats_out[3]                = {norm, found_inf, scale}
 *   apply:                      backup[t][i] = w[i] (the bits, always).  found_inf == 0: adaptive == 0:
 *                               w[i] = w[i] + scale * s;  adaptive == 1: w[i] = w[i] + (scale * t) * s, i.e. a step of
 *                               scale * t^2 * g'.  found_inf != 0: no parameter is written (and G is not read again)
 *   calm_sam_restore:           w[i] = backup[t][i], 32-bit words moved, no arithmetic: whatever the perturbed weights
 *                               were (they differ between data-parallel ranks whose first-pass gradients were not
 *                               exchanged), the restored ones are the saved bits
 * A chunk whose operand addresses are all 16-byte aligned (the gradient; the weights where they are read or written; the
 * backup in the apply pass and in the restore) is moved as 16-byte vectors, any other as single words; the thread that
 * owns an element differs between the two, the summation depth does not.
 * backup_dev: device array of n_tensors pointers (fp32 storage of numel elements each, 4-byte aligned, overlapping
 * nothing else of the call).  scratch: calm_sam_scratch_floats(n_tensors, n_chunks) floats (host-only query), written by
 * calm_sam_perturb and needed by nothing afterwards.  calm_sam_perturb writes param, the backups, scratch and stats_out;
 * calm_sam_restore writes param; neither writes anything else.  calm_sam_restore reads param / numel / chunk0 of the
 * table only: stale gradient pointers in it do not matter.
 * calm_sam_perturb: four launches, calm_sam_restore: one.  No atomics, no result depends on the grid; neither allocates
 * or synchronises (capturable).
 * CALM_E_INVAL, before any launch: a null tensors_dev / chunk_tensor_dev / hparams / backup_dev / scratch / stats_out
 * (calm_sam_restore: tensors_dev / chunk_tensor_dev / backup_dev), n_tensors <= 0, n_chunks <= 0, rho < 0 or NaN,
 * eps <= 0 or NaN, adaptive other than 0 or 1, and with adaptive == 1 eta < 0 or NaN.
 * ------------------------------------------------------------------------------------- */
typedef struct calm_sam_hparams { float rho, eps, eta; int32_t adaptive; } calm_sam_hparams;   /* 16 bytes */
int64_t calm_sam_scratch_floats(int32_t n_tensors, int32_t n_chunks);
int calm_sam_perturb(const calm_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev,
                     int32_t n_chunks, const calm_sam_hparams* hparams, const float* grad_scale /* device scalar or NULL */,
                     float* const* backup_dev, float* scratch, float* stats_out /* [3] */, void* stream);
int calm_sam_restore(const calm_optim_tensor* tensors_dev, int32_t n_tensors, const int32_t* chunk_tensor_dev,
                     int32_t n_chunks, const float* const* backup_dev, void* stream);

/* ---------------------------------------------------------------------------------------
 * Exponential moving average of ALL parameters (additions to ABI v7), a launch of its own behind calm_optim_step — the
 * weight EMA every ImageNet ViT recipe evaluates and checkpoints with (timm's ModelEmaV2 / torch's AveragedModel):
 *   ema += w * (src - ema),  w = 1 - d,  d = decay (CALM_EMA_CONSTANT) | min(decay, (1 + n) / (10 + n)) (CALM_EMA_WARMUP)
 * with n = count_dev[0], the number of updates applied so far; d is evaluated in fp32: nf = (float)n,
 * d = min(decay, (1.0f + nf) / (10.0f + nf)) with a correctly rounded division, w = 1.0f - d.
 *
 * entries_dev: table in device memory.  Work items are chunks of calm_ema_chunk_elems() consecutive elements of one
 * entry: chunk_entry_dev[k] = entry of chunk k, entry.chunk0 = its first chunk (as calm_cast_bf16 / calm_optim_step).
 * Any 4-byte aligned src / ema; a chunk whose src + i0 and ema + i0 are both 16-byte aligned moves 16-byte vectors.
 * src and ema of one entry, and the tensors of different entries, do not overlap.
 *
 * calm_ema_update — two launches.  The first (one thread) reads n and, when skip_dev (nullable device scalar, e.g.
 *   calm_optim_step's stats_out + 1) is given and non-zero, writes weight_out = {0, 1} and leaves count_dev alone;
 *   otherwise it writes weight_out = {w, 0} and count_dev[0] = n + 1.  The second (one workgroup per chunk) returns at
 *   once when weight_out[1] != 0 — a skipped update stores nothing — and otherwise applies w.  weight_out[2] (device)
 *   thereby reports the weight the call used.  No atomics, a fixed result per element: equal inputs give bit-identical
 *   averages on all data-parallel ranks.
 * calm_ema_swap — exchanges src and ema element for element (bits moved, no arithmetic): evaluation with the average
 *   while every cached parameter address (optimizer plan, bf16 weight copies, captured graphs) stays valid.
 * Neither allocates nor synchronises: both capture into a hipGraph.
 * CALM_E_INVAL, before any launch: a null entries_dev / chunk_entry_dev (and count_dev / weight_out for the update),
 * n_entries <= 0, n_chunks <= 0, decay outside [0, 1) or NaN, a schedule other than the two below.
 * ------------------------------------------------------------------------------------- */
typedef struct calm_ema_entry {      /* 32 bytes */
    float* src;        /* live parameter */
    float* ema;        /* its average */
    int64_t numel;
    int32_t chunk0;    /* index of this tensor's first chunk */
    int32_t reserved;  /* 0 */
} calm_ema_entry;
#define CALM_EMA_CONSTANT 0
#define CALM_EMA_WARMUP   1
int32_t calm_ema_chunk_elems(void);          /* multiple of 4 */
int calm_ema_update(const calm_ema_entry* entries_dev, int32_t n_entries, const int32_t* chunk_entry_dev,
                    int32_t n_chunks, float decay, int32_t schedule, int32_t* count_dev,
                    const float* skip_dev /* device scalar or NULL */, float* weight_out, void* stream);
int calm_ema_swap(const calm_ema_entry* entries_dev, int32_t n_entries, const int32_t* chunk_entry_dev,
                  int32_t n_chunks, void* stream);

/* ---------------------------------------------------------------------------------------
 * Training snapshots (additions to ABI v7): every state tensor of a run gathered into one contiguous device buffer in
 * one launch, and scattered back in place in one launch — what trainer.TrainState saves and resumes from.
 *   calm_snapshot_pack    packed[entry.offset + b] = entry.tensor[b]   for every entry, 0 <= b < entry.nbytes
 *   calm_snapshot_unpack  entry.tensor[b] = packed[entry.offset + b]
 * Bits are moved through integer registers (no arithmetic: NaN payloads and integer counters survive).  Work items are
 * chunks of calm_snapshot_chunk_bytes() consecutive bytes of one entry: chunk_entry_dev[k] = entry of chunk k,
 * entry.chunk0 = its first chunk (as calm_ema_swap).  One workgroup per chunk, every word moved by one thread: no atomics,
 * no workspace, nothing allocates or synchronises (both capture into a hipGraph).  `packed` is 16-byte aligned
 * (CALM_E_LAYOUT otherwise) and offsets are multiples of 16, so the packed side of every chunk is 16-byte aligned; a chunk
 * whose tensor side is too moves 16-byte vectors with a word tail, any other 4-byte aligned tensor moves single words.
 * The bytes of `packed` between two entries are never written by pack and never read by unpack.  The entries do not
 * overlap, in memory or in the buffer, and offset + nbytes <= packed_bytes: the host that builds the table checks it (a
 * record that leaves the buffer moves nothing).
 * CALM_E_INVAL, before any launch: a null entries_dev / chunk_entry_dev / packed, n_entries <= 0, n_chunks <= 0,
 * packed_bytes <= 0.
 * ------------------------------------------------------------------------------------- */
typedef struct calm_snapshot_entry {   /* 32 bytes */
    void*   tensor;      /* live tensor, 4-byte aligned, contiguous           */
    int64_t offset;      /* byte offset in the packed buffer, multiple of 16 */
    int64_t nbytes;      /* multiple of 4, > 0                               */
    int32_t chunk0;      /* index of this entry's first chunk                */
    int32_t reserved;    /* 0 */
} calm_snapshot_entry;
int32_t calm_snapshot_chunk_bytes(void);   /* multiple of 16 */
int calm_snapshot_pack(const calm_snapshot_entry* entries_dev, int32_t n_entries, const int32_t* chunk_entry_dev,
                       int32_t n_chunks, void* packed, int64_t packed_bytes, void* stream);
int calm_snapshot_unpack(const calm_snapshot_entry* entries_dev, int32_t n_entries, const int32_t* chunk_entry_dev,
                         int32_t n_chunks, const void* packed, int64_t packed_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Device-side batch collate feeding the path: uint8 images [B,3,H,W] -> normalised fp32 batch with
 * per-sample horizontal flip (flip[b] != 0; NULL = none) and the batch-level CutMix / MixUp of
 * distributed_trainer_cls.py:58-61 (torchvision.transforms.v2 semantics: partner = the batch rolled by one):
 *   mode 0 none | 1 MixUp: lam*x + (1-lam)*x_rolled | 2 CutMix: box = {y1,y2,x1,x2} (host ints) taken from x_rolled
 * mean/std: host float[3] (Normalize after ToDtype(scale=True), cls:137-139).  The random draws (lam ~ Beta, box,
 * flips) and the soft labels lam*onehot(y) + (1-lam)*onehot(y_rolled) are the caller's.
 * ------------------------------------------------------------------------------------- */
int calm_collate_mix(const uint8_t* img_u8, const uint8_t* flip, float* out, int32_t B, int32_t H, int32_t W,
                     int32_t mode, float lam, const int32_t* box, const float* mean, const float* std, void* stream);
/* ABI v5 — the same pass with the per-sample RandomCrop((H, W)) of distributed_trainer_cls.py:130 folded in and, optionally,
 * the output written directly as the row tokens the first Block consumes (Vi_Tools_CNN_less_V2.py:389-391):
 *   img_u8 [B,3,Hs,Ws] (the loader's Resize((256,256)) output, cls:129), crop_yx: DEVICE int32 [B,2] top-left corners
 *   (y0 in [0, Hs-H], x0 in [0, Ws-W]; NULL needs Hs == H, Ws == W); flips, mix and box act on the cropped window (the
 *   order of the reference's transform list: crop, ..., flip, ..., Normalize, then the batch-level CutMix / MixUp);
 *   out_tokens == 0: out [B,3,H,W];  != 0: out [B,H,3W] with out[b,i,3j+c] = image[b,c,i,j] (needs H == W for the model). */
int calm_collate_crop_mix(const uint8_t* img_u8, int32_t Hs, int32_t Ws, const int32_t* crop_yx, const uint8_t* flip,
                          float* out, int32_t B, int32_t H, int32_t W, int32_t out_tokens, int32_t mode, float lam,
                          const int32_t* box, const float* mean, const float* std, void* stream);

/* ---------------------------------------------------------------------------------------
 * Photometric augmentation fused into the collate (an addition to ABI v7 — no existing signature or struct changes, so
 * the version number stays).  calm_collate_crop_mix with the per-pixel transforms of distributed_trainer_cls.py:131-135
 * between the crop and Normalize, which the reference runs on PIL images in its DataLoader workers:
 *   ColorJitter(brightness, contrast, saturation, hue) cls:131, RandomSolarize cls:132, RandomHorizontalFlip cls:133,
 *   RandomGrayscale cls:134, GaussianBlur(3, sigma) cls:135.
 * Per sample, on the cropped H x W window in fp32 on [0, 1] from v = (float)u8 / 255.0f, in this order:
 *   1. the jitter operations order[0..3] (ids below; 255 or any other value = none, skipped; an id appears at most once),
 *      each blend(a, b, r) = clamp(r a + (1 - r) b, 0, 1) with gray = 0.2989 R + 0.587 G + 0.114 B:
 *        0 brightness: blend(x, 0, f)     1 contrast: blend(x, m, f), m = mean of gray over the window as the image stands
 *        2 saturation: blend(x, gray, f)    when contrast runs (after the operations in front of it in this order)
 *        3 hue: RGB -> HSV, h = (h + f) mod 1, HSV -> RGB (the hexcone formulas of Python's colorsys)
 *   2. solarize (flag): a channel value v >= solarize_thr becomes 1 - v
 *   3. horizontal flip (flag)             4. grayscale (flag): R = G = B = gray
 *   5. 3 x 3 Gaussian blur (flag), separable, w1 = exp(-0.5 / sigma^2), centre 1 / (1 + 2 w1), edge w1 / (1 + 2 w1),
 *      reflect padding at the edges of the WINDOW (-1 -> 1, H -> H - 2), never of the source image
 *   6. Normalize, then MixUp / CutMix with the partner (b - 1) mod B as calm_collate_crop_mix does — the partner goes
 *      through steps 1-5 with its own parameters, crop corner and contrast mean.
 * Nothing is rounded to 8 bits between the operations (the reference's PIL images are after each one).
 * samples_dev: DEVICE array [B].  Corners outside [0, Hs-H] x [0, Ws-W] are clamped into that range.  A blur flag needs
 * H >= 2 and W >= 2 (the flags live on the device: the caller checks).  gray_mean: DEVICE float [B], written by the first
 * of the two launches (one workgroup per sample, fixed summation order: repeats bit for bit; 0 for a sample without a
 * contrast operation) and read by the second.  out, out_tokens, mode, lam, box, mean, std: as calm_collate_crop_mix.
 * CALM_E_INVAL as calm_collate_crop_mix, and for a null samples_dev / gray_mean; CALM_E_UNSUPP for B > 65535 or
 * H * W > 2^30.
 * ------------------------------------------------------------------------------------- */
enum { CALM_AUG_FLIP = 1, CALM_AUG_SOLARIZE = 2, CALM_AUG_GRAYSCALE = 4, CALM_AUG_BLUR = 8 };          /* calm_aug_sample.flags */
enum { CALM_AUG_OP_BRIGHTNESS = 0, CALM_AUG_OP_CONTRAST = 1, CALM_AUG_OP_SATURATION = 2, CALM_AUG_OP_HUE = 3,
       CALM_AUG_OP_NONE = 255 };                                                                         /* .order[k]   */
typedef struct calm_aug_sample {   /* 48 bytes */
    int32_t  y0, x0;               /* crop corner */
    uint32_t flags;                /* CALM_AUG_* */
    uint8_t  order[4];             /* jitter operation ids in application order */
    float    brightness, contrast, saturation, hue;
    float    solarize_thr, blur_sigma;
    float    reserved[2];
} calm_aug_sample;

int calm_augment_collate(const uint8_t* img_u8, int32_t Hs, int32_t Ws, const calm_aug_sample* samples_dev,
                         float* gray_mean /* DEVICE [B], written */, float* out, int32_t B, int32_t H, int32_t W,
                         int32_t out_tokens, int32_t mode, float lam, const int32_t* box, const float* mean,
                         const float* std, void* stream);

/* ---------------------------------------------------------------------------------------
 * RandomErasing inside the augmenting collate (an addition to ABI v7 — no existing signature or struct changes, so the
 * version number stays).  calm_augment_collate with one more per-sample step between Normalize and the batch mix:
 *   e_s(c, y, x) = inside(box_s, y, x) ? fill_s(c, y, x) : normalised_s(c, y, x)
 * for every source sample s, where normalised_s is what calm_augment_collate computes for s up to and including
 * Normalize.  The box is in OUTPUT coordinates — rows y .. y + h - 1, columns x .. x + w - 1 of the H x W window, after
 * crop and flip; h == 0 or w == 0: the sample is not erased.  Erasing comes after the blur: an erased pixel is not
 * blurred, a pixel beside the box still blurs over the un-erased neighbours.  The mix then runs on e: MixUp is
 * e_b lam + e_pb (1 - lam), CutMix takes e_pb inside the CutMix box, pb = (b - 1) mod B — the partner is erased with ITS
 * box and ITS fill.
 *   value_mode 0: fill_s(c, y, x) = value[c] (host float[3], in normalised space)
 *   value_mode 1: per-pixel, per-channel standard normal noise (value is not read): with p = (s H + y) W + x,
 *     (w0, w1, w2, w3) = Philox4x32-10 of the counter (lo32(p), hi32(p), lo32(offset), hi32(offset)) under the key
 *     (lo32(seed), hi32(seed)) — the generator of calm_dropout —
 *       u1 = ((w0 >> 8) + 1) 2^-24,  u2 = (w1 >> 8) 2^-24,  u3 = ((w2 >> 8) + 1) 2^-24,  u4 = (w3 >> 8) 2^-24
 *       channel 0 = sqrt(-2 ln u1) cos(2 pi u2),  channel 1 = sqrt(-2 ln u1) sin(2 pi u2),  channel 2 = sqrt(-2 ln u3) cos(2 pi u4)
 *     in fp32 with the precise logf / sincospif / cospif; |n| <= sqrt(48 ln 2) = 5.77.  The fill is a function of
 *     (seed, offset, s, c, y, x) alone: not of the output sample that reads it, the tile, the store path or the layout.
 * boxes_dev: DEVICE array [B].  A box is only a predicate on output pixels: whatever a record holds, the kernel addresses
 * nothing outside `out`; it clips and checks nothing (the caller checks: 0 <= y, 0 <= x, y + h <= H, x + w <= W).  With
 * no box in the table the output and gray_mean equal calm_augment_collate's bit for bit.
 * CALM_E_INVAL / CALM_E_UNSUPP as calm_augment_collate, and CALM_E_INVAL for a null boxes_dev, a value_mode outside
 * {0, 1} and a null value in mode 0 — all before any launch.
 * ------------------------------------------------------------------------------------- */
typedef struct calm_erase_box {    /* 16 bytes */
    int32_t y, x, h, w;            /* top-left corner and size in output coordinates; h == 0 || w == 0: not erased */
} calm_erase_box;

int calm_augment_collate_erase(const uint8_t* img_u8, int32_t Hs, int32_t Ws, const calm_aug_sample* samples_dev,
                               float* gray_mean /* DEVICE [B], written */, float* out, int32_t B, int32_t H, int32_t W,
                               int32_t out_tokens, int32_t mode, float lam, const int32_t* box, const float* mean,
                               const float* std, const calm_erase_box* boxes_dev, int32_t value_mode, const float* value,
                               uint64_t seed, uint64_t offset, void* stream);

/* ---------------------------------------------------------------------------------------
 * Device resize over a ragged uint8 batch (an addition to ABI v7 — no existing signature or struct changes, so the
 * version number stays).  The first transform of the reference's list, transforms.Resize((256, 256)) on a PIL image
 * (distributed_trainer_cls.py:129), is Image.resize((ow, oh), BILINEAR): antialiased, a horizontal pass and then a
 * vertical pass, the intermediate rounded to uint8, coefficients computed per axis in double and converted to 22-bit
 * fixed point.  Per axis, with `in` source and `out` output pixels:
 *   scale = (double)in / out;  fs = max(scale, 1.0);  support = fs;  ss = 1.0 / fs
 *   output o:  center = (o + 0.5) * scale
 *              lo = max((int)(center - support + 0.5), 0);  hi = min((int)(center + support + 0.5), in);  n = hi - lo
 *              w[j] = tri((j + lo - center + 0.5) * ss) for j < n,  tri(t) = max(1 - |t|, 0)
 *              ww = w[0] + w[1] + ... (in this order);  w[j] /= ww when ww != 0
 *              k[j] = (int)(0.5 + w[j] * 4194304.0)                                            (1 << 22)
 *   pixel:     acc = (1 << 21) + sum_j src[lo + j] * k[j];  result = clamp(acc >> 22, 0, 255)
 * every floating-point operation a single IEEE double operation (no fused multiply-add).  From the coefficients on the
 * arithmetic is integer, so the output equals PIL's byte for byte; a source of the output's size comes back unchanged.
 *
 * calm_resize_coeffs: the definition of those coefficients, on the host (no GPU, no launch).  bounds[2 o], bounds[2 o + 1]
 *   = lo, n of output pixel o; kk[o * ksize + j] = k[j], zero for n <= j < ksize.  ksize >= 2 * ceil(max(in / out, 1)) + 1
 *   always holds every pixel's taps.  CALM_E_INVAL: a null pointer, in / out / ksize <= 0, a pixel with more than ksize
 *   taps (nothing is written then); CALM_E_UNSUPP: in or out above 16384.
 * calm_resize_u8: one launch.  packed: DEVICE byte buffer of nbytes bytes holding B images, image b as h x w x 3 uint8,
 *   interleaved (the bytes of np.asarray(pil_image)), at byte offset samples_dev[b].offset — any offset, any base
 *   alignment.  samples_dev: DEVICE array [B].  out: DEVICE uint8 [B, 3, oh, ow], planar, the layout
 *   calm_collate_crop_mix and calm_augment_collate read.  Source sides from 1 to 16384, up- and downscaling.  The records
 *   live on the device, so the launch cannot refuse one: a record with h or w outside [1, 16384] or with
 *   offset + 3 h w > nbytes is not read and its output is zeros (the caller that holds the sizes on the host checks them;
 *   trainer.DeviceResize does).  Deterministic: no atomics, every output byte written once.
 *   CALM_E_INVAL: a null packed / samples_dev / out, nbytes <= 0, B <= 0, oh <= 0 or ow <= 0;
 *   CALM_E_UNSUPP: B > 65535, oh or ow above 16384.  All of them before any launch.
 * ------------------------------------------------------------------------------------- */
typedef struct calm_resize_sample {   /* 16 bytes */
    int64_t offset;                   /* of the image's first byte in `packed` */
    int32_t h, w;                     /* source rows, columns */
} calm_resize_sample;

int calm_resize_coeffs(int32_t in, int32_t out, int32_t* bounds /* [2 * out] */, int32_t* kk /* [out * ksize] */,
                       int32_t ksize);
int calm_resize_u8(const uint8_t* packed, int64_t nbytes, const calm_resize_sample* samples_dev, uint8_t* out /* [B,3,oh,ow] */,
                   int32_t B, int32_t oh, int32_t ow, void* stream);

/* ---------------------------------------------------------------------------------------
 * Device resized crop (an addition to ABI v7 — no existing signature or struct changes, so the version number stays):
 * calm_resize_u8 with a per-sample source box, a per-sample output size and an output window, i.e. what
 * Image.crop((bx0, by0, bx0 + bw, by0 + bh)).resize((vw, vh), BILINEAR) returns — torchvision's resized_crop on a PIL
 * image — of which only the H x W pixels from (wy0, wx0) on are computed:
 *   out[b, :, y, x] = pixel (wy0 + y, wx0 + x) of resize(crop(image_b, box_b), (vh_b, vw_b)).
 * One launch covers Resize(int) + CenterCrop (box = the image, vh x vw = the aspect-preserving size, the window = the
 * central crop), RandomResizedCrop (a random box, vh x vw = H x W, window at (0, 0)) and Resize(size) + RandomCrop
 * (box = the image, window = the crop).
 * The contract is the per-axis formulas above — the horizontal pass, rounded to uint8, then the vertical pass — with
 * `in` = bw / bh, `out` = vw / vh and the source indices shifted by bx0 / by0; pixels outside the box are never read
 * (this is crop-then-resize: Image.resize(size, BILINEAR, box=box) is a different function, it reads pixels around the
 * box).  PIL returns the same bytes for sources whose sides are within a factor of about 100 of one another; on very
 * tall and narrow ones (w = 2 .. 6 with h above roughly 100 w, downscaled vertically) PIL 12.2.0 runs the vertical pass
 * first and a few bytes differ.  There the contract is these formulas, as it is for calm_resize_u8.
 * out_kind: 0  uint8 [B,3,H,W] planar, the layout calm_collate_crop_mix and calm_augment_collate read;
 *           1  fp32 [B,3,H,W], n(v) = (v / 255 - mean[c]) / std[c];
 *           2  fp32 row tokens [B,H,3W], out[b,i,3j+c] = n(v) of channel c at (i, j) (what the first Block consumes).
 * mean, std: HOST float[3], required for kinds 1 and 2, ignored for kind 0.  In fp32 n(v) is evaluated as
 *   fma((float)v, 1.0f / 255.0f, -mean[c]) * (1.0f / std[c]), three roundings, the same on every launch.
 * A record is valid when 1 <= h, w <= 16384, the image lies inside nbytes, by0, bx0 >= 0, bh, bw >= 1, by0 + bh <= h,
 * bx0 + bw <= w, 1 <= vh, vw <= 16384, wy0, wx0 >= 0, wy0 + H <= vh and wx0 + W <= vw, evaluated in 64-bit by one
 * function (csrc/rcrop_check.h) that the kernel calls before it forms any address and that calm_resized_crop_check
 * exposes on the host (no GPU, no launch; a null sample is invalid).  The records live on the device, so the launch cannot
 * refuse one: an invalid record is never read and its output is what an all-zero source gives — zeros for kind 0, n(0)
 * for kinds 1 and 2 (trainer.DeviceResizedCrop refuses it on the host).  packed: any offsets, any base alignment; no
 * dword is loaded that does not hold a byte of the image.  Deterministic: no atomics, every output element written once.
 *   CALM_E_INVAL: a null packed / samples_dev / out, nbytes <= 0, B <= 0, H <= 0 or W <= 0, an out_kind outside 0 .. 2,
 *     a null mean or std for kinds 1 and 2;
 *   CALM_E_UNSUPP: B > 65535, H or W above 16384.  All of them before any launch.
 * ------------------------------------------------------------------------------------- */
typedef struct calm_rcrop_sample {   /* 48 bytes */
    int64_t offset;                   /* of the image's first byte in `packed`, as calm_resize_sample */
    int32_t h, w;                     /* source rows, columns */
    int32_t by0, bx0, bh, bw;         /* source box: PIL crop((bx0, by0, bx0 + bw, by0 + bh)) */
    int32_t vh, vw;                   /* the size the box is resized to */
    int32_t wy0, wx0;                 /* top-left of the output window inside vh x vw */
} calm_rcrop_sample;

int calm_resized_crop(const uint8_t* packed, int64_t nbytes, const calm_rcrop_sample* samples_dev, void* out, int32_t B,
                      int32_t H, int32_t W, int32_t out_kind, const float* mean, const float* std, void* stream);
int calm_resized_crop_check(const calm_rcrop_sample* sample /* HOST */, int64_t nbytes, int32_t H, int32_t W);  /* 1 valid, 0 not */

/* ---------------------------------------------------------------------------------------
 * Device RandAugment (an addition to ABI v7 — no existing signature or struct changes, so the version number stays): a
 * uint8 -> uint8 stage between the uint8 batch and the collate.  img_u8 [B,3,Hs,Ws] -> out [B,3,H,W]; per sample the
 * RandomCrop window (corner clamped into [0, Hs-H] x [0, Ws-W] as calm_augment_collate clamps it) and the horizontal
 * flip first — the order of the reference's transform list — then a chain of up to CALM_RA_MAX_OPS operations, each
 * rounded to uint8 as PIL rounds it: the output equals, byte for byte, what PIL 12 gives for the same chain on
 * Image.fromarray(window).  The semantics are torchvision.transforms.v2.RandAugment's on a PIL image, restated.
 *
 * CALM_RA_OP_AFFINE (ShearX, ShearY, TranslateX, TranslateY, Rotate): nearest-neighbour affine in PIL's 16.16 fixed
 *   point on the H x W window, never on source pixels outside the crop.  The host has six doubles a[0..5], the inverse
 *   map (output -> input): ShearX s (1, s, 0, 0, 1, 0); ShearY s (1, 0, 0, s, 1, 0); TranslateX by an integer t
 *   (1, 0, -t, 0, 1, 0); TranslateY (1, 0, 0, 0, 1, -t); Rotate by `angle` degrees counter-clockwise about (W/2, H/2),
 *   Image.rotate's matrix: r = -radians(angle % 360), m = (round(cos r, 15), round(sin r, 15), 0, round(-sin r, 15),
 *   round(cos r, 15), 0), m[2] = m[0] (-W/2) + m[1] (-H/2) + W/2, m[5] = m[3] (-W/2) + m[4] (-H/2) + H/2.  It converts
 *   them with FIX(v) = floor(v * 65536 + 0.5): coef = (FIX(a0), FIX(a1), FIX(a2 + a0 * 0.5 + a1 * 0.5), FIX(a3), FIX(a4),
 *   FIX(a5 + a3 * 0.5 + a4 * 0.5)) = (A0 .. A5), and the device computes
 *     xin = (A2 + A1 y + A0 x) >> 16,  yin = (A5 + A4 y + A3 x) >> 16      (arithmetic shift)
 *     out[c][y][x] = 0 <= xin < W && 0 <= yin < H ? window[c][yin][xin] : fill[c]
 *   Integer translations and the identity agree with PIL's separate scale-only path; bit parity with non-integer
 *   translations is not claimed.  32 bits suffice: x, y < 4096 = 2^12, so with |A0|, |A1|, |A3|, |A4| <= 2^17 (|a| <= 2:
 *   every shear, rotation and translation) and |A2|, |A5| <= 2^30 (an offset below 16384 pixels) each sum stays below
 *   2^29 + 2^29 + 2^30 = 2^31.  trainer.DeviceRandAugment.check refuses a record outside those bounds; the device
 *   evaluates the sums in wrapping 32-bit arithmetic, so any other record still gives a defined pixel or the fill.
 * blend(d, s, f) is Image.blend: in fp32, t = d + f * (s - d), every operation one IEEE rounding and no fused
 *   multiply-add; for 0 <= f <= 1 the result is (uint8)(int)t, otherwise 0 for t <= 0, 255 for t >= 255, (int)t between.
 *   L(R, G, B) = (19595 R + 38470 G + 7471 B + 32768) >> 16.
 *   CALM_RA_OP_BRIGHTNESS blend(0, x, f);  CALM_RA_OP_COLOR blend(L, x, f) per channel;
 *   CALM_RA_OP_CONTRAST blend(m, x, f), m = floor((2 sum L + n) / (2 n)) over the n window pixels as the image stands
 *     when the operation runs (= int(mean + 0.5));
 *   CALM_RA_OP_SHARPNESS blend(smooth(x), x, f), smooth = ImageFilter.SMOOTH: on interior pixels acc = 0.5f, then
 *     acc += p * k for the nine taps in row-major order with k = (1,1,1,1,5,1,1,1,1), each entry divided by 13 in fp32,
 *     result clamp((int)acc, 0, 255); the outermost rows and columns are copied; a window with H < 3 or W < 3 is copied.
 * CALM_RA_OP_POSTERIZE v & (0xFF << (8 - param)), param = bits; bits outside 0 .. 8 are treated as 8.
 * CALM_RA_OP_SOLARIZE  v < param ? v : 255 - v.
 * CALM_RA_OP_AUTOCONTRAST per channel: lo, hi = the channel's min and max; hi <= lo: unchanged; otherwise in IEEE
 *   double, single operations, a correctly rounded division: scale = 255.0 / (hi - lo), off = -lo * scale,
 *   lut[i] = clamp((int)(i * scale + off), 0, 255).
 * CALM_RA_OP_EQUALIZE per channel, h the 256-bin histogram: fewer than two non-empty bins: unchanged;
 *   step = (sum h - h[last non-empty]) / 255 in integers, step == 0: unchanged; otherwise
 *   lut[i] = min((step / 2 + sum_{j < i} h[j]) / step, 255) in integers.
 * CALM_RA_OP_IDENTITY and every id outside the table: the slot is skipped.
 *
 * samples_dev: DEVICE array [B].  A sample runs its first min(n_ops, n_slots) slots (n_ops < 0 counts as 0).  The records
 * live on the device, so the host says what the batch needs: n_slots (0 .. CALM_RA_MAX_OPS) is the number of slot passes
 * launched, and bit k of stats_mask says that some sample has CONTRAST, AUTOCONTRAST or EQUALIZE in slot k — that slot is
 * then preceded by a statistics launch (R / G / B / L histograms per sample: LDS-private counts, then integer atomics,
 * so the result repeats bit for bit; there is no floating-point atomic anywhere).  One of those three operations in a
 * slot whose bit is not set is skipped.  Whatever a record holds, the kernels address nothing outside their buffers.
 * fill: HOST uint8[3], NULL = (0, 0, 0).  scratch: DEVICE, at least calm_randaugment_scratch_bytes(B, H, W) bytes, 16-byte
 * aligned: two ping-pong images [B,3,H,W] and 4 x 256 int32 histograms per sample.  out must not overlap img_u8.
 *   CALM_E_INVAL: a null img_u8 / samples_dev / out / scratch, B <= 0, H or W <= 0, H > Hs or W > Ws, n_slots outside
 *     0 .. CALM_RA_MAX_OPS, scratch_bytes below calm_randaugment_scratch_bytes(B, H, W);
 *   CALM_E_UNSUPP: B > 65535, H or W above CALM_RA_MAX_SIDE.  All of them before any launch.
 *   calm_randaugment_scratch_bytes: the size, or CALM_E_INVAL / CALM_E_UNSUPP for the same B, H, W.
 * ------------------------------------------------------------------------------------- */
#define CALM_RA_MAX_OPS 4
#define CALM_RA_MAX_SIDE 4096
enum { CALM_RA_OP_IDENTITY = 0, CALM_RA_OP_AFFINE = 1, CALM_RA_OP_BRIGHTNESS = 2, CALM_RA_OP_COLOR = 3, CALM_RA_OP_CONTRAST = 4,
       CALM_RA_OP_SHARPNESS = 5, CALM_RA_OP_POSTERIZE = 6, CALM_RA_OP_SOLARIZE = 7, CALM_RA_OP_AUTOCONTRAST = 8,
       CALM_RA_OP_EQUALIZE = 9 };
typedef struct calm_ra_sample {    /* 160 bytes */
    int32_t  y0, x0;                        /* crop corner */
    uint32_t flip;                          /* != 0: horizontal flip of the window */
    int32_t  n_ops;                         /* slots in use, 0 .. CALM_RA_MAX_OPS */
    int32_t  op[CALM_RA_MAX_OPS];           /* CALM_RA_OP_* per slot */
    float    factor[CALM_RA_MAX_OPS];       /* f of the four blends */
    int32_t  param[CALM_RA_MAX_OPS];        /* posterize bits, solarize threshold */
    int32_t  coef[CALM_RA_MAX_OPS][6];      /* A0 .. A5 of CALM_RA_OP_AFFINE */
} calm_ra_sample;

int64_t calm_randaugment_scratch_bytes(int32_t B, int32_t H, int32_t W);
int calm_randaugment_u8(const uint8_t* img_u8, int32_t Hs, int32_t Ws, const calm_ra_sample* samples_dev,
                        uint8_t* out /* [B,3,H,W] */, int32_t B, int32_t H, int32_t W, int32_t n_slots, uint32_t stats_mask,
                        const uint8_t* fill /* HOST [3] or NULL */, void* scratch, int64_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Tokenisation (bit-exact index work).
 * image_to_rows : rows[b,i,3j+c] = img[b,c,i,j]           (Vi_Tools:389-391); rows_to_image inverse.
 * grid_transpose: out[b,j,3i+c]  = in[b,i,3j+c]           (Vi_Tools:394-395,397-398; self-inverse)
 * ------------------------------------------------------------------------------------- */
int calm_image_to_rows(const float* img, float* rows, int32_t B, int32_t S, void* stream);
int calm_rows_to_image(const float* rows, float* img, int32_t B, int32_t S, void* stream);
int calm_grid_transpose(const float* in, float* out, int32_t B, int32_t S, void* stream);

/* ---------------------------------------------------------------------------------------
 * Depthwise 3x3 conv (padding 1, zeros) + bias on a channels-last [B,S,S,C] grid
 * (middle layer of Block.proj, Vi_Tools:382; CALM_ViT_V2.py:64).  w: [C,3,3], bias: [C].
 * act: CALM_ACT_NONE/GELU; y_pre (optional) receives the pre-activation.
 * bwd: dx from dz (gradient wrt the pre-activation); dw[C,9], db[C] accumulated (caller zeroes; fp32 atomics —
 * a standalone helper, the path runs the convolutions fused in calm_cnn_residual_*).
 * ------------------------------------------------------------------------------------- */
int calm_dwconv3x3_fwd(const float* x, const float* w, const float* inv_scale, const float* bias,
                       float* y, float* y_pre, int32_t act, int32_t B, int32_t S, int32_t C, void* stream);
int calm_dwconv3x3_bwd(const float* dz, const float* x, const float* w, const float* inv_scale,
                       float* dx, float* dw, float* db, int32_t B, int32_t S, int32_t C, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused CNN residual of Block.proj / ViT.proj (Vi_Tools:378-385,400-403; CALM_ViT_V2.py:60-67,80-83):
 *   out = x + conv1x1_{hidden->3}(gelu(dwconv3x3(gelu(conv1x1_{3->hidden}(x)))))   on [B,S,S,3] tokens.
 * w0:[hidden,3] w2:[hidden,9] w4:[3,hidden] are the *_orig weights, s0/s2/s4 their device sigmas.
 * The hidden maps stay in LDS per 16x16 tile; backward recomputes them.  bwd writes dx and ADDS (fixed order through
 * `partials`) the gradients wrt the effective weights W/sigma (g0,g2,g4) and biases onto the caller's tensors.
 * hidden must be 32.  residual (ABI v7): 1 = the form above (Block.forward / ViT.forward, Vi_Tools:400-403); 0 = the bare
 * `proj(x)` a caller of the reference may invoke on its own (out = conv(...), dx without the skip term).
 * ------------------------------------------------------------------------------------- */
int calm_cnn_residual_fwd(const float* x, const float* w0, const float* s0, const float* b0, const float* w2,
                          const float* s2, const float* b2, const float* w4, const float* s4, const float* b4,
                          float* out, int32_t B, int32_t S, int32_t hidden, int32_t residual, void* stream);
int calm_cnn_residual_bwd(const float* dy, const float* x, const float* w0, const float* s0, const float* b0,
                          const float* w2, const float* s2, const float* b2, const float* w4, const float* s4,
                          const float* b4, float* dx, float* g0, float* gb0, float* g2, float* gb2, float* g4,
                          float* gb4, int32_t B, int32_t S, int32_t hidden, int32_t residual, float* partials,
                          void* stream);

/* ---------------------------------------------------------------------------------------
 * Small streaming helpers.
 * add          : out = a + b                         (residual / U-net skips, Vi_Tools:309,315,403,513-522)
 * gelu_fwd     : y = gelu_erf(x)                     (ABI v7: the GELU module called on its own; fused everywhere else)
 * gelu_bwd     : dz = dy * gelu'(z)                  (where it is not fused into a GEMM epilogue)
 * colsum       : out[n] += sum_m x[m,n]              (bias gradients; fixed order through `partials`)
 * row_scale    : out[r,c] = x[r,c] * s[r]            (ls-scaled weight for the dgrad of out_proj/mlp.3; fp32 or bf16 out)
 * mean_seq     : y[b,d] = mean_s x[b,s,d]            (AdaptiveAvgPool1d, CALM_ViT_V2.py:74-75) and bwd
 * ------------------------------------------------------------------------------------- */
int calm_add(const float* a, const float* b, float* out, int64_t n, void* stream);
int calm_gelu_fwd(const float* x, float* y, int64_t n, void* stream);
int calm_gelu_bwd(const float* dy, const float* z, float* dz, int64_t n, void* stream);
int calm_colsum(const void* x, float* out, int64_t rows, int32_t cols, int32_t x_type /* CALM_ST_* */,
                float* partials /* ABI v7 */, void* stream);
int calm_row_scale(const float* x, const float* s, void* out, int32_t rows, int32_t cols, int32_t out_type /* CALM_ST_* */,
                   void* stream);
int calm_mean_seq_fwd(const float* x, float* y, int32_t B, int32_t S, int32_t D, void* stream);
int calm_mean_seq_bwd(const float* dy, float* dx, int32_t B, int32_t S, int32_t D, void* stream);

/* ---------------------------------------------------------------------------------------
 * Dropout with a counter-based mask (an addition to ABI v7; nn.Dropout at Vi_Tools:301 and inside the MLP, Vi_Tools:203).
 * For j in [0, n), e = e0 + j:
 *     y[j] = x[j] * (word(e) >= thr ? scale : 0) + (residual ? residual[j] : 0)
 *   word(e) = output word (e & 3) of Philox4x32-10 with counter (lo32(e >> 2), hi32(e >> 2), lo32(offset), hi32(offset)),
 *             key (lo32(seed), hi32(seed)), multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85;
 *   thr = (uint32_t)((double)p * 2^32),  scale = 1.0f / (1.0f - p)   (fp32; computed by the entry point).
 * key: DEVICE uint64[2] = (seed, offset), read by the kernel — no host synchronisation, valid inside a captured graph.  The
 * mask depends on (seed, offset, e) only: the backward passes the forward's key and gets the forward's mask, so no mask is
 * ever stored.  e0 (a multiple of 4) lets a caller cover one logical tensor with several calls.
 * One fp32 multiply and one fp32 add, each rounded on its own (the add is skipped without a residual); bf16 inputs widen
 * exactly, a bf16 output is one round-to-nearest-even of the fp32 result.  A multiply, not a select: a dropped NaN / inf
 * yields NaN (torch.nn.functional.dropout does the same).  y may alias x.  x_type / r_type / y_type: CALM_ST_F32 or
 * CALM_ST_BF16.  CALM_E_INVAL: null x / y / key, n < 0, p outside [0, 1), e0 < 0 or e0 % 4 != 0, another storage type.
 * n == 0 returns 0 without a launch.
 * ------------------------------------------------------------------------------------- */
int calm_dropout(const void* x, const void* residual /* nullable */, void* y, int64_t n, int64_t e0, float p,
                 const uint64_t* key /* device, [2] = seed, offset */, int32_t x_type, int32_t r_type, int32_t y_type,
                 void* stream);

/* ---------------------------------------------------------------------------------------
 * Stochastic depth with the mask of calm_dropout, one decision per sample (an addition to ABI v7; timm's drop_path,
 * torchvision's StochasticDepth(mode="row"); no counterpart in the reference).  x, residual, y: [B, L], rows contiguous.
 *     y[b, j] = x[b, j] * f_b + (residual ? residual[b, j] : 0),      f_b = word(sample0 + b) >= thr ? scale : 0
 * word(s), thr and scale are calm_dropout's (word(s) is what that entry point uses for element index s), so the keep
 * decisions of a call are those of elements sample0 .. sample0 + B - 1 of a calm_dropout mask under the same key and p:
 * a function of (seed, offset, sample0 + b) only — not of L, the grid, the vector width, the storage types or of how a
 * batch is split into calls.  sample0 >= 0 is ANY value (no multiple of 4 is asked for).
 * key: DEVICE uint64[2] = (seed, offset), read by the kernel — no host synchronisation, valid inside a captured graph.  The
 * backward is the same entry point: dx = calm_drop_path(dy, NULL, ...) with the forward's key, dresidual = dy.
 * One fp32 multiply and one fp32 add, each rounded on its own (the add is skipped without a residual); bf16 inputs widen
 * exactly, a bf16 output is one round-to-nearest-even of the fp32 result.  A multiply, not a select: a NaN / inf in a
 * dropped sample yields NaN (timm's x * mask does the same).  y may alias x.  Rows move as 16-byte vectors when every base
 * is 16-byte aligned and L is a multiple of the unit (4 elements with all tensors fp32, 8 with any bf16), else element by
 * element.  No LDS, no atomics.  x_type / r_type / y_type: CALM_ST_F32 or CALM_ST_BF16.
 * CALM_E_INVAL: null x / y / key, B < 0, L < 0, sample0 < 0, p outside [0, 1), another storage type.  B == 0 or L == 0
 * returns 0 without a launch.
 * ------------------------------------------------------------------------------------- */
int calm_drop_path(const void* x, const void* residual /* nullable */, void* y, int64_t B, int64_t L, int64_t sample0,
                   float p, const uint64_t* key /* device, [2] = seed, offset */, int32_t x_type, int32_t r_type,
                   int32_t y_type, void* stream);

/* ---------------------------------------------------------------------------------------
 * The loss end of the step (additions to ABI v7 — no existing signature or struct changes, so the version number
 * stays): logits -> loss and loss -> dL/dlogits as entry points, so that a host driving this boundary without torch can
 * train (forward, one of these, backward, calm_optim_step).  Logits are fp32 (module outputs stay fp32 in every
 * precision mode).  Cross-workgroup sums go through `partials` (calm_reduce_scratch_floats with CALM_RED_SOFT_CE /
 * CALM_RED_HUBER) and one final workgroup that adds them in a fixed order: no atomics, results repeat bit for bit.
 *
 * calm_soft_ce_fwd / _bwd: nn.CrossEntropyLoss() with class-probability targets (distributed_trainer_cls.py:63,86; the
 *   CutMix / MixUp labels of cls:58-61), mean over the batch.  ld / td: row strides in elements (rows are read as 16-byte
 *   vectors where pointers and strides allow, element by element otherwise).  The row maximum is subtracted before the
 *   exponential in both directions; targets need not sum to one.  row_stats [B,2] (row maximum, log sum exp(z - max)) is
 *   what the backward needs besides its inputs.  dloss is a DEVICE scalar: it carries GradScaler's scale (cls:87).
 * metrics (nullable): caller-owned device float[4], updated in place by the last launch of calm_soft_ce_fwd with a plain
 *   read-modify-write of one thread (ordered by the stream):
 *     [0] += sum of the B row losses     [1] += #{b : argmax_c z[b,:] == argmax_c y[b,:]}  (the "dominant class"
 *     [2] += B                                  accuracy of cls:98-102; ties go to the lowest index, a row holding a
 *     [3] += 1                                  NaN counts as no agreement)
 *   The counts are exact below 2^24.  A training loop reads them once per epoch instead of `loss.item()` per step (cls:97).
 * calm_top1_count: the eval loop's top-1 count against integer labels (CALM_ViT_V2.py:228-239): metrics[1] += hits,
 *   metrics[2] += B; [0] and [3] are left alone.
 * calm_huber_tokens_fwd / _bwd: nn.HuberLoss(delta) between the generative model's token output and the input image
 *   (distributed_trainer_reg.py:59,78-81): tokens [B,S,3S] ARE the channels-last image, so the reference's
 *   reshape(-1,S,S,3).permute(0,3,1,2) costs nothing here — the interleave against x [B,3,S,S] happens in LDS, both
 *   tensors are read (and dtokens written) as 16-byte vectors.  S % 4 == 0 and S <= 4096, CALM_E_UNSUPP otherwise;
 *   16-byte aligned bases, CALM_E_LAYOUT otherwise.
 * ------------------------------------------------------------------------------------- */
/* loss = mean_b sum_c y[b,c] * (logsumexp(z[b,:]) - z[b,c])          (cls:63,86; CrossEntropyLoss with class-probability targets) */
int calm_soft_ce_fwd(const float* logits, int64_t ld, const float* targets, int64_t td,
                     float* row_stats /* [B,2]: row maximum, log(sum exp(z - max)) */,
                     float* loss /* scalar, overwritten */, float* metrics /* nullable, [4], see above */,
                     int32_t B, int32_t C, float* partials, void* stream);
/* dlogits[b,c] = dloss/B * (exp((z - max_b) - logsum_b) * sum_c y[b,c] - y[b,c]);  dloss: device scalar (carries GradScaler's scale) */
int calm_soft_ce_bwd(const float* logits, int64_t ld, const float* targets, int64_t td, const float* row_stats,
                     const float* dloss, float* dlogits /* [B,C] contiguous */, int32_t B, int32_t C, void* stream);
/* loss = mean over B*3*S*S of huber_delta(tokens[b,i,3j+c] - x[b,c,i,j])   (reg:59,78-81; tokens [B,S,3S], x [B,3,S,S]) */
int calm_huber_tokens_fwd(const float* tokens, const float* x, float delta, float* loss, int32_t B, int32_t S,
                          float* partials, void* stream);
/* dtokens[b,i,3j+c] = dloss/(3*B*S*S) * clamp(tokens[b,i,3j+c] - x[b,c,i,j], -delta, delta) */
int calm_huber_tokens_bwd(const float* tokens, const float* x, float delta, const float* dloss, float* dtokens,
                          int32_t B, int32_t S, void* stream);
/* metrics[1] += #{b : argmax_c z[b,:] == labels[b]},  metrics[2] += B        (CALM_ViT_V2.py:228-239) */
int calm_top1_count(const float* logits, int64_t ld, const int64_t* labels, float* metrics, int32_t B, int32_t C, void* stream);

/* ---------------------------------------------------------------------------------------
 * Validation metrics (an addition to ABI v7 — no existing signature or struct changes, so the version number stays):
 * top-k hits, the cross-entropy sum, per-class support / top-1 hits and (optionally) the confusion matrix of one batch of
 * logits against integer labels, ADDED to caller-owned device accumulators by two launches.  No atomics: every counter
 * has one owning thread, the loss is added in a fixed order, results repeat bit for bit.
 *
 * logits [B,C], row stride ld elements, logits_type CALM_ST_F32 or CALM_ST_BF16 (rows are read as 16-byte vectors where
 * the base is 16-byte aligned and ld is a multiple of the 4 / 8 elements of one, element by element otherwise); labels [B] int64.
 *   row kernel (one wave per row, four rows per workgroup): writes one 16-byte record per row into `partials`
 *   (calm_reduce_scratch_floats(CALM_RED_EVAL, B, C) = 4 * B floats, 16-byte aligned):
 *       { float nll = (max - z_l) + log(sum exp(z - max));  int32 beaten;  int32 pred;  int32 flags }
 *     beaten = #{c : z_c > z_l, or z_c == z_l and c < l}: the label l is in the top k exactly when beaten < k (for k = 1
 *     the tie rule of calm_top1_count: the lowest index wins);  pred = argmax, lowest index among equals;
 *     flags bit 0: the label is outside [0, C) — the row is SKIPPED: counted in `skipped` and in nothing else;
 *     flags bit 1: the row holds a NaN — the row is NON-FINITE: counted in `rows`, `nonfinite` and its class's support,
 *     never a hit, and it adds to neither the loss sum nor the confusion matrix.
 *   fold kernel (one workgroup): loss_sum[0] (double) += the fp32 sum, in a fixed order, of the nll of the counted finite
 *     rows;  counts (int64, 7 + 2 C values) += this batch's
 *       [0] rows   [1] skipped   [2] nonfinite   [3 + i] hits@ks[i], i < nk ([3 + nk .. 6] are left alone)
 *       [7 .. 7 + C) support[c] = #{counted rows with label c}     [7 + C .. 7 + 2 C) hits1[c] = #{of those, pred == c}
 *     confusion (nullable, int64 [C,C]): confusion[label * C + pred] += 1 for every counted finite row.
 * ks: HOST array of nk values, 1 <= nk <= 4, every k >= 1 (a k above C counts every finite counted row).
 * CALM_E_INVAL: a null logits / labels / ks / counts / loss_sum / partials, B <= 0, C <= 0, ld < C, nk outside 1 .. 4,
 * a k < 1, a storage type other than the two above;  CALM_E_UNSUPP: C > 65536;  CALM_E_LAYOUT: partials not 16-byte
 * aligned.  All of them before any launch.
 * ------------------------------------------------------------------------------------- */
int calm_eval_metrics(const void* logits, int64_t ld, int32_t logits_type, const int64_t* labels, const int32_t* ks,
                      int32_t nk, int64_t* counts, double* loss_sum, int64_t* confusion /* nullable */, int32_t B, int32_t C,
                      float* partials, void* stream);

/* ---------------------------------------------------------------------------------------
 * The generative job on row tokens (additions to ABI v7 — no existing signature or struct changes, so the version number
 * stays; csrc/recon.hip).  With the device collate the batch reaches the model as row tokens [B,S,3S], which ARE the
 * channels-last image: the Huber target has the layout of the model's output, and validation wants reconstruction
 * measures instead of class counts.  No atomics; cross-workgroup sums go through `partials` and are added in a fixed
 * order: results repeat bit for bit.
 *
 * calm_recon_huber_rows_fwd / _bwd: nn.HuberLoss(delta), mean over n elements, between two fp32 tensors of the same flat
 *   layout.  0 < n < 2^31 (CALM_E_INVAL / CALM_E_UNSUPP).  Both tensors (and dtokens) are accessed as 16-byte vectors when
 *   every base is 16-byte aligned, element by element otherwise; the last n % 4 elements always go one by one.  partials:
 *   calm_reduce_scratch_floats(CALM_RED_HUBER, ...) floats.  dloss is a DEVICE scalar (it carries GradScaler's scale).
 *
 * calm_recon_metrics: the reconstruction tallies of one batch, ADDED to the caller's device accumulator `double sums[8]`:
 *     [0] images counted
 *     [1] images holding a non-finite generated value; such an image adds to [0] and [1] and to nothing else
 *     [2] sum of Huber_delta(d) over elements, normalised space, d = generated - target
 *     [3] sum of |d|            [4] sum of d^2            [5] elements counted (3 S S per finite image)
 *     [6] sum over images of PSNR_b = 10 log10(1 / max(mse_b, 1e-10)), mse_b over the 3 S S pixel-space values of image b
 *     [7] sum over images of SSIM_b (left alone when want_ssim is 0)
 *   tokens [B,S,3S] (tokens[b,i,3j+c]), tokens_type CALM_ST_F32 or CALM_ST_BF16; target fp32, target_layout
 *   CALM_RECON_ROWS ([B,S,3S]) or CALM_RECON_NCHW ([B,3,S,S]).  Pixel space: p = clamp(v * std[c] + mean[c], 0, 1) on both
 *   tensors; mean / std are HOST arrays of three floats, read before the call returns.  SSIM (Wang et al. 2004) per channel
 *   in pixel space: 11 x 11 Gaussian window, sigma 1.5, weights normalised to sum 1, "valid" positions only ((S - 10)^2 per
 *   channel), C1 = 0.01^2, C2 = 0.03^2, population moments; SSIM_b is the mean over positions and channels.
 *   Launch 1: a workgroup owns a band of output rows of one image (and a strip of 246 output columns when S > 256); it
 *   writes one 32-byte record {huber, abs, sq, pixel sq, ssim, non-finite flag, 0, 0} into `partials`
 *   (calm_reduce_scratch_floats(CALM_RED_RECON, B, S) floats, 16-byte aligned).  Launch 2: one workgroup adds an image's
 *   records in double in record order and then the per-image values to `sums` in image order.
 *   CALM_E_INVAL: a null tokens / target / mean / std / sums / partials, B <= 0, S <= 0, an unknown storage type or
 *   layout;  CALM_E_UNSUPP: S < 11 with want_ssim, S > 4096, 2^31 workgroups or more;  CALM_E_LAYOUT: partials not
 *   16-byte aligned, tokens / target not aligned to their element.  All of them before any launch.
 * ------------------------------------------------------------------------------------- */
enum { CALM_RECON_ROWS = 0, CALM_RECON_NCHW = 1 };
int calm_recon_huber_rows_fwd(const float* tokens, const float* target, float delta, float* loss /* scalar, overwritten */,
                              int64_t n, float* partials, void* stream);
/* dtokens[e] = dloss / n * clamp(tokens[e] - target[e], -delta, delta) */
int calm_recon_huber_rows_bwd(const float* tokens, const float* target, float delta, const float* dloss, float* dtokens,
                              int64_t n, void* stream);
int calm_recon_metrics(const void* tokens, int32_t tokens_type, const float* target, int32_t target_layout,
                       const float* mean /* host [3] */, const float* std /* host [3] */, float delta, int32_t want_ssim,
                       double* sums /* device [8] */, int32_t B, int32_t S, float* partials, void* stream);

/* ---------------------------------------------------------------------------------------
 * Knowledge distillation (additions to ABI v7 — no existing signature or struct changes, so the version number stays):
 * the loss of a student trained against a frozen teacher's logits, cross-entropy with the CutMix / MixUp labels and the
 * distillation term in ONE pass per direction.  Per row b, with z the student logits (fp32, row stride ld), t the teacher
 * logits (teacher_type CALM_ST_F32 or CALM_ST_BF16, row stride tld; bf16 widens exactly), y the soft targets (fp32, row
 * stride td; they need not sum to one), T = temperature, a = alpha:
 *     p1 = softmax(z)      pT = softmax(z / T)      q = softmax(t / T)
 *     CE_b = sum_c y_c (max z - z_c) + log(sum exp(z - max z)) * sum_c y_c          (the form of calm_soft_ce_fwd)
 *     CALM_DISTILL_SOFT:  D_b = sum_c q_c (log q_c - log pT_c), a class with q_c == 0 adds 0 (F.kl_div);   w = a T^2
 *     CALM_DISTILL_HARD:  D_b = -log p1_k, k = argmax_c t_c (lowest index among equals); T is not used;    w = a
 *     loss = 1/B sum_b [(1 - a) CE_b + w D_b]
 *     soft: dlogits[b,c] = dloss/B [(1 - a)(p1_c sum_c y - y_c) + a T (pT_c - q_c)]
 *     hard: dlogits[b,c] = dloss/B [(1 - a)(p1_c sum_c y - y_c) + a (p1_c - [c == k])]
 * Every row maximum is subtracted before every exponential in both directions; pT and q come out of one expression
 * (exp((x - max x) * (1/T) - log sum exp((x - max x) * (1/T)))), so identical student and teacher rows give a distillation
 * gradient of exactly zero.  A NaN anywhere in a row (z, t or y; in hard mode as well) makes the loss NaN.  Rows are read
 * in groups of eight elements, each input as 16-byte vectors where its base is 16-byte aligned and its stride a multiple
 * of one vector (4 fp32 / 8 bf16 elements), element by element otherwise; dlogits likewise.  One workgroup per row; up
 * to C = 2048 a row of all three inputs stays in registers between the passes, beyond that it is read again (from cache).
 *
 * row_stats [B, CALM_DISTILL_ROW_STATS] fp32 — what the backward needs besides its inputs:
 *     [0] max_c z        [1] log sum exp(z - max z)        [2] log sum exp((z - max z) / T)
 *     [3] max_c t        [4] log sum exp((t - max t) / T)  [5] argmax_c t as a float (exact: C <= 65536)
 *     [6] sum_c y        [7] 0; NaN in hard mode when the teacher row holds a NaN (the argmax skips it: the backward
 *                            adds [7] to the row's gradient, so that a NaN loss comes with a NaN gradient)
 * partials: calm_reduce_scratch_floats(CALM_RED_DISTILL, B, C) floats, 16-byte aligned: five values per row (total, CE_b,
 *   D_b, agreement with y, agreement with t); one final workgroup adds them in a fixed order.  No atomics: results repeat
 *   bit for bit.
 * metrics (nullable): the float[4] of calm_soft_ce_fwd with its meaning — [0] += sum of the total row losses, [1] +=
 *   #{b : argmax z == argmax y} (a NaN in z or y: no agreement), [2] += B, [3] += 1.
 * dmetrics (nullable): device float[4]:  [0] += sum_b CE_b   [1] += sum_b D_b (unweighted)
 *   [2] += #{b : argmax z == argmax t} (ties to the lowest index; a NaN in z or t: no agreement)   [3] += B.
 *   Both are updated by one thread of the last launch with a plain read-modify-write.
 * CALM_E_INVAL: a null logits / teacher / targets / row_stats / loss (dloss, dlogits) / partials, B <= 0, C <= 0, a row
 * stride below C, T <= 0 or not finite, alpha outside [0, 1] or NaN, an unknown mode, a teacher storage type other than
 * the two above;  CALM_E_UNSUPP: C > 65536;  CALM_E_LAYOUT: partials not 16-byte aligned.  All of them before any launch.
 * ------------------------------------------------------------------------------------- */
enum { CALM_DISTILL_SOFT = 0, CALM_DISTILL_HARD = 1 };
#define CALM_DISTILL_ROW_STATS 8
int calm_distill_fwd(const float* logits, int64_t ld, const void* teacher, int64_t tld, int32_t teacher_type,
                     const float* targets, int64_t td, float temperature, float alpha, int32_t mode,
                     float* row_stats /* [B, CALM_DISTILL_ROW_STATS] */, float* loss /* scalar, overwritten */,
                     float* metrics /* nullable, [4] */, float* dmetrics /* nullable, [4] */, int32_t B, int32_t C,
                     float* partials, void* stream);
int calm_distill_bwd(const float* logits, int64_t ld, const void* teacher, int64_t tld, int32_t teacher_type,
                     const float* targets, int64_t td, float temperature, float alpha, int32_t mode,
                     const float* row_stats, const float* dloss /* device scalar */, float* dlogits /* [B,C] contiguous */,
                     int32_t B, int32_t C, void* stream);

/* ---------------------------------------------------------------------------------------
 * Binary cross-entropy with logits (additions to ABI v7 — no existing signature or struct changes, so the version number
 * stays): the loss the DeiT III / timm recipe trains with on the CutMix / MixUp soft targets, every class its own two-way
 * problem.  z the logits (fp32, row stride ld), y the soft targets (fp32, row stride td); rows are read as 16-byte vectors
 * where pointers and strides allow, element by element otherwise (and always for the last C % 4 classes).
 *     t = y;  with CALM_BCE_THRESHOLD  t = (y > threshold) ? 1 : 0            (timm's target_threshold: strict >)
 *     l(z, t) = max(z, 0) - z t + log(1 + exp(-|z|)),  evaluated as  |z| * (z >= 0 ? 1 - t : t) + log1p(exp(-|z|))
 *     loss = sum_{b,c} l / (B C)                 (torch.nn.BCEWithLogitsLoss(), the DeiT III form)
 *          = sum_{b,c} l / B                     with CALM_BCE_SUM_CLASSES (timm's sum_classes)
 *     dlogits[b,c] = dloss (sigmoid(z) - t) / (B C),  / B with CALM_BCE_SUM_CLASSES
 * The exponential never sees a positive argument, and for t in [0, 1] both terms of l are non-negative: nothing overflows
 * and nothing cancels.  Targets outside [0, 1] are legal, the formula is used as it is.  The sigmoid is the two-branch form
 * (1 / (1 + e) for z >= 0, e / (1 + e) otherwise, e = exp(-|z|)).  The backward needs nothing saved: it recomputes from
 * z and y.  dloss is a DEVICE scalar: it carries GradScaler's scale.  A NaN or infinite logit makes the loss non-finite
 * and its own dlogits element NaN (the other elements do not depend on it), so that the scaled optimizer step is skipped
 * as with the cross-entropy.
 * partials: calm_reduce_scratch_floats(CALM_RED_BCE, B, C) = 2 * B floats: one workgroup per row writes the row's sum and
 *   its agreement flag; the final workgroup of calm_soft_ce_fwd adds them in its fixed order.  No atomics: results repeat
 *   bit for bit.
 * metrics (nullable): the float[4] of calm_soft_ce_fwd with its meaning —
 *     [0] += B * loss (so that [0] / [2] is the mean of the printed loss under either reduction)
 *     [1] += #{b : argmax_c z[b,:] == argmax_c y[b,:]} — over the ORIGINAL y, not the thresholded one; ties go to the
 *            lowest index, a row holding a NaN in z or y counts as no agreement
 *     [2] += B        [3] += 1
 * CALM_E_INVAL: a null logits / targets / loss (dloss, dlogits) / partials, B <= 0, C <= 0, flag bits other than the two,
 * a threshold that is not finite with CALM_BCE_THRESHOLD set;  CALM_E_UNSUPP: B * C >= 2^31.  All of them before any launch.
 * ------------------------------------------------------------------------------------- */
enum { CALM_BCE_SUM_CLASSES = 1, CALM_BCE_THRESHOLD = 2 };   /* flags */
int calm_bce_fwd(const float* logits, int64_t ld, const float* targets, int64_t td, int32_t flags, float threshold,
                 float* loss /* scalar, overwritten */, float* metrics /* nullable, [4] */,
                 int32_t B, int32_t C, float* partials, void* stream);
int calm_bce_bwd(const float* logits, int64_t ld, const float* targets, int64_t td, int32_t flags, float threshold,
                 const float* dloss /* device scalar */, float* dlogits /* [B,C] contiguous */,
                 int32_t B, int32_t C, void* stream);

/* ---------------------------------------------------------------------------------------
 * Masked image modelling on row tokens (additions to ABI v7 — no existing signature or struct changes, so the version
 * number stays; csrc/mim.hip; SimMIM / MAE style pre-training of the generative job, no counterpart in the reference):
 * a per-sample patch mask with EXACTLY k set patches, the masked copy of a batch, and the Huber loss over the masked
 * elements alone.  Tokens are [B,S,3S] fp32, tokens[b, r, 3x + c] (the channels-last image).  Patch side p, S % p == 0,
 * G = S / p, P = G * G <= 1024; the patch of pixel (r, x) is i = (r / p) * G + x / p; mask is uint8 [B,P], 0 or 1.
 *
 * calm_mim_draw: mask[b, i] = rank(b, i) < k ? 1 : 0 with
 *     w(b, i)    = calm_dropout's word(e), e = (sample0 + b) * 1024 + i          (same generator, same key layout)
 *     rank(b, i) = #{ j < P : w(b, j) < w(b, i), or w(b, j) == w(b, i) and j < i }     (a permutation of 0 .. P - 1)
 *   so exactly k patches of every sample are set; k == 0 writes zeros, k == P ones.  The slot stride is 1024 whatever P is:
 *   the mask of a sample is a function of (seed, offset, sample0 + b, P, k) only — not of B, the grid, or of how a batch is
 *   split into calls.  key: DEVICE uint64[2] = (seed, offset), read by the kernel — no host synchronisation, valid inside a
 *   captured graph.  One workgroup per sample: the P words go to LDS, every thread ranks its patches against all of them
 *   (at most 2^20 compares per sample); no sort, no atomics.
 *   CALM_E_INVAL: null mask / key, B < 0, G < 1, k < 0, k > P, sample0 < 0, sample0 + B > 2^53;  CALM_E_UNSUPP: G > 32.
 *   B == 0 returns 0 without a launch.
 *
 * calm_mim_apply: y[b, r, 3x + c] = mask[b, i] ? fill[c] : x[b, r, 3x + c].  fill: HOST array of three floats (normalised
 *   space), read before the call returns.  A select: a NaN in a masked pixel of x does not reach y.  y may alias x (in
 *   place, unmasked elements are not touched).
 *   CALM_E_INVAL: null x / y / mask / fill, B < 0, S <= 0, p <= 0, S % p != 0;  CALM_E_UNSUPP: G > 32,
 *   3 * B * S * S >= 2^31;  CALM_E_LAYOUT: x or y not 4-byte aligned.  B == 0 returns 0 without a launch.
 *
 * calm_mim_huber_fwd / _bwd: with n = 3 * p * p * masked,
 *     loss       = 1/n * sum over the elements e with mask set of huber_delta(tokens[e] - target[e])
 *     dtokens[e] = mask ? dloss / n * clamp(tokens[e] - target[e], -delta, delta) : +0.0f       (EVERY element is written)
 *   masked: the number of set mask bytes in the batch — B * k behind calm_mim_draw, the caller's own count for a mask it
 *   made itself (the kernels do not count).  dloss is a DEVICE scalar (it carries GradScaler's scale).  Both select and
 *   never multiply: a NaN / inf at an unmasked position of tokens or target reaches neither the loss nor dtokens (a
 *   16-byte vector without a masked element is not even loaded); a non-finite value at a masked position propagates.
 *   partials: calm_reduce_scratch_floats(CALM_RED_MIM, B, S) floats, 16-byte aligned: one block sum per workgroup, added
 *   by one final workgroup in a fixed order.  No atomics: results repeat bit for bit.
 *   CALM_E_INVAL: a null pointer, B <= 0, S <= 0, p <= 0, S % p != 0, delta <= 0 or not finite, masked <= 0,
 *   masked > B * P;  CALM_E_UNSUPP: G > 32, 3 * B * S * S >= 2^31;  CALM_E_LAYOUT: partials not 16-byte aligned, a
 *   tensor not 4-byte aligned.
 *
 * The three streaming entry points move 16-byte vectors when every tensor base of the call is 16-byte aligned, single
 * elements otherwise (and always for the last 3 B S^2 % 4 elements).  The mask decision is per element either way: with
 * 3p % 4 != 0 a vector straddles a patch edge, with 3S % 4 != 0 a row end.  All refusals come before any launch.
 * ------------------------------------------------------------------------------------- */
int calm_mim_draw(uint8_t* mask /* [B,P] */, int64_t B, int32_t G, int32_t k, int64_t sample0,
                  const uint64_t* key /* device, [2] = seed, offset */, void* stream);
int calm_mim_apply(const float* x, float* y, const uint8_t* mask, const float* fill /* host [3] */, int32_t B, int32_t S,
                   int32_t p, void* stream);
int calm_mim_huber_fwd(const float* tokens, const float* target, const uint8_t* mask, float delta,
                       float* loss /* scalar, overwritten */, int32_t B, int32_t S, int32_t p, int64_t masked,
                       float* partials, void* stream);
int calm_mim_huber_bwd(const float* tokens, const float* target, const uint8_t* mask, float delta,
                       const float* dloss /* device scalar */, float* dtokens, int32_t B, int32_t S, int32_t p,
                       int64_t masked, void* stream);

/* ---------------------------------------------------------------------------------------
 * Weighted k-NN probe on frozen features (additions to ABI v7 — no existing signature or struct changes, so the version
 * number stays; csrc/knn.hip; the protocol of Wu et al. 2018 and DINO's eval_knn, no counterpart in the reference): rows
 * are L2-normalised, the k nearest bank items of every query are selected EXACTLY, chunk by chunk, and their labels vote
 * with weight exp(sim / T).  The similarities are calm_gemm's (queries [Nq,D] x a bank chunk [n,D]^T, fp32) in a scratch.
 * All three enqueue on `stream`, never synchronise, use no float atomics and repeat bit for bit.
 *
 * calm_knn_normalize: out[i, :] = x[i, :] / ||x[i, :]||.  x [N,D] fp32 or bf16 (x_type CALM_ST_F32 / CALM_ST_BF16), unit
 *   column stride, row stride ld elements; out fp32 [N,D] contiguous.  The squared norm is summed in fp32 in a fixed order
 *   (one wave per row).  A row that holds a non-finite element, or whose fp32 norm is 0 or not finite, becomes all +0.0f
 *   and the DEVICE counter bad[0] gains 1 (an integer add).  16-byte loads when x is 16-byte aligned and ld is a multiple
 *   of the elements in 16 bytes, element loads otherwise.
 *   CALM_E_INVAL: null x / out / bad, N < 0, D < 1, ld < D, an x_type other than the two;  CALM_E_UNSUPP: D > 4096;
 *   CALM_E_LAYOUT: x not aligned to its element, out not 4-byte aligned.  N == 0 returns 0 without a launch.
 *
 * calm_knn_merge: sims fp32 [Nq,n], unit column stride, row stride ld; element (q, j) is the similarity of query q to
 *   bank item base + j.  best_sim fp32 [Nq,k] and best_idx int64 [Nq,k] are the running state, read and rewritten: on
 *   return they hold the best k of (old state U this chunk), sorted, under the TOTAL order
 *       similarity descending, then bank index ascending.
 *   Values compare as floats (-0.0 == +0.0: the index decides; the stored bits are the element's own); a NaN similarity
 *   ranks, and is stored, as -inf.  An empty slot is (-inf, -1): it ranks below every real entry, a real -inf included.
 *   The caller resets the state by filling it with empty slots, and gives every bank item to the state once.  Because
 *   the order is total, the state after any chunking of the bank, in any order of the chunks, is the same bit for bit.
 *   One workgroup per query: a compare pass against the state's k-th entry (a row without a candidate writes nothing),
 *   an 8-bit radix select over the candidates' keys when they do not fit the LDS, a bitonic sort of at most 1024 entries.
 *   CALM_E_INVAL: null sims / best_sim / best_idx, k < 1, n < 1, Nq < 0, ld < n, base < 0, base + n > 2^63 - 1;
 *   CALM_E_UNSUPP: k > 256, Nq >= 2^31;  CALM_E_LAYOUT: a tensor not aligned to its element.  Nq == 0 returns 0
 *   without a launch.
 *
 * calm_knn_vote: scores fp32 [Nq,C], row stride ld, every element overwritten:
 *       scores[q, c] = sum over the slots j, ascending, with best_idx[q, j] in [0, Nb) and bank_labels[best_idx[q, j]] == c
 *                      of exp((best_sim[q, j] - best_sim[q, 0]) * inv_T)
 *   (the difference of two equal values is taken as 0, also of two -inf).  Subtracting the row's largest similarity
 *   changes no ranking and keeps every weight in (0, 1].  A label outside [0, C) votes for nothing; a class without a
 *   neighbour gets exactly +0.0f; two classes with bit-equal votes get bit-equal scores.  bank_labels int64 [Nb].
 *   CALM_E_INVAL: null best_sim / best_idx / bank_labels / scores, k < 1, C < 1, Nq < 0, Nb < 0, ld < C, inv_T <= 0 or
 *   not finite;  CALM_E_UNSUPP: k > 256, Nq >= 2^31;  CALM_E_LAYOUT: a tensor not aligned to its element.  Nq == 0
 *   returns 0 without a launch.
 * All refusals come before any launch.
 * ------------------------------------------------------------------------------------- */
int calm_knn_normalize(const void* x, int64_t ld, int32_t x_type, float* out /* [N,D] */, int64_t* bad /* device, [1] */,
                       int64_t N, int32_t D, void* stream);
int calm_knn_merge(const float* sims, int64_t ld, int64_t base, float* best_sim /* [Nq,k] */, int64_t* best_idx /* [Nq,k] */,
                   int64_t Nq, int32_t n, int32_t k, void* stream);
int calm_knn_vote(const float* best_sim, const int64_t* best_idx, const int64_t* bank_labels /* [Nb] */, int64_t Nb,
                  float inv_T, float* scores /* [Nq,C] */, int64_t ld, int64_t Nq, int32_t k, int32_t C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CALM_VIT_H */
