"""ctypes binding of libcalmvit_hip.so (the C-ABI declared in include/calm_vit.h).

There is NO fallback: if the shared object is missing or a symbol cannot be resolved, loading
raises and every op of the package fails loudly.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# CALM_VIT_LIB: A/B another build of the same library (kernel tuning); never a different implementation
LIB_PATH = os.environ.get("CALM_VIT_LIB") or os.path.join(HERE, "libcalmvit_hip.so")

ACT_NONE, ACT_GELU, ACT_GELU_BWD = 0, 1, 2
F32 = 0
ST_F32, ST_BF16, ST_FP8_E4M3, ST_FP8_E5M2 = 0, 1, 2, 3   # storage type of a tensor in HBM (CALM_ST_*)
E_INVAL, E_LAYOUT, E_UNSUPP = -1, -2, -3      # CALM_E_*
ABI_VERSION = 7          # CALM_ABI_VERSION of include/calm_vit.h

_p = C.c_void_p
_i32 = C.c_int32
_i64 = C.c_int64
_f32 = C.c_float


class GemmArgs(C.Structure):
    """struct calm_gemm_args (include/calm_vit.h)."""
    _fields_ = [
        ("A", _p), ("B", _p), ("C", _p),
        ("M", _i32), ("N", _i32), ("K", _i32),
        ("batch0", _i32), ("batch1", _i32),
        ("a_rs", _i64), ("a_cs", _i64), ("a_b0", _i64), ("a_b1", _i64),
        ("b_rs", _i64), ("b_cs", _i64), ("b_b0", _i64), ("b_b1", _i64),
        ("c_rs", _i64), ("c_b0", _i64), ("c_b1", _i64),
        ("alpha", _f32),
        ("inv_scale", _p), ("bias", _p), ("col_scale", _p),
        ("residual", _p), ("r_rs", _i64), ("r_b0", _i64), ("r_b1", _i64),
        ("C_pre", _p), ("aux", _p),
        ("act", _i32), ("accumulate", _i32), ("reduce_batch", _i32), ("split_k", _i32), ("dtype", _i32),
        ("n_group", _i32),
        ("A_group", _p * 4), ("B_group", _p * 4), ("C_group", _p * 4), ("inv_scale_group", _p * 4),
        ("workspace", _p), ("workspace_bytes", _i64),
        ("a_type", _i32), ("b_type", _i32), ("c_type", _i32), ("aux_type", _i32), ("r_type", _i32), ("reserved_", _i32),
        ("a_dq", _p), ("b_dq", _p),
    ]


class GemmPlan(C.Structure):
    """struct calm_gemm_plan (calm_gemm_describe, ABI v7)."""
    _fields_ = [(n, _i32) for n in ("family", "tile_m", "tile_n", "tile_k", "tiles_m", "tiles_n", "k_slices", "items",
                                    "grid", "epi_unit", "uses_workspace", "threads")]


RED_LAYERNORM_BWD, RED_ROPE_BWD, RED_LATENT_FWD, RED_COLSUM, RED_CNN_BWD = range(5)     # CALM_RED_*
RED_SOFT_CE, RED_HUBER = 5, 6                      # the loss entry points (csrc/loss.hip)
RED_EVAL = 7                                       # calm_eval_metrics: one 16-byte record per row
RED_RECON = 8                                      # calm_recon_metrics: one 32-byte record per workgroup
RED_DISTILL = 9                                    # calm_distill_fwd: five sums per row
RED_BCE = 10                                       # calm_bce_fwd: row sums and agreement flags
RED_MIM = 11                                       # calm_mim_huber_fwd: one block sum per workgroup
BCE_SUM_CLASSES, BCE_THRESHOLD = 1, 2              # calm_bce_*'s flags (CALM_BCE_*)
DISTILL_SOFT, DISTILL_HARD = 0, 1                  # calm_distill_*'s mode (CALM_DISTILL_*)
DISTILL_ROW_STATS = 8                              # CALM_DISTILL_ROW_STATS: floats per row of calm_distill_*'s row_stats
RECON_ROWS, RECON_NCHW = 0, 1                      # calm_recon_metrics' target_layout (CALM_RECON_*)
EVAL_COUNTS_HEAD = 7                               # counts: rows, skipped, nonfinite, hits@k[0..3], then support[C], hits1[C]


class ReduceShape(C.Structure):
    """struct calm_reduce_shape (48 bytes): the rows of partials a calm_part_* entry point wrote."""
    _fields_ = [("G", _i32), ("n", _i32), ("stride", _i32), ("nseg", _i32), ("begin", _i32 * 7), ("reserved", _i32)]


class ReduceEntry(C.Structure):
    """struct calm_reduce_entry (104 bytes, one per reduction of calm_reduce_partials_batch)."""
    _fields_ = [("partials", _p), ("G", _i32), ("n", _i32), ("stride", _i32), ("nseg", _i32), ("out", _p * 6),
                ("begin", _i32 * 7), ("reserved", _i32)]


class SnBwdEntry(C.Structure):
    """struct calm_sn_bwd_entry (80 bytes, one per layer of calm_sn_weight_bwd_batch)."""
    _fields_ = [("G", _p), ("w_orig", _p), ("u", _p), ("v", _p), ("sigma", _p), ("ls", _p), ("d_w_orig", _p), ("d_ls", _p),
                ("rowdot", _p), ("rows", _i32), ("cols", _i32)]


class OptimTensor(C.Structure):
    """struct calm_optim_tensor (80 bytes); `group`: the parameter group calm_optim_step_groups reads."""
    _fields_ = [("param", _p), ("grad", _p), ("exp_avg", _p), ("exp_avg_sq", _p), ("sn_u", _p), ("sn_v", _p),
                ("sn_sigma", _p), ("numel", _i64), ("rows", _i32), ("cols", _i32), ("chunk0", _i32), ("group", _i32)]


class OptimGroup(C.Structure):
    """struct calm_optim_group (8 bytes, one per parameter group of calm_optim_step_groups)."""
    _fields_ = [("lr", _f32), ("weight_decay", _f32)]


class OptimHparams(C.Structure):
    """struct calm_optim_hparams."""
    _fields_ = [("lr", _f32), ("beta1", _f32), ("beta2", _f32), ("eps", _f32), ("weight_decay", _f32),
                ("max_norm", _f32), ("step", _i32)]


class LambHparams(C.Structure):
    """struct calm_lamb_hparams (8 bytes)."""
    _fields_ = [("trust_clip", _f32), ("always_adapt", _i32)]


class GradStat(C.Structure):
    """struct calm_grad_stat (32 bytes, one per tensor of calm_grad_stats; np.dtype(GradStat) is the numpy record)."""
    _fields_ = [("grad_sq", _f32), ("grad_absmax", _f32), ("param_sq", _f32), ("param_absmax", _f32), ("dir_sq", _f32),
                ("nonfinite", _i32), ("bad_calls", _i32), ("first_bad_call", _i32)]


class SamHparams(C.Structure):
    """struct calm_sam_hparams (16 bytes)."""
    _fields_ = [("rho", _f32), ("eps", _f32), ("eta", _f32), ("adaptive", _i32)]


class CastEntry(C.Structure):
    """struct calm_cast_entry."""
    _fields_ = [("src", _p), ("dst", _p), ("numel", _i64), ("chunk0", _i32), ("reserved", _i32)]


EMA_CONSTANT, EMA_WARMUP = 0, 1                   # calm_ema_update's schedule (CALM_EMA_*)


class EmaEntry(C.Structure):
    """struct calm_ema_entry (32 bytes)."""
    _fields_ = [("src", _p), ("ema", _p), ("numel", _i64), ("chunk0", _i32), ("reserved", _i32)]


class SnapshotEntry(C.Structure):
    """struct calm_snapshot_entry (32 bytes)."""
    _fields_ = [("tensor", _p), ("offset", _i64), ("nbytes", _i64), ("chunk0", _i32), ("reserved", _i32)]


class SnLayer(C.Structure):
    """struct calm_sn_layer."""
    _fields_ = [("w", _p), ("u", _p), ("v", _p), ("sigma", _p), ("rows", _i32), ("cols", _i32)]


class SnPlanInfo(C.Structure):
    """struct calm_sn_plan_info."""
    _fields_ = [("blob_bytes", _i64), ("scratch_floats", _i64), ("n_layers", _i32), ("n_work", _i32),
                ("n_work_a", _i32), ("reserved", _i32)]


AUG_FLIP, AUG_SOLARIZE, AUG_GRAYSCALE, AUG_BLUR = 1, 2, 4, 8                       # calm_aug_sample.flags (CALM_AUG_*)
AUG_OP_BRIGHTNESS, AUG_OP_CONTRAST, AUG_OP_SATURATION, AUG_OP_HUE, AUG_OP_NONE = 0, 1, 2, 3, 255


class AugSample(C.Structure):
    """struct calm_aug_sample (48 bytes, one per sample of calm_augment_collate)."""
    _fields_ = [("y0", _i32), ("x0", _i32), ("flags", C.c_uint32), ("order", C.c_uint8 * 4),
                ("brightness", _f32), ("contrast", _f32), ("saturation", _f32), ("hue", _f32),
                ("solarize_thr", _f32), ("blur_sigma", _f32), ("reserved", _f32 * 2)]


class EraseBox(C.Structure):
    """struct calm_erase_box (16 bytes, one per sample of calm_augment_collate_erase): a box in output coordinates."""
    _fields_ = [("y", _i32), ("x", _i32), ("h", _i32), ("w", _i32)]


class ResizeSample(C.Structure):
    """struct calm_resize_sample (16 bytes, one per image of calm_resize_u8)."""
    _fields_ = [("offset", _i64), ("h", _i32), ("w", _i32)]


RCROP_U8, RCROP_IMAGE, RCROP_TOKENS = 0, 1, 2                                      # calm_resized_crop's out_kind


class RCropSample(C.Structure):
    """struct calm_rcrop_sample (48 bytes, one per image of calm_resized_crop)."""
    _fields_ = [("offset", _i64), ("h", _i32), ("w", _i32), ("by0", _i32), ("bx0", _i32), ("bh", _i32), ("bw", _i32),
                ("vh", _i32), ("vw", _i32), ("wy0", _i32), ("wx0", _i32)]


RA_MAX_OPS, RA_MAX_SIDE = 4, 4096                                                  # CALM_RA_MAX_OPS, CALM_RA_MAX_SIDE
(RA_OP_IDENTITY, RA_OP_AFFINE, RA_OP_BRIGHTNESS, RA_OP_COLOR, RA_OP_CONTRAST, RA_OP_SHARPNESS, RA_OP_POSTERIZE,
 RA_OP_SOLARIZE, RA_OP_AUTOCONTRAST, RA_OP_EQUALIZE) = range(10)                    # CALM_RA_OP_*
RA_STATS_OPS = (RA_OP_CONTRAST, RA_OP_AUTOCONTRAST, RA_OP_EQUALIZE)                 # the slots a statistics launch precedes


class RaSample(C.Structure):
    """struct calm_ra_sample (160 bytes, one per sample of calm_randaugment_u8)."""
    _fields_ = [("y0", _i32), ("x0", _i32), ("flip", C.c_uint32), ("n_ops", _i32), ("op", _i32 * 4), ("factor", _f32 * 4),
                ("param", _i32 * 4), ("coef", (_i32 * 6) * 4)]


# name -> (restype, argtypes); every symbol include/calm_vit.h declares
SIGNATURES = {
    "calm_abi_version": (_i32, []),
    "calm_build_info": (C.c_char_p, []),
    "calm_gemm": (_i32, [C.POINTER(GemmArgs), _p]),
    "calm_gemm_workspace_bytes": (_i64, [C.POINTER(GemmArgs)]),
    "calm_gemm_set_option": (C.c_int, [_i32, _i32]),
    "calm_gemm_describe": (_i32, [C.POINTER(GemmArgs), C.POINTER(GemmPlan)]),
    "calm_gemm_lane": (_i32, [C.POINTER(GemmArgs), _p]),
    "calm_gemm_lane_fork": (_i32, [_p]),
    "calm_gemm_lane_join": (_i32, [_p]),
    "calm_gemm_lane_stats": (_i32, [C.POINTER(_i64 * 4)]),
    "calm_reduce_scratch_floats": (_i64, [_i32, _i64, _i32]),
    "calm_reduce_batch_max": (_i32, []),
    "calm_reduce_partials_batch": (_i32, [C.POINTER(ReduceEntry), _i32, _p]),
    "calm_part_layernorm_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _i64, _i32, _i32, _p, C.POINTER(ReduceShape), _p]),
    "calm_part_rope_bwd": (_i32, [_p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p,
                                  C.POINTER(ReduceShape), _p]),
    "calm_part_colsum": (_i32, [_p, _i64, _i32, _i32, _p, C.POINTER(ReduceShape), _p]),
    "calm_part_cnn_residual_bwd": (_i32, [_p] * 12 + [_i32, _i32, _i32, _i32, _p, C.POINTER(ReduceShape), _p]),
    "calm_sn_bwd_batch_max": (_i32, []),
    "calm_sn_weight_bwd_batch": (_i32, [C.POINTER(SnBwdEntry), _i32, _p]),
    "calm_layernorm_fwd": (_i32, [_p, _p, _p, _p, _p, _i64, _i32, _f32, _i32, _p]),
    "calm_layernorm_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i32, _i32, _p, _p]),
    "calm_cast_chunk_elems": (_i32, []),
    "calm_cast_bf16": (_i32, [_p, _p, _i32, _p]),
    "calm_cast_bf16_one": (_i32, [_p, _p, _i64, _p]),
    "calm_cast_f32_one": (_i32, [_p, _p, _i64, _p]),
    "calm_quantize_fp8": (_i32, [_p, _i32, _i64, _p, _i32, _p, _p]),
    "calm_transpose_u8": (_i32, [_p, _p, _i32, _i32, _p]),
    "calm_rope_fwd": (_i32, [_p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "calm_rope_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p]),
    "calm_softmax_fwd": (_i32, [_p, _i64, _i32, _p]),
    "calm_softmax_bwd": (_i32, [_p, _p, _i64, _i32, _p]),
    "calm_softmax_bwd_heads": (_i32, [_p, _p, _p, _i32, _i32, _i32, _i32, _p]),
    "calm_sum_heads": (_i32, [_p, _p, _i32, _i32, _i64, _p]),
    "calm_attention_fwd_supported": (_i32, [_i32, _i32, _i32, _i32]),
    "calm_attention_fwd": (_i32, [_p] * 15 + [_i32] * 5 + [_p]),
    "calm_attention_bwd_preferred": (_i32, [_i32, _i32, _i32, _i32]),
    "calm_attention_bwd": (_i32, [_p] * 10 + [_i32] * 5 + [_p]),
    "calm_attention_bwd_front": (_i32, [_p] * 5 + [_i32] * 5 + [_p]),
    "calm_attention_bwd_back": (_i32, [_p] * 9 + [_i32] * 5 + [_p]),
    "calm_attention_bwd_fold_preferred": (_i32, [_i32, _i32, _i32, _i32]),
    "calm_attention_set_option": (C.c_int, [_i32, _i32]),
    "calm_attention_fwd_lse": (_i32, [_p] * 15 + [_i32] * 5 + [_p]),
    "calm_attention_bwd_lse_scratch_bytes": (_i64, [_i32] * 5),
    "calm_attention_bwd_lse": (_i32, [_p] * 7 + [_i64] + [_p] * 4 + [_i32] * 5 + [_p]),
    "calm_attention_infer": (_i32, [_p] * 11 + [_i32] * 5 + [_p]),
    "calm_attention16_supported": (_i32, [_i32, _i32, _i32]),
    "calm_attention16_fwd": (_i32, [_p] * 16 + [_i32] * 4 + [_p]),
    "calm_attention16_bwd": (_i32, [_p] * 13 + [_i32] * 4 + [_p]),
    "calm_attention16_infer": (_i32, [_p] * 11 + [_i32] * 4 + [_p]),
    "calm_latent_fwd": (_i32, [_p, _p, _p, _p, _p, _i64, _i32, _p, _p]),
    "calm_latent_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _i64, _i32, _p]),
    "calm_sn_plan": (_i32, [C.POINTER(SnLayer), _i32, _p, C.POINTER(SnPlanInfo)]),
    "calm_sn_power_iter": (_i32, [_p, C.POINTER(SnPlanInfo), _i32, _f32, _p, _p]),
    "calm_sn_weight_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _p, _p]),
    "calm_optim_chunk_elems": (_i32, []),
    "calm_optim_step": (_i32, [_p, _i32, _p, _i32, _p, C.POINTER(OptimHparams), _p, _p, _p, _p, _p]),
    "calm_optim_step_groups": (_i32, [_p, _i32, _p, _i32, _p, C.POINTER(OptimHparams), _p, _i32, _p, _p, _p, _p]),
    "calm_optim_lamb_scratch_floats": (_i64, [_i32, _i32]),
    "calm_optim_step_lamb": (_i32, [_p, _i32, _p, _i32, _p, C.POINTER(OptimHparams), C.POINTER(LambHparams), _p, _i32, _p, _p,
                                    _p, _p, _p, _p]),
    "calm_grad_accum": (_i32, [_p, _i32, _p, _i32, _p, _p, _i32, _p]),
    "calm_grad_stats_scratch_floats": (_i64, [_i32, _i32]),
    "calm_grad_stats": (_i32, [_p, _i32, _p, _i32, C.POINTER(OptimHparams), _p, _p, _p, _p, _p, _p]),
    "calm_sam_scratch_floats": (_i64, [_i32, _i32]),
    "calm_sam_perturb": (_i32, [_p, _i32, _p, _i32, C.POINTER(SamHparams), _p, _p, _p, _p, _p]),
    "calm_sam_restore": (_i32, [_p, _i32, _p, _i32, _p, _p]),
    "calm_ema_chunk_elems": (_i32, []),
    "calm_ema_update": (_i32, [_p, _i32, _p, _i32, _f32, _i32, _p, _p, _p, _p]),
    "calm_ema_swap": (_i32, [_p, _i32, _p, _i32, _p]),
    "calm_snapshot_chunk_bytes": (_i32, []),
    "calm_snapshot_pack": (_i32, [_p, _i32, _p, _i32, _p, _i64, _p]),
    "calm_snapshot_unpack": (_i32, [_p, _i32, _p, _i32, _p, _i64, _p]),
    "calm_collate_mix": (_i32, [_p, _p, _p, _i32, _i32, _i32, _i32, _f32, _p, _p, _p, _p]),
    "calm_collate_crop_mix": (_i32, [_p, _i32, _i32, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _f32, _p, _p, _p, _p]),
    "calm_augment_collate": (_i32, [_p, _i32, _i32, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _f32, _p, _p, _p, _p]),
    "calm_augment_collate_erase": (_i32, [_p, _i32, _i32, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _f32, _p, _p, _p, _p, _i32, _p,
                                          C.c_uint64, C.c_uint64, _p]),
    "calm_resize_coeffs": (_i32, [_i32, _i32, _p, _p, _i32]),
    "calm_resize_u8": (_i32, [_p, _i64, _p, _p, _i32, _i32, _i32, _p]),
    "calm_resized_crop": (_i32, [_p, _i64, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _p]),
    "calm_resized_crop_check": (_i32, [C.POINTER(RCropSample), _i64, _i32, _i32]),
    "calm_randaugment_scratch_bytes": (_i64, [_i32, _i32, _i32]),
    "calm_randaugment_u8": (_i32, [_p, _i32, _i32, _p, _p, _i32, _i32, _i32, _i32, C.c_uint32, _p, _p, _i64, _p]),
    "calm_image_to_rows": (_i32, [_p, _p, _i32, _i32, _p]),
    "calm_rows_to_image": (_i32, [_p, _p, _i32, _i32, _p]),
    "calm_grid_transpose": (_i32, [_p, _p, _i32, _i32, _p]),
    "calm_dwconv3x3_fwd": (_i32, [_p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _p]),
    "calm_dwconv3x3_bwd": (_i32, [_p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _p]),
    "calm_cnn_residual_fwd": (_i32, [_p] * 11 + [_i32, _i32, _i32, _i32, _p]),
    "calm_cnn_residual_bwd": (_i32, [_p] * 18 + [_i32, _i32, _i32, _i32, _p, _p]),
    "calm_add": (_i32, [_p, _p, _p, _i64, _p]),
    "calm_gelu_fwd": (_i32, [_p, _p, _i64, _p]),
    "calm_gelu_bwd": (_i32, [_p, _p, _p, _i64, _p]),
    "calm_colsum": (_i32, [_p, _p, _i64, _i32, _i32, _p, _p]),
    "calm_row_scale": (_i32, [_p, _p, _p, _i32, _i32, _i32, _p]),
    "calm_mean_seq_fwd": (_i32, [_p, _p, _i32, _i32, _i32, _p]),
    "calm_mean_seq_bwd": (_i32, [_p, _p, _i32, _i32, _i32, _p]),
    "calm_soft_ce_fwd": (_i32, [_p, _i64, _p, _i64, _p, _p, _p, _i32, _i32, _p, _p]),
    "calm_soft_ce_bwd": (_i32, [_p, _i64, _p, _i64, _p, _p, _p, _i32, _i32, _p]),
    "calm_huber_tokens_fwd": (_i32, [_p, _p, _f32, _p, _i32, _i32, _p, _p]),
    "calm_huber_tokens_bwd": (_i32, [_p, _p, _f32, _p, _p, _i32, _i32, _p]),
    "calm_top1_count": (_i32, [_p, _i64, _p, _p, _i32, _i32, _p]),
    "calm_eval_metrics": (_i32, [_p, _i64, _i32, _p, C.POINTER(_i32), _i32, _p, _p, _p, _i32, _i32, _p, _p]),
    "calm_recon_huber_rows_fwd": (_i32, [_p, _p, _f32, _p, _i64, _p, _p]),
    "calm_recon_huber_rows_bwd": (_i32, [_p, _p, _f32, _p, _p, _i64, _p]),
    "calm_recon_metrics": (_i32, [_p, _i32, _p, _i32, C.POINTER(_f32), C.POINTER(_f32), _f32, _i32, _p, _i32, _i32, _p, _p]),
    "calm_distill_fwd": (_i32, [_p, _i64, _p, _i64, _i32, _p, _i64, _f32, _f32, _i32, _p, _p, _p, _p, _i32, _i32, _p, _p]),
    "calm_distill_bwd": (_i32, [_p, _i64, _p, _i64, _i32, _p, _i64, _f32, _f32, _i32, _p, _p, _p, _i32, _i32, _p]),
    "calm_bce_fwd": (_i32, [_p, _i64, _p, _i64, _i32, _f32, _p, _p, _i32, _i32, _p, _p]),
    "calm_bce_bwd": (_i32, [_p, _i64, _p, _i64, _i32, _f32, _p, _p, _i32, _i32, _p]),
    "calm_dropout": (_i32, [_p, _p, _p, _i64, _i64, _f32, _p, _i32, _i32, _i32, _p]),
    "calm_drop_path": (_i32, [_p, _p, _p, _i64, _i64, _i64, _f32, _p, _i32, _i32, _i32, _p]),
    "calm_mim_draw": (_i32, [_p, _i64, _i32, _i32, _i64, _p, _p]),
    "calm_mim_apply": (_i32, [_p, _p, _p, C.POINTER(_f32), _i32, _i32, _i32, _p]),
    "calm_mim_huber_fwd": (_i32, [_p, _p, _p, _f32, _p, _i32, _i32, _i32, _i64, _p, _p]),
    "calm_mim_huber_bwd": (_i32, [_p, _p, _p, _f32, _p, _p, _i32, _i32, _i32, _i64, _p]),
    "calm_knn_normalize": (_i32, [_p, _i64, _i32, _p, _p, _i64, _i32, _p]),
    "calm_knn_merge": (_i32, [_p, _i64, _i64, _p, _p, _i64, _i32, _i32, _p]),
    "calm_knn_vote": (_i32, [_p, _p, _p, _i64, _f32, _p, _i64, _i64, _i32, _i32, _p]),
}

_lib = None


def load():
    """dlopen the library once and type every entry point.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  The CALM-ViT path has no non-HIP fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.calm_abi_version() != ABI_VERSION:
        raise RuntimeError("libcalmvit_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        kind = "invalid argument/unsupported shape" if rc < 0 else "hipError_t"
        raise RuntimeError(f"{what} failed: code {rc} ({kind})")
