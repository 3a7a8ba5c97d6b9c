"""The drop-in boundary without a GPU: libcalmvit_hip.so builds / loads on a CPU-only host, exports every entry point
include/calm_vit.h declares, the ctypes binding (calm-vit-dte_amd/_lib.py) names exactly those entry points, and the ABI
version of the library is the header's.  No compute entry point is called here."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "calm_vit.h")
LIB = os.path.join(ROOT, "calm-vit-dte_amd", "libcalmvit_hip.so")


def _declared():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(calm_\w+)\s*\(", text, flags=re.M)))


def _library():
    if not os.path.exists(LIB):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(LIB)


def test_header_declares_the_path_entry_points():
    names = _declared()
    for must in ("calm_gemm", "calm_attention_fwd", "calm_attention_bwd", "calm_layernorm_fwd", "calm_layernorm_bwd",
                 "calm_rope_fwd", "calm_sn_power_iter", "calm_cnn_residual_fwd", "calm_cnn_residual_bwd",
                 "calm_optim_step", "calm_collate_mix", "calm_abi_version"):
        assert must in names, must
    assert len(names) >= 35


def test_library_exports_every_declared_symbol_and_binding_matches():
    lib = _library()
    names = _declared()
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    sys.path.insert(0, ROOT)
    from importlib import import_module
    binding = import_module("calm_vit_dte_amd._lib")
    assert sorted(binding.SIGNATURES) == names          # the Python side binds exactly the declared C-ABI
    version = int(re.search(r"#define\s+CALM_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    lib.calm_abi_version.restype = ctypes.c_int
    assert lib.calm_abi_version() == version
    lib.calm_build_info.restype = ctypes.c_char_p
    assert b"gfx950" in lib.calm_build_info()


def test_struct_layouts_match_the_header():
    """sizeof of the by-pointer structs as the C compiler lays them out vs the ctypes mirrors."""
    import subprocess
    import tempfile
    sys.path.insert(0, ROOT)
    from importlib import import_module
    binding = import_module("calm_vit_dte_amd._lib")
    src = '#include <stdio.h>\n#include "calm_vit.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(calm_gemm_args), ' \
          'sizeof(calm_sn_layer), sizeof(calm_sn_plan_info), sizeof(calm_optim_tensor), sizeof(calm_optim_hparams), ' \
          'sizeof(calm_gemm_plan));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        sizes = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    mirrors = [binding.GemmArgs, binding.SnLayer, binding.SnPlanInfo, binding.OptimTensor, binding.OptimHparams, binding.GemmPlan]
    assert sizes == [ctypes.sizeof(m) for m in mirrors]


def test_host_side_planning_entry_points_answer_without_a_gpu():
    """The planning half of the C-ABI is host code (no launch, no device query): the scratch a reduction entry point
    needs (calm_reduce_scratch_floats, ABI v7) and what a calm_gemm launch decomposes into (calm_gemm_describe).  The
    pointers handed to describe are never dereferenced."""
    sys.path.insert(0, ROOT)
    from importlib import import_module
    binding = import_module("calm_vit_dte_amd._lib")
    lib = binding.load()
    for op in (binding.RED_LAYERNORM_BWD, binding.RED_ROPE_BWD, binding.RED_LATENT_FWD, binding.RED_COLSUM, binding.RED_CNN_BWD):
        for rows, cols in ((1, 4), (57344, 672), (20480, 240), (3, 1344)):
            need = int(lib.calm_reduce_scratch_floats(op, rows, cols))
            assert 0 < need <= (1 << 22), (op, rows, cols, need)          # a few MB at most: the backend keeps 4 MB per stream
    assert int(lib.calm_reduce_scratch_floats(99, 10, 10)) == 0
    g = binding.GemmArgs()
    M, N, K = 57344, 1344, 672                                  # the bench's MLP forward on bf16 tensors
    g.A, g.B, g.C = 0x10000, 0x20000, 0x30000
    g.M, g.N, g.K = M, N, K
    g.a_rs, g.a_cs, g.b_rs, g.b_cs, g.c_rs = K, 1, K, 1, N
    g.batch0 = g.batch1 = 1
    g.alpha = 1.0
    g.dtype = 1
    g.a_type = g.b_type = g.c_type = binding.ST_BF16
    g.split_k = 1
    plan = binding.GemmPlan()
    assert lib.calm_gemm_describe(ctypes.byref(g), ctypes.byref(plan)) == 0
    assert plan.family == 3 and plan.tile_k == 64 and plan.grid == 256 and plan.threads == 512
    assert plan.tiles_m * plan.tile_m >= M and plan.tiles_n * plan.tile_n >= N and plan.items == plan.tiles_m * plan.tiles_n
    g.dtype, g.a_type, g.b_type, g.c_type = 0, 0, 0, 0          # the same product on fp32 tensors: 128-row tiles
    assert lib.calm_gemm_describe(ctypes.byref(g), ctypes.byref(plan)) == 0
    assert plan.family == 0 and plan.tile_m == 128 and plan.tile_n in (96, 128)


def test_gemm_workspace_bytes_and_describe_report_one_plan():
    """calm_gemm_workspace_bytes and calm_gemm_describe read the same plan as the launch.  Over a seeded sweep of argument
    sets (every option setting, operand layout and storage type, batches, groups, batch-reduced and k-split launches,
    epilogue operands): an error asks for no workspace; the workspace is whole fp32 partial tiles and is asked for only
    in deterministic mode or from CALM_GEMM_WS_MIN_SLICES (48) k-slices per output; describe uses exactly the bytes asked
    for (not 4 fewer); the persistent families launch min(items, 256) workgroups, the others one per item."""
    import random
    sys.path.insert(0, ROOT)
    from importlib import import_module
    binding = import_module("calm_vit_dte_amd._lib")
    lib = binding.load()
    rng = random.Random(1234)
    sizes = (57344, 20480, 1344, 672, 528, 480, 384, 240, 224, 176, 80, 1, 3, 100, 1000)
    types = ((0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0), (1, 1, 1, 0), (1, 1, 1, 1), (1, 2, 2, 1), (1, 3, 2, 0))
    addr = iter(range(1 << 32, 1 << 56, 1 << 20))                  # fake device addresses: describe never reads them
    ptr = lambda: next(addr) + (4 if rng.random() < 0.03 else 0)  # noqa: E731
    opt_pipe, opt_pipe32, opt_det = 0, 1, 2                         # CALM_GEMM_OPT_*
    saved = [lib.calm_gemm_set_option(o, 0) for o in (opt_pipe, opt_pipe32, opt_det)]
    families, with_ws = set(), 0
    try:
        for _ in range(4000):
            det = rng.randint(0, 1)
            for o, v in ((opt_pipe, rng.randint(0, 1)), (opt_pipe32, rng.randint(0, 2)), (opt_det, det)):
                lib.calm_gemm_set_option(o, v)
            g = binding.GemmArgs()
            M, N, K = g.M, g.N, g.K = [rng.choice(sizes) for _ in range(3)]
            g.dtype, g.a_type, g.b_type, g.c_type = rng.choice(types)
            g.A, g.B, g.C, g.a_dq, g.b_dq = ptr(), ptr(), ptr(), ptr(), ptr()
            g.a_rs, g.a_cs = (K, 1) if rng.random() < 0.6 else (1, M)
            g.b_rs, g.b_cs = (K, 1) if rng.random() < 0.6 else (1, N)
            g.c_rs = N
            g.batch0 = g.batch1 = 1
            if rng.random() < 0.3:
                g.n_group = g.batch0 = rng.randint(1, 4)
                for i in range(g.n_group):
                    g.A_group[i], g.B_group[i], g.C_group[i] = ptr(), ptr(), ptr()
            elif rng.random() < 0.3:
                g.batch0 = rng.choice((2, 8, 64))
            g.a_b0, g.b_b0, g.c_b0 = M * K, N * K, M * N
            g.reduce_batch = int(rng.random() < 0.2)
            g.split_k = rng.choice((0, 0, 1, 2, 64))
            g.bias = ptr() if rng.random() < 0.2 else None
            g.accumulate = int(rng.random() < 0.2)
            g.alpha = 1.0
            plan = binding.GemmPlan()
            rc = lib.calm_gemm_describe(ctypes.byref(g), ctypes.byref(plan))
            need = int(lib.calm_gemm_workspace_bytes(ctypes.byref(g)))
            if rc != 0:
                assert need == 0
                continue
            families.add(plan.family)
            assert need >= 0 and need % (4 * M * N) == 0, (need, M, N)
            assert need == 0 or det or plan.k_slices >= 48, (need, plan.k_slices)
            assert plan.grid == (min(plan.items, 256) if plan.family in (3, 4) else plan.items)
            assert plan.uses_workspace == 0                              # none offered
            if need:
                with_ws += 1
                g.workspace, g.workspace_bytes = 1 << 60, need - 4
                assert lib.calm_gemm_describe(ctypes.byref(g), ctypes.byref(plan)) == 0 and plan.uses_workspace == 0
            g.workspace, g.workspace_bytes = 1 << 60, need
            assert lib.calm_gemm_describe(ctypes.byref(g), ctypes.byref(plan)) == 0
            assert plan.uses_workspace == (need > 0)
    finally:
        for o, v in zip((opt_pipe, opt_pipe32, opt_det), saved):
            lib.calm_gemm_set_option(o, v)
    assert families == {0, 1, 2, 3, 4, 5} and with_ws > 100, (families, with_ws)        # the sweep reaches every case


# ---- what the streaming entry points refuse before they launch anything ----------------------------------------------
# name -> (a valid argument list with fake, 16-byte aligned device addresses; indices of the pointers that are required).
# The valid list itself is never passed: every call below changes it into one the entry point has to turn down in its
# argument checks, so no kernel is launched and nothing is dereferenced.
_P = 0x7f0000010000
_STREAMING = {
    "calm_layernorm_fwd": ([_P, _P, _P, _P, _P, 64, 672, 1e-5, 0, None], (0, 1, 2, 3, 4)),
    "calm_layernorm_bwd": ([_P, _P, _P, _P, _P, _P, _P, None, 64, 672, 0, _P, None], (0, 1, 2, 3, 4, 5, 6, 11)),
    "calm_rope_fwd": ([_P, _P, _P, _P, _P, 2, 16, 4, 24, 8, 0, 0, 0, None], (0, 1, 2, 3, 4)),
    "calm_rope_bwd": ([_P, _P, _P, _P, _P, _P, 2, 16, 4, 24, 8, 0, 0, 0, 0, _P, None], (0, 1, 2, 3, 4, 5, 15)),
    "calm_softmax_fwd": ([_P, 64, 224, None], (0,)),
    "calm_softmax_bwd": ([_P, _P, 64, 224, None], (0, 1)),
    "calm_softmax_bwd_heads": ([_P, _P, _P, 2, 4, 16, 224, None], (0, 1, 2)),
    "calm_sum_heads": ([_P, _P, 2, 4, 256, None], (0, 1)),
    "calm_latent_fwd": ([_P, None, _P, _P, _P, 64, 240, _P, None], (0, 2, 3, 4, 7)),
    "calm_latent_bwd": ([None, None, _P, None, _P, _P, 64, 240, None], (2, 4, 5)),
    "calm_add": ([_P, _P, _P, 1024, None], (0, 1, 2)),
    "calm_gelu_fwd": ([_P, _P, 1024, None], (0, 1)),
    "calm_gelu_bwd": ([_P, _P, _P, 1024, None], (0, 1, 2)),
    "calm_colsum": ([_P, _P, 64, 672, 0, _P, None], (0, 1, 5)),
    "calm_row_scale": ([_P, _P, _P, 64, 672, 0, None], (0, 1, 2)),
    "calm_mean_seq_fwd": ([_P, _P, 2, 16, 64, None], (0, 1)),
    "calm_mean_seq_bwd": ([_P, _P, 2, 16, 64, None], (0, 1)),
    "calm_cnn_residual_fwd": ([_P] * 11 + [2, 32, 32, 1, None], tuple(range(11))),
    "calm_cnn_residual_bwd": ([_P] * 18 + [2, 32, 32, 1, _P, None], tuple(range(18)) + (22,)),
    "calm_soft_ce_fwd": ([_P, 1000, _P, 1000, _P, _P, None, 8, 1000, _P, None], (0, 2, 4, 5, 9)),
    "calm_soft_ce_bwd": ([_P, 1000, _P, 1000, _P, _P, _P, 8, 1000, None], (0, 2, 4, 5, 6)),
    "calm_huber_tokens_fwd": ([_P, _P, 1.0, _P, 2, 32, _P, None], (0, 1, 3, 6)),
    "calm_huber_tokens_bwd": ([_P, _P, 1.0, _P, _P, 2, 32, None], (0, 1, 3, 4)),
    "calm_top1_count": ([_P, 1000, _P, _P, 8, 1000, None], (0, 2, 3)),
}
# (name, {argument index: value}, expected code, what it is)
_REFUSED = [
    ("calm_layernorm_fwd", {8: 2}, "E_INVAL", "y_type fp8"),
    ("calm_layernorm_fwd", {8: -1}, "E_INVAL", "y_type negative"),
    ("calm_layernorm_bwd", {10: 3}, "E_INVAL", "dy_type fp8"),
    ("calm_layernorm_bwd", {9: 2049}, "E_UNSUPP", "D above 2048"),
    ("calm_layernorm_bwd", {9: 4096}, "E_UNSUPP", "D above 2048"),
    ("calm_rope_fwd", {10: 2}, "E_INVAL", "content_type fp8"),
    ("calm_rope_fwd", {11: 2}, "E_INVAL", "xr_type fp8"),
    ("calm_rope_fwd", {12: 7}, "E_INVAL", "out_type unknown"),
    ("calm_rope_fwd", {9: 7}, "E_INVAL", "odd dr"),
    ("calm_rope_bwd", {11: 2}, "E_INVAL", "dout_type fp8"),
    ("calm_rope_bwd", {12: 2}, "E_INVAL", "xr_type fp8"),
    ("calm_rope_bwd", {13: 2}, "E_INVAL", "dcontent_type fp8"),
    ("calm_rope_bwd", {14: 2}, "E_INVAL", "dxr_type fp8"),
    ("calm_rope_bwd", {10: 7}, "E_INVAL", "odd dr"),
    ("calm_rope_bwd", {10: 514}, "E_UNSUPP", "257 rotation pairs"),
    ("calm_rope_bwd", {10: 1024}, "E_UNSUPP", "512 rotation pairs"),
    ("calm_rope_bwd", {6: 1 << 15, 7: 1 << 10, 8: 2, 9: 24, 10: 8}, "E_UNSUPP", "2^31 elements"),
    ("calm_rope_bwd", {6: 1 << 16, 7: 1 << 10, 8: 4, 9: 0, 10: 8}, "E_UNSUPP", "2^31 elements, no content"),
    ("calm_softmax_fwd", {2: 1025}, "E_UNSUPP", "cols above 1024"),
    ("calm_softmax_bwd", {3: 1025}, "E_UNSUPP", "cols above 1024"),
    ("calm_softmax_bwd_heads", {6: 1025}, "E_UNSUPP", "cols above 1024"),
    ("calm_colsum", {4: 2}, "E_INVAL", "x_type fp8"),
    ("calm_colsum", {3: 4097}, "E_UNSUPP", "cols above 4096"),
    ("calm_colsum", {3: 8192}, "E_UNSUPP", "cols above 4096"),
    ("calm_row_scale", {5: 2}, "E_INVAL", "out_type fp8"),
    ("calm_cnn_residual_fwd", {13: 16}, "E_UNSUPP", "hidden 16"),
    ("calm_cnn_residual_fwd", {13: 64}, "E_UNSUPP", "hidden 64"),
    ("calm_cnn_residual_bwd", {20: 16}, "E_UNSUPP", "hidden 16"),
    ("calm_cnn_residual_bwd", {20: 64}, "E_UNSUPP", "hidden 64"),
    ("calm_huber_tokens_fwd", {5: 30}, "E_UNSUPP", "S % 4 != 0"),
    ("calm_huber_tokens_fwd", {5: 223}, "E_UNSUPP", "S % 4 != 0"),
    ("calm_huber_tokens_bwd", {6: 30}, "E_UNSUPP", "S % 4 != 0"),
    ("calm_huber_tokens_bwd", {6: 223}, "E_UNSUPP", "S % 4 != 0"),
]


def test_streaming_entry_points_refuse_bad_arguments_before_any_launch():
    """The argument checks of the streaming entry points (csrc/norm_act.hip, cnn_fused.hip, loss.hip) on a host without a
    GPU: a null required pointer, a storage type other than fp32 / bf16 and an odd rotation width are CALM_E_INVAL; a
    shape no kernel is compiled for is CALM_E_UNSUPP (softmax rows above 1024, LayerNorm backward rows above 2048, column
    sums above 4096 columns, a RoPE backward with more than 256 rotation pairs or 2^31 elements, a CNN tail whose hidden
    width is not 32, a Huber loss on an image side that is not a multiple of 4).  The expected codes are those of the
    library before its launch code was rewritten (one launch helper, typed dispatch): they are part of the C-ABI."""
    sys.path.insert(0, ROOT)
    from importlib import import_module
    binding = import_module("calm_vit_dte_amd._lib")
    lib = binding.load()
    assert sorted(n for n in binding.SIGNATURES if re.match(
        r"calm_(layernorm|rope|softmax|sum_heads|latent|add$|gelu|colsum|row_scale|mean_seq|cnn_residual|soft_ce|huber|top1)", n)
    ) == sorted(_STREAMING)                                        # the table names every streaming entry point
    calls = 0
    for name, (valid, required) in _STREAMING.items():
        assert len(valid) == len(binding.SIGNATURES[name][1]), name
        for i in required:                                          # one null pointer at a time
            args = list(valid)
            args[i] = None
            assert getattr(lib, name)(*args) == binding.E_INVAL, (name, "null pointer", i)
            calls += 1
    for name, change, code, what in _REFUSED:
        args = list(_STREAMING[name][0])
        for i, v in change.items():
            args[i] = v
        assert getattr(lib, name)(*args) == getattr(binding, code), (name, what)
        calls += 1
    assert calls > 120
