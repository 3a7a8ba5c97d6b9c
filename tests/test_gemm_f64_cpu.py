"""The calm_gemm float64 tests without a GPU: (1) the case tables of gemm_f64 / tests/golden/gemm_f64_cases.json,
passed through calm_gemm_describe (host code; fake 16-byte aligned addresses as in test_abi_cpu.py), plan exactly the
compiled kernel instances of gemm_f64.CENSUS — every one of them, each case the one it names; (2) the checker catches
planted faults in CPU-made "kernel outputs" and passes clean ones."""
import itertools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "calm-vit-dte_amd", "libcalmvit_hip.so")

import gemm_f64 as G

# caps on the GPU case table: it may not quietly grow heavy
MAX_INSTANCE_CASES = len(G.CENSUS)          # one per instance
MAX_CASE_MACS = 2.2e9                       # multiply-adds of the largest case (the 256 x 256 pipelined bf16 tiles)
MAX_TOTAL_MACS = 6.0e10                     # ... of all instance cases together
MAX_EPILOGUE_CASES, MAX_SPLIT_CASES = 100, 12

# Instances no argument set reaches: (census entry, the dispatcher condition that excludes it).  Empty: the sweep of
# scripts/gemm_instance_sweep.py found arguments for all 209.
UNREACHABLE = []


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return G.binding().load()


def _described(lib, case, epi=None):
    with G.options(lib, G.full_case(case)):
        g = G.fake_args(case, epi)
        rc, plan = G.describe(lib, g)
    assert rc == 0, (rc, case)
    return G.instance_key(g, plan), plan


# ------------------------------------------------------------------------------------------------------- coverage
def test_case_table_reaches_exactly_the_census(lib):
    cases = G.instance_cases()
    assert len(cases) <= MAX_INSTANCE_CASES
    assert max(G.macs(c) for c in cases) <= MAX_CASE_MACS
    assert sum(G.macs(c) for c in cases) <= MAX_TOTAL_MACS
    reached = set()
    for c in cases:
        key, plan = _described(lib, c)
        assert list(key) == c["key"], (c, key)                       # the case plans the instance it names
        assert plan["k_slices"] == 1 and G.macs(c) // (c["M"] * c["N"]) <= G.MAX_TERMS
        reached.add(G.kernel_of(key))
    exempt = {tuple(k) for k, _ in UNREACHABLE}
    assert exempt <= G.CENSUS and not (exempt & reached)
    assert reached | exempt == G.CENSUS, sorted(G.CENSUS - reached - exempt)
    assert reached <= G.CENSUS, sorted(reached - G.CENSUS)


def test_cases_are_ragged(lib):
    """M has a tail that is no multiple of 16, N one that is no multiple of the tile, both behind at least one full tile
    (the sweep found such arguments for every instance), K a tail shorter than the k-tile; and
    K % 8 == 4 wherever every k-contiguous operand is fp32 (a bf16 row of K elements is staged in 16-byte vectors of 8)."""
    for c in G.instance_cases():
        key, plan = _described(lib, c)
        assert c["M"] % 16 and c["N"] % key.tile_n and c["K"] % plan["tile_k"], c
        assert c["M"] > key.tile_m and c["N"] > key.tile_n, c          # a full tile, then the tail: an interior tile boundary
        k_free = all(st == G.ST_F32 or not kc for st, kc in ((c["a_st"], c["akc"]), (c["b_st"], c["bkc"])))
        if k_free and not c["scalar"]:
            assert c["K"] % 8 == 4, c
        if c["scalar"]:
            assert key.staging == 1


def test_epilogue_and_split_tables_reach_every_epilogue_form(lib):
    epi = G.epilogue_cases()
    assert len(epi) <= MAX_EPILOGUE_CASES and len(G.SPLIT_CASES) <= MAX_SPLIT_CASES
    forms = set()
    for name, c, e, family, form in epi:
        key, _ = _described(lib, c, e)
        assert (key.family, key.epi) == (family, form), (name, key)
        assert G.macs(c) <= MAX_CASE_MACS
        forms.add((key.family, key.epi))
    for name, c, family in G.SPLIT_CASES:
        for det in (0, 1):
            key, plan = _described(lib, dict(c, det=det))
            assert key.family == family and plan["k_slices"] > 1 and key.epi == 1, (name, key, plan)
            assert G.macs(c) <= MAX_CASE_MACS and c["K"] <= G.MAX_TERMS
            with G.options(lib, G.full_case(dict(c, det=det))):
                need = lib.calm_gemm_workspace_bytes(G.fake_args(c))
            assert need > 0 if det else need >= 0
        forms.add((key.family, key.epi))
    assert forms == set(G.EPILOGUE_FORMS), sorted(set(G.EPILOGUE_FORMS) ^ forms)


def test_split_group_and_batch_summed_launches_plan_what_they_name(lib):
    """every way the GPU file combines k-slices (gemm_f64.split_launches), and the grouped and reduce_batch launches of
    GROUP_CASES: the family, that the slices are combined (one element per access) or, unsplit over groups, that they
    are not — the branches of `atomic` in instance_key"""
    launches = G.split_launches()
    assert len(launches) <= 5 * MAX_SPLIT_CASES and len(G.GROUP_CASES) <= MAX_SPLIT_CASES
    for name, c, e, family, workspace in launches:
        key, plan = _described(lib, c, e)
        assert key.family == family and plan["k_slices"] > 1 and key.epi == 1, (name, key, plan)
    for name, c, family, split in G.GROUP_CASES:
        assert G.macs(c) <= MAX_CASE_MACS and c["K"] * (c["b0"] if c.get("reduce_batch") else 1) <= G.MAX_TERMS
        for det in (0, 1):
            key, plan = _described(lib, dict(c, det=det))
            assert key.family == family and (plan["k_slices"] > 1) == split and key.epi == (1 if split else 4), (name, key, plan)
    kinds = {(f, bool(c.get("grouped")), bool(c.get("reduce_batch"))) for _, c, f, _ in G.GROUP_CASES}
    assert {(0, False, True), (1, False, True), (0, True, False), (1, True, False), (3, True, False), (4, True, False),
            (0, True, True), (1, True, True)} <= kinds
    assert sorted({k[0] for k in G.NAN_KERNELS}) == [0, 1, 2, 3, 4, 5] and len(G.NAN_KERNELS) == 7


def sweep_for(lib, kernel, limit=None):
    """Every argument set of the describe sweep that plans `kernel`: its layouts, storage types and matrix pipe; every
    setting of the options that bear on it (default first), split_k 0 / 1 / 2, batch in {1, 4, 16, 64, 256}, M and N over
    1..2056 on a grid of 64 plus the ragged sizes of the case tables, K in {3, 37, 40, 64, 160, 200}.  Yields the cases."""
    family, _, _, akc, bkc, staging, a_st, b_st, npass = kernel
    dtype = G.F32 if family in (0, 4) else G.BF16X3 if npass == 3 else G.BF16
    used = {c[d] for c in G.instance_cases() for d in "MN"} | {c[d] for _, c, _ in G.SPLIT_CASES for d in "MN"}
    sizes = sorted({1, 2056} | set(range(64, 2049, 64)) | {s for s in used if s <= 2056})
    pipes = (1, 0) if (a_st, b_st) == (G.ST_BF16, G.ST_BF16) else (1,)          # the option only bears on bf16 pairs
    pipe32s = (0, 1, 2) if dtype == G.F32 else (0,)                             # ... and this one on fp32 launches
    found = 0
    for pipe, pipe32, det, split_k in itertools.product(pipes, pipe32s, (0, 1), (1, 0, 2)):
        for c_st in ((0,) if dtype != G.BF16 else (0, 1)):
            base = dict(akc=akc, bkc=bkc, dtype=dtype, a_st=a_st, b_st=b_st, c_st=c_st, pipe=pipe, pipe32=pipe32, det=det,
                        split_k=split_k, scalar=int(staging == 1))
            with G.options(lib, G.full_case(dict(base, M=1, N=1, K=1))):
                for M, N, K, b0 in itertools.product(sizes, sizes, (3, 37, 40, 64, 160, 200), (1, 4, 16, 64, 256)):
                    c = dict(base, M=M, N=N, K=K, b0=b0)
                    g = G.fake_args(c)
                    rc, plan = G.describe(lib, g)
                    if rc == 0 and G.kernel_of(G.instance_key(g, plan)) == tuple(kernel):
                        yield c
                        found += 1
                        if limit and found >= limit:
                            return


def test_unreachable_instances_are_unreachable(lib):
    """An instance is exempt from the coverage only with its dispatcher condition written in UNREACHABLE, and only while
    the describe sweep finds no arguments for it.  The sweep itself is checked on an instance the table does reach."""
    for kernel, why in UNREACHABLE:
        assert why
        assert next(sweep_for(lib, kernel, limit=1), None) is None, (kernel, why)
    probe = (3, 128, 128, 1, 1, 16, 1, 1, 1)
    assert next(sweep_for(lib, probe, limit=1), None) is not None


# ------------------------------------------------------------------------------------------ checker self-test
M_, N_, K_, B0 = 150, 136, 100, 2            # two 128-row tiles in M and N, K tail 4


@pytest.fixture(scope="module")
def clean():
    A, B = G.exact_operand(B0, 1, M_, K_, 1), G.exact_operand(B0, 1, N_, K_, 2)
    return A, B, G.product64(A, B)


PLAN = dict(family=0, tile_m=128, tile_n=128, tile_k=16, tiles_m=2, tiles_n=2, k_slices=1, items=8, grid=8, epi_unit=0,
            uses_workspace=0, threads=256)


def _caught(fn, *a, **kw):
    with pytest.raises(AssertionError) as e:
        fn(*a, **kw)
    return str(e.value)


def test_exact_operands_are_exact_in_every_storage_type(clean):
    A, B, ref = clean
    assert int(A.abs().min()) == 1 and int(A.abs().max()) == 8
    for st in (G.ST_BF16, G.ST_E4M3, G.ST_E5M2):
        assert torch.equal(A.to(G.TORCH_ST[st]).float(), A)
    assert float(ref.abs().max()) < 2 ** 24 and torch.equal(ref, ref.round())
    assert 64 * G.MAX_TERMS <= 2 ** 24


def test_clean_outputs_pass(clean):
    A, B, ref = clean
    G.compare_exact(ref.float(), ref, PLAN)
    G.compare_exact(ref.bfloat16(), ref, PLAN)
    C = G.Guarded(B0, 1, M_, N_, device="cpu")
    C.t.copy_(ref.float())
    assert torch.equal(C.check(), ref)
    C16 = G.Guarded(B0, 1, M_, N_, dtype=torch.bfloat16, device="cpu")
    C16.t.copy_(ref.bfloat16())
    G.compare_exact(C16.values(), ref, PLAN)
    C16.check()


@pytest.mark.parametrize("fault", ["k_element_dropped", "k_tile_twice", "rows_swapped", "k_slice_missing"])
def test_planted_product_faults_are_caught(clean, fault):
    A, B, ref = clean
    a, b = A.double(), B.double()
    got = ref.clone()
    if fault == "k_element_dropped":                 # tile (0, 1) of batch entry 1 skips k = 97
        got[1, 0, :128, 128:] -= a[1, 0, :128, 97:98] @ b[1, 0, 128:, 97:98].T
    elif fault == "k_tile_twice":                    # tile (1, 0) adds its k-tile 16..31 twice
        got[0, 0, 128:, :128] += a[0, 0, 128:, 16:32] @ b[0, 0, :128, 16:32].T
    elif fault == "rows_swapped":
        a2 = a.clone()
        a2[0, 0, [3, 4]] = a[0, 0, [4, 3]]
        got = a2 @ b.transpose(-1, -2)
    elif fault == "k_slice_missing":                 # the last of four k-slices never arrives
        got -= a[..., 75:] @ b[..., 75:].transpose(-1, -2)
    for out in (got.float(), got.bfloat16()):
        msg = _caught(G.compare_exact, out, ref, PLAN)
        assert "by tile" in msg and "plan" in msg
    if fault == "k_element_dropped":
        assert "by tile: {1: " in msg and "by batch: {1: " in msg        # the report names the tile and the batch entry


def test_stale_element_and_guard_band_store_are_caught(clean):
    _, _, ref = clean
    for dtype in (torch.float32, torch.bfloat16):
        C = G.Guarded(B0, 1, M_, N_, dtype=dtype, device="cpu")
        C.t.copy_(ref.to(dtype))
        C.check()
        stale = G.Guarded(B0, 1, M_, N_, dtype=dtype, device="cpu")
        keep = stale.t[1, 0, 149, 135].clone()
        stale.t.copy_(ref.to(dtype))
        stale.t[1, 0, 149, 135] = keep
        assert "not written" in _caught(stale.check)
        assert "not written" in _caught(stale.check, allow_nan=True)
        C.buf[C.off + N_] = 1.0                       # first guard column right of row 0
        assert "outside C" in _caught(C.check)
        C2 = G.Guarded(B0, 1, M_, N_, dtype=dtype, device="cpu")
        C2.t.copy_(ref.to(dtype))
        C2.buf[C2.off + M_ * C2.ld] = float("nan")    # row M of batch entry 0: a NaN, but not the fill
        assert "outside C" in _caught(C2.check)


@pytest.mark.parametrize("st,kcontig", [(G.ST_F32, True), (G.ST_BF16, True), (G.ST_F32, False), (G.ST_E4M3, True)])
def test_fenced_pad_read_as_k_tail_is_caught(clean, st, kcontig):
    """A kernel that feeds its k-tail from the operand's pad columns (or its next k-row) and multiplies by zero: NaN x 0."""
    A, B, ref = clean
    fa = G.Fenced(A, kcontig, st, device="cpu")
    rs, cs, s0, s1 = fa.strides
    assert torch.equal(fa.t.float(), A)                                       # the operand itself reads back
    over = fa.buf.as_strided((B0, 1, M_, K_ + 1), (s0, s1, rs, cs), fa.off)    # one element past K
    assert torch.isnan(over[..., K_].float()).all()
    before = fa.buf.as_strided((B0, 1, 1, K_), (s0, s1, rs, cs), fa.off - (rs if kcontig else 1))   # row -1
    assert torch.isnan(before.float()).all()
    b_pad = torch.cat([B, torch.zeros(B0, 1, N_, 1)], dim=-1)
    got = over.float().double() @ b_pad.double().transpose(-1, -2)
    C = G.Guarded(B0, 1, M_, N_, device="cpu")
    C.t.copy_(got.float())
    _caught(C.check)
    assert "wrong elements" in _caught(G.compare_exact, got.float(), ref, PLAN)


def test_fence_geometry_keeps_staging_kind():
    for st, m in ((G.ST_F32, 4), (G.ST_BF16, 8), (G.ST_E4M3, 16)):
        for kc in (True, False):
            off, (rs, cs, s0, s1), numel = G.fence_geometry(150, 104, 3, 2, kc, st)
            ld = rs if kc else cs
            assert ld % m == 0 and ld >= (104 if kc else 150) + m and off % m == 0 and s0 % m == 0 and s1 % m == 0
            assert off + 2 * s0 + s1 + 150 * 104 * 0 + (149 * rs + 103 * cs) < numel
    off, (rs, cs, s0, s1), _ = G.fence_geometry(150, 104, 1, 1, True, G.ST_F32, scalar=True)
    assert rs % 4 != 0


def _epilogue_operands():
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(bias=rn(N_), col_scale=rn(N_), aux=1.5 * rn(B0, 1, M_, N_), residual=rn(B0, 1, M_, N_), c_old=rn(B0, 1, M_, N_),
                inv_scale=torch.tensor([1.3]))


def _fp32_epilogue(acc, alpha, inv_scale, bias, act=0, aux=None, col_scale=None, residual=None, c_old=None):
    """what a correct kernel stores: the epilogue's operations in its order, each rounded to fp32 (GELU and GELU' exact,
    rounded once)"""
    r = lambda t: t.float().double()
    s = r(torch.tensor(alpha, dtype=torch.float64) / inv_scale.double())
    v = r(r(acc * s) + bias.double())
    pre = v
    if act == G.ACT_GELU:
        v = r(G.gelu64(v))
    elif act == G.ACT_GELU_BWD:
        v = r(v * r(G.gelu_grad64(aux.double())))
    if col_scale is not None:
        v = r(v * col_scale.double())
    for t in (residual, c_old):
        if t is not None:
            v = r(v + t.double())
    return v.float(), pre.float()


EPI = {"gelu_pre": dict(act=G.ACT_GELU), "gelu_bwd": dict(act=G.ACT_GELU_BWD, aux=1), "scale_res": dict(col_scale=1, residual=1),
       "accumulate": dict(c_old=1)}


@pytest.mark.parametrize("name", list(EPI))
def test_epilogue_checker_passes_clean_and_catches_faults(clean, name):
    _, _, acc = clean
    ops = _epilogue_operands()
    alpha = float(torch.tensor(1.3 / (25.5 * K_ ** 0.5), dtype=torch.float32))
    kw = dict(alpha=alpha, inv_scale=ops["inv_scale"], bias=ops["bias"], act=EPI[name].get("act", 0))
    kw.update({k: ops[k] for k in ("aux", "col_scale", "residual", "c_old") if k in EPI[name]})
    ref, bound, pre, pre_bound = G.epilogue_reference(acc, **kw)
    got, got_pre = _fp32_epilogue(acc, **kw)
    assert float(ref.abs().max()) > 1.0 and float((bound / ref.abs().clamp_min(1e-3)).median()) < 1e-5
    G.compare_bounded(got, ref, bound, PLAN)
    G.compare_bounded(got_pre, pre, pre_bound, PLAN, what="C_pre")
    G.compare_bounded(got.bfloat16(), ref, bound, PLAN)
    # the bias of the neighbouring column
    wrong, _ = _fp32_epilogue(acc, **dict(kw, bias=ops["bias"].roll(1)))
    assert "by tile" in _caught(G.compare_bounded, wrong, ref, bound, PLAN)
    _caught(G.compare_bounded, wrong.bfloat16(), ref, bound, PLAN)
    # a bf16 store that truncates instead of rounding to nearest even
    trunc = (got.view(torch.int32) & -65536).view(torch.float32).bfloat16()
    assert "equal the rounded reference" in _caught(G.compare_bounded, trunc, ref, bound, PLAN)
    # one element a few fp32 ulps off, far beyond u per operation
    off = got.clone()
    off[1, 0, 77, 130] += 64 * 2.0 ** -24 * max(1.0, float(off[1, 0, 77, 130].abs()))
    assert "first at (1, 0, 77, 130)" in _caught(G.compare_bounded, off, ref, bound, PLAN)


def test_truncated_bf16_product_is_caught(clean):
    _, _, ref = clean
    trunc = (ref.float().view(torch.int32) & -65536).view(torch.float32).bfloat16()
    assert bool((trunc != ref.bfloat16()).any())
    _caught(G.compare_exact, trunc, ref, PLAN)


def test_census_counts():
    fam = lambda f: sum(1 for k in G.CENSUS if k[0] == f)
    assert [fam(f) for f in range(6)] == [64, 40, 16, 45, 42, 2]
    assert len({k[:5] for k in G.CENSUS if k[0] in (3, 4)}) == 87
