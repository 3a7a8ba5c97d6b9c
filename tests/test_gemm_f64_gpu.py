"""calm_gemm against float64 on every compiled kernel instance (gemm_f64.CENSUS; test_gemm_f64_cpu.py proves on the host
that the tables used here plan exactly that set).  Every test first asserts through calm_gemm_describe that the launch
plans the kernel it names, then runs it from operands between NaN fences into a C inside a NaN guard band.  Operands are
integers from +-1..8, so the fp32 accumulator is exact in every family, through atomics and workspace partials too: plain
launches, k-split launches, grouped and batch-summed launches must equal the float64 product BIT FOR BIT (bf16 C: its
round-to-nearest-even).  Epilogues are held to the element-wise bound derived in gemm_f64's docstring."""
import pytest
import torch

import calm_vit_dte_amd  # noqa: F401  (the package: its library is what gemm_f64.binding() loads)
import gemm_f64 as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return G.binding().load()


@pytest.mark.parametrize("case", G.instance_cases(), ids=G.case_id)
def test_instance_equals_the_float64_product_bit_for_bit(lib, case):
    with G.options(lib, case):
        L = G.Launch(case)
        key, plan = L.plan(lib)
        assert list(key) == case["key"] and plan["k_slices"] == 1, (key, plan)
        L.run(lib)
    L.C.check()
    G.compare_exact(L.C.values(), L.acc, plan, case)


_EPI = G.epilogue_cases()


@pytest.mark.parametrize("name,case,epi,family,form", _EPI, ids=[e[0] for e in _EPI])
def test_epilogue_within_the_fp32_bound(lib, name, case, epi, family, form):
    with G.options(lib, case):
        L = G.Launch(case, epi, seed=3)
        key, plan = L.plan(lib)
        assert (key.family, key.epi) == (family, form) and plan["k_slices"] == 1, (key, plan)
        L.run(lib)
    ref, bound, pre, pre_bound = L.reference()
    L.C.check()
    G.compare_bounded(L.C.values(), ref, bound, plan, name)
    if L.C_pre is not None:
        L.C_pre.check()
        G.compare_bounded(L.C_pre.values(), pre, pre_bound, plan, name, what="C_pre")


_SPLIT = G.split_launches()


@pytest.mark.parametrize("name,case,epi,family,workspace", _SPLIT, ids=[s[0] for s in _SPLIT])
def test_split_k_is_exact(lib, name, case, epi, family, workspace):
    """atomics, workspace partials + fixed-order reduction (vector and one-element, strided C rows, accumulating), the
    deterministic option: all exact on integer operands; two deterministic runs bit-equal to each other as well"""
    outs = []
    with G.options(lib, G.full_case(case)):
        for _ in range(2 if workspace else 1):
            L = G.Launch(case, epi, seed=5)
            key, plan = L.plan(lib)
            assert key.family == family and key.epi == 1 and plan["k_slices"] > 1, (key, plan)
            L.run(lib, workspace=workspace)
            assert G.describe(lib, L.g)[1]["uses_workspace"] == int(workspace)
            L.C.check()
            outs.append(L.C.values())
    ref = L.acc + (L.ops["c_old"].double() if "c_old" in L.ops else 0.0)
    G.compare_exact(outs[0], ref, plan, name)
    if workspace:
        assert torch.equal(G.bits_of(outs[0]), G.bits_of(outs[1]))


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("name,case,family,split", G.GROUP_CASES, ids=[c[0] for c in G.GROUP_CASES])
def test_grouped_and_batch_summed_launches_are_exact(lib, name, case, family, split, det):
    case = dict(case, det=det)
    with G.options(lib, G.full_case(case)):
        L = G.Launch(case, seed=7)
        key, plan = L.plan(lib)
        assert key.family == family and (plan["k_slices"] > 1) == split and key.epi == (1 if split else 4), (key, plan)
        L.run(lib)
    L.C.check()
    G.compare_exact(L.C.values(), L.acc, plan, name)


@pytest.mark.parametrize("operand", ["A", "B"])
@pytest.mark.parametrize("kernel", G.NAN_KERNELS, ids=lambda k: "f%d-%dx%d" % tuple(k[:3]))
def test_nan_poisons_exactly_its_row_or_column(lib, kernel, operand):
    """a NaN in A (last batch entry, last row: the M tail; last k: the k tail) poisons that output row and nothing else; one
    in B (first batch entry, last column, first k) that output column"""
    case = G.table_case(kernel)
    M, N, K, b0, b1 = (case[f] for f in ("M", "N", "K", "b0", "b1"))
    at = (b0 - 1, b1 - 1, M - 1, K - 1) if operand == "A" else (0, 0, N - 1, 0)
    with G.options(lib, case):
        L = G.Launch(case, seed=9, poison=(operand, at))
        key, plan = L.plan(lib)
        assert list(key) == case["key"], (key, plan)
        L.run(lib)
    L.C.check(allow_nan=True)
    got = L.C.values()
    want = torch.zeros(b0, b1, M, N, dtype=torch.bool)
    if operand == "A":
        want[at[0], at[1], at[2], :] = True
    else:
        want[at[0], at[1], :, at[2]] = True
    nan = torch.isnan(got.float())
    assert torch.equal(nan, want), G.failure_report(nan != want, plan, case)
    ref = L.acc.clone()
    G.compare_exact(torch.where(want, torch.zeros((), dtype=got.dtype), got), torch.where(want, 0.0, ref), plan, case)
