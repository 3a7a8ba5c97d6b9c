"""Shared checker and case tables of calm_gemm against float64, by compiled kernel instance (test_gemm_f64_cpu.py proves
them on the host; test_gemm_f64_gpu.py launches them).

Which kernel a calm_gemm call runs is decided by the cost models of plan_gemm() (csrc/gemm.hip), so a test that names a
shape does not name a kernel.  Everything here is therefore keyed by `instance_key`: the template arguments of the
launchers, recomputed from the launch arguments and from what calm_gemm_describe answers.

Exact operands.  A and B hold integers from +-1..8 (no zeros: every dropped product changes the sum; exact in fp32, bf16,
e4m3 and e5m2, and their bf16 hi / lo split is (value, 0)).  |a b| <= 64, so with at most MAX_TERMS = 2^18 products per
output element every partial sum, in any order and through atomics or workspace partials, is an integer below 2^24: the
fp32 accumulator of every family is EXACT.  A plain launch into an fp32 C must equal the float64 product bit for bit, one
into a bf16 C its round-to-nearest-even bf16, bit for bit.  No tolerance is involved.

Epilogue bound (`epilogue_reference`).  Both epilogues (gemm_epilogue of gemm_common.h; pipe_epilogue_rows of
gemm_bf16p.h, which differs only in rounding acc x scale before the bias is added, where the former may contract the two
into one fma) apply, in this order and in fp32, to the exact accumulator `acc`:

    s  = alpha / inv_scale                  one division                   u |s|         (relative u on everything below)
    v1 = acc s + bias                       product, add                   u |acc s| + u |v1|
         C_pre = v1                         (stored; bf16 C_pre: one more rounding)
    v2 = gelu(v1)                           |gelu'| <= 1.13 carries e1     1.13 e1 + 2 GELU_FWD_ERR max(1, |v1|)
      or v1 gelu'(aux)                      gelu' evaluation, product      e1 |g| + |v1| 2 GELU_BWD_ERR max(1, |aux|) + u |v2|
    v3 = v2 col_scale                       product                        e2 |cs| + u |v3|
    v4 = v3 + residual                      add                            e3 + u |v4|
    v5 = v4 + C_old                         add                            e4 + u |v5|

with u = U32 = 2^-24, every magnitude taken from the float64 intermediate.  GELU_FWD_ERR / GELU_BWD_ERR are the errors of
gelu_erf_f / gelu_erf_grad_f of common.h against float64, measured once on an MI355X over [-12, 12] by the stand-alone
GELU kernels (docstring of test_rowwise_f64_gpu.py) and asserted at twice their value as there; no constant is fitted to a
GEMM kernel.  The sum is widened by SECOND_ORDER = 1 + 2^-12 for the products of two roundings the first-order terms
leave out (each term above is computed from an intermediate that is itself off by a few u).  bf16 stores are checked with
attn16_f64.assert_bf16_rounding_of: the float64 reference rounded once, or one ulp away within the fp32 bound.
"""
import ctypes
import math
from collections import Counter, namedtuple
from importlib import import_module

import torch

from attn16_f64 import FILL, GELU_BWD_ERR, GELU_FWD_ERR, assert_bf16_rounding_of, bf16_ulp

U32 = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -12
MAX_TERMS = 1 << 18           # products per output element for which the fp32 accumulator stays exact (64 x 2^18 = 2^24)

F32, BF16, BF16X3 = 0, 1, 2                         # calm_gemm_args.dtype
ST_F32, ST_BF16, ST_E4M3, ST_E5M2 = 0, 1, 2, 3      # CALM_ST_*
OPT_PIPE, OPT_PIPE32, OPT_DET = 0, 1, 2             # CALM_GEMM_OPT_*
ACT_NONE, ACT_GELU, ACT_GELU_BWD = 0, 1, 2
PRECISION_NAME = {F32: "fp32", BF16: "bf16", BF16X3: "bf16x3"}
ESIZE = {ST_F32: 4, ST_BF16: 2, ST_E4M3: 1, ST_E5M2: 1}
TORCH_ST = {ST_F32: torch.float32, ST_BF16: torch.bfloat16, ST_E4M3: torch.float8_e4m3fn, ST_E5M2: torch.float8_e5m2}
# NaN bit patterns the fences and guard bands are filled with: attn16_f64.FILL for fp32 / bf16 (quiet NaNs with payloads
# no arithmetic yields); fp8 has one NaN (e4m3fn: 0x7F) or few (e5m2: 0x7E is a quiet one)
FILL_BITS = {ST_F32: (torch.int32, FILL[torch.float32]), ST_BF16: (torch.int16, FILL[torch.bfloat16]),
             ST_E4M3: (torch.uint8, 0x7F), ST_E5M2: (torch.uint8, 0x7E)}


# ----------------------------------------------------------------------------------------------------- instances
Key = namedtuple("Key", "family tile_m tile_n akc bkc staging a_st b_st npass epi")
LAYOUTS = [(1, 1), (1, 0), (0, 1), (0, 0)]          # (A k-contiguous, B k-contiguous)
PIPE_LAYOUTS = [(1, 1), (1, 0), (0, 0)]             # plan_pipe: row-contiguous A with k-contiguous B is not instantiated


def _census():
    """Every main-kernel instance the launchers can reach: Key without its epilogue form (a run-time branch)."""
    c = []
    # family 0, 128-row tiles — gemm_f32.hip: launch_f32 (VEC 4 / 1 x 4 layouts) -> launch<AKC, BKC, VEC> (BN 128 / 96)
    c += [(0, 128, bn, a, b, st, 0, 0, 1) for st in (16, 1) for a, b in LAYOUTS for bn in (96, 128)]
    # family 0, 64-row tiles — gemm_f32.hip: launch_f32_t64 (VEC 4 / 1 x 4 layouts) -> launch_t64 (NB 3..8)
    c += [(0, 64, 16 * nb, a, b, st, 0, 0, 1) for st in (16, 1) for a, b in LAYOUTS for nb in range(3, 9)]
    # family 1 — gemm_bf16.hip: launch_bf16 (storage pairs; NPASS 3 on fp32 tensors only) -> launch_c_layout (4 layouts)
    # -> launch_c (BN 128 / 96)
    c += [(1, 128, bn, a, b, 16, sa, sb, np_) for sa, sb, np_ in ((0, 0, 1), (1, 1, 1), (1, 0, 1), (0, 1, 1), (0, 0, 3))
          for a, b in LAYOUTS for bn in (96, 128)]
    # family 2 — gemm_bf16.hip: launch_bf16_wide (4 storage pairs) -> launch_wide_t (4 layouts), 256 x 128
    c += [(2, 256, 128, a, b, 16, sa, sb, 1) for sa in (0, 1) for sb in (0, 1) for a, b in LAYOUTS]
    # families 3 / 4 — gemm.hip launch_main (3 layouts: gemm_{bf16,f32}p_{kk,km,mm}.hip) -> gemm_bf16p.h
    # launch_pipe_layout (MT 2..4) -> launch_pipe_nt (NT 4..8); plan_pipe never plans fp32 MT 4 x NT 8 (spills)
    c += [(3, 64 * mt, 32 * nt, a, b, 16, 1, 1, 1) for a, b in PIPE_LAYOUTS for mt in (2, 3, 4) for nt in range(4, 9)]
    c += [(4, 64 * mt, 32 * nt, a, b, 16, 0, 0, 1) for a, b in PIPE_LAYOUTS for mt in (2, 3, 4) for nt in range(4, 9)
          if (mt, nt) != (4, 8)]
    # family 5 — gemm_fp8.hip: launch_fp8 (A e5m2 / e4m3; B e4m3, both k-contiguous)
    c += [(5, 256, 128, 1, 1, 16, sa, ST_E4M3, 1) for sa in (ST_E4M3, ST_E5M2)]
    return frozenset(c)


CENSUS = _census()
assert len(CENSUS) == 16 + 48 + 40 + 16 + 45 + 42 + 2
# run-time epilogue forms per family: one element per access (unaligned tensors, atomics, workspace partials), 4 columns
# per lane (p.epi_vec), 8 columns per lane (pipelined bf16 family, every epilogue tensor bf16: p.epi_unit)
EPILOGUE_FORMS = frozenset([(f, e) for f in (0, 1, 2, 5) for e in (1, 4)] + [(3, 1), (3, 4), (3, 8), (4, 1), (4, 4)])


def _field(plan, name):
    return plan[name] if isinstance(plan, dict) else getattr(plan, name)


def _aligned16(p):
    return p is None or (int(p) & 15) == 0


def instance_key(g, plan):
    """Key of the kernel a launch runs: `g` the calm_gemm_args (ctypes), `plan` what calm_gemm_describe answered for it
    (struct or dict).  Family and tile are the plan's; layouts, storage types and passes are the arguments'; the staging
    kind and the epilogue form are recomputed from the conditions plan_gemm documents:
      staging  16-byte vectors (`vec`) when A and B (and every group's) are 16-byte aligned and each operand's contiguous
               extent, its stride and its batch strides are multiples of 4 (fp32) / 8 (bf16) elements; only the fp32
               family has one-element kernels (a bf16 tensor that cannot be staged is CALM_E_LAYOUT)
      epilogue 4 columns per lane (`epi_vec`) when N, C's strides, the residual's strides are multiples of 4 and C, C_pre,
               aux, bias, col_scale, residual are 16-byte aligned; one element per access otherwise and in every launch
               that combines k-slices (atomics / workspace); the pipelined families report theirs (epi_unit 4 / 8)."""
    family = _field(plan, "family")
    ma = 7 if g.a_type == ST_BF16 else 3
    mb = 7 if g.b_type == ST_BF16 else 3
    akc, bkc = int(g.a_cs == 1), int(g.b_cs == 1)
    vec = _aligned16(g.A) and _aligned16(g.B) and not (g.a_b0 & ma or g.a_b1 & ma or g.b_b0 & mb or g.b_b1 & mb)
    for i in range(g.n_group):
        vec = vec and _aligned16(g.A_group[i]) and _aligned16(g.B_group[i])
    vec = vec and not ((g.K & ma or g.a_rs & ma) if akc else (g.M & ma or g.a_cs & ma))
    vec = vec and not ((g.K & mb or g.b_rs & mb) if bkc else (g.N & mb or g.b_cs & mb))
    ev = not (g.N & 3 or g.c_rs & 3 or g.c_b0 & 3 or g.c_b1 & 3) and all(
        _aligned16(p) for p in (g.C, g.C_pre, g.aux, g.bias, g.col_scale, g.residual))
    ev = ev and (not g.residual or not (g.r_rs & 3 or g.r_b0 & 3 or g.r_b1 & 3))
    for i in range(g.n_group):
        ev = ev and _aligned16(g.C_group[i])
    atomic = _field(plan, "k_slices") > 1 or bool(g.reduce_batch and not (g.n_group and g.split_k <= 1))
    if family in (3, 4):
        epi = 1 if atomic else _field(plan, "epi_unit")
    else:
        epi = 4 if ev and not atomic else 1
    staging = 16 if (vec or family != 0) else 1
    npass = 3 if (family == 1 and g.dtype == BF16X3) else 1
    return Key(family, _field(plan, "tile_m"), _field(plan, "tile_n"), akc, bkc, staging, g.a_type, g.b_type, npass, epi)


def kernel_of(key):
    """the census entry of a Key: everything but the epilogue form"""
    return tuple(key[:-1])


# -------------------------------------------------------------------------------------------- layouts in memory
DEVICE = "cuda"                # where Guarded / Fenced allocate unless told otherwise (the CPU self-tests pass "cpu")
FENCE_ROWS = 2                 # NaN rows (k-rows) before and after every operand matrix
GUARD_ROWS, GUARD_COLS = 3, 12 # NaN rows above and below every C matrix, NaN columns beside it (4 left, 8 right)


def _mult(st):
    return 16 // ESIZE[st]


def fence_geometry(rows, K, b0, b1, kcontig, st, scalar=False):
    """Where a [b0, b1, rows, K] operand sits inside its fenced buffer: (offset, (rs, cs, s_b0, s_b1), numel), in elements.
    k-contiguous: rows of K elements at stride ld; row-contiguous: K k-rows of `rows` elements at stride ld.  ld exceeds
    the extent by at least one 16-byte vector and is a multiple of it — or, scalar=True (one-element staging wanted), is
    no multiple of 4; FENCE_ROWS rows of fill lie before and after every matrix, one vector before the first."""
    m = _mult(st)
    ext, lines = (K, rows) if kcontig else (rows, K)
    if scalar:
        ld = ext + 5
        ld += ld % 4 == 0
    else:
        ld = ((ext + m - 1) // m + 1) * m
    s1 = (lines + 2 * FENCE_ROWS) * ld
    strides = (ld, 1, b1 * s1, s1) if kcontig else (1, ld, b1 * s1, s1)
    return FENCE_ROWS * ld + m, strides, b0 * b1 * s1 + 2 * m


def guard_geometry(b0, b1, M, N, shift=0, st=ST_F32):
    """C-shaped tensor in its guard band: (offset, (rs, s_b0, s_b1), numel).  fp32: GUARD_COLS = 4 + 8 columns of fill; bf16:
    8 + 8, so that an N that is a multiple of 8 keeps strides that are (the 8-column epilogue)."""
    left, ld = (4, N + GUARD_COLS) if st == ST_F32 else (8, N + 16)
    rows = M + 2 * GUARD_ROWS
    return GUARD_ROWS * ld + left + shift, (ld, b1 * rows * ld, rows * ld), b0 * b1 * rows * ld + 8


def _filled(numel, st, device):
    it, bits = FILL_BITS[st]
    if it == torch.int32:
        bits -= 1 << 32 if bits >= 1 << 31 else 0
    return torch.full((numel,), bits, dtype=it, device=device).view(TORCH_ST[st])


class Guarded:
    """A [b0, b1, M, N] fp32 (or bf16) matrix inside a NaN-filled buffer (row stride N + GUARD_COLS, GUARD_ROWS rows above
    and below each matrix); `shift` moves it off 16-byte alignment (one-element epilogue).  The fill is attn16_f64.FILL:
    NaN bit patterns no kernel produces."""

    def __init__(self, b0, b1, M, N, shift=0, init=None, dtype=torch.float32, device=None):
        device = device or DEVICE
        st = ST_BF16 if dtype == torch.bfloat16 else ST_F32
        self.st = st
        self.off, self.strides, numel = guard_geometry(b0, b1, M, N, shift, st)
        self.ld = self.strides[0]
        self.buf = _filled(numel, st, device)
        size, stv = (b0, b1, M, N), (self.strides[1], self.strides[2], self.ld, 1)
        self.t = self.buf.as_strided(size, stv, self.off)
        self.mask = torch.zeros(self.buf.numel(), dtype=torch.bool, device=device)
        self.mask.as_strided(size, stv, self.off).fill_(True)
        self.view = self.buf[self.off:]              # what a launch gets as the tensor's base
        if init is not None:
            self.t.copy_(init)

    def _is_fill(self):
        it, bits = FILL_BITS[self.st]
        return self.buf.view(it) == (bits - (1 << 32) if bits >= 1 << 31 else bits)

    def check(self, allow_nan=False):
        """every element of C written and nothing around it; allow_nan: NaN results are legitimate (propagation tests)"""
        assert torch.isnan(self.buf[~self.mask].float()).all(), "a store landed outside C"
        assert bool(self._is_fill()[~self.mask].all()), "a store landed outside C"
        if allow_nan:
            assert not bool(self._is_fill()[self.mask].any()), "an element of C was not written"
        else:
            assert torch.isfinite(self.buf[self.mask].float()).all(), "an element of C was not written"
        return self.t.cpu().double()

    def values(self):
        return self.t.cpu()


class Fenced:
    """An operand [b0, b1, rows, K] (values: a CPU tensor) inside a larger buffer of the storage type `st`, laid out by
    fence_geometry: fill (NaN) before it and after it, in the pad columns between rows / k-rows and in FENCE_ROWS rows
    between batch entries.  The fences are allocated memory: a clamped or over-long read lands in NaN and shows in the
    output, never outside the allocation."""

    def __init__(self, values, kcontig, st=ST_F32, scalar=False, device=None):
        device = device or DEVICE
        b0, b1, rows, K = values.shape
        self.off, self.strides, numel = fence_geometry(rows, K, b0, b1, kcontig, st, scalar)
        self.buf = _filled(numel, st, device)
        rs, cs, s0, s1 = self.strides
        self.t = self.buf.as_strided((b0, b1, rows, K), (s0, s1, rs, cs), self.off)
        it = FILL_BITS[st][0]                        # copied as bit patterns: no conversion on the way
        self.buf.view(it).as_strided((b0, b1, rows, K), (s0, s1, rs, cs), self.off).copy_(
            values.to(TORCH_ST[st]).contiguous().view(it))
        self.view = self.buf[self.off:]


# ------------------------------------------------------------------------------------------------- exact operands
def exact_operand(b0, b1, rows, K, seed):
    """integers from +-1..8, no zeros, as fp32"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.randint(1, 9, (b0, b1, rows, K), generator=g)
    sign = torch.randint(0, 2, (b0, b1, rows, K), generator=g) * 2 - 1
    return (mag * sign).float()


def product64(A, B, chunk_bytes=1 << 27):
    """float64 A B^T per batch entry ([b0, b1, M, K] x [b0, b1, N, K] -> [b0, b1, M, N]), chunked over the batch"""
    b0, b1, M, K = A.shape
    N = B.shape[2]
    assert K <= MAX_TERMS
    a, b = A.reshape(b0 * b1, M, K), B.reshape(b0 * b1, N, K)
    out = torch.empty(b0 * b1, M, N, dtype=torch.float64, device=a.device)
    step = max(1, chunk_bytes // (8 * (M * K + N * K + M * N)))
    for i in range(0, b0 * b1, step):
        out[i:i + step] = a[i:i + step].double() @ b[i:i + step].double().transpose(1, 2)
    return out.view(b0, b1, M, N)


def bits_of(t):
    """the bit patterns of a bf16 / fp32 tensor, for bit-for-bit comparisons"""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# --------------------------------------------------------------------------------------------- epilogue reference
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def epilogue_reference(acc, alpha=1.0, inv_scale=None, bias=None, act=ACT_NONE, aux=None, col_scale=None, residual=None,
                       c_old=None):
    """(ref, bound, pre, pre_bound) in float64 from the exact accumulator, element-wise: the table of the module
    docstring.  Operands are the values the kernel reads (a bf16 aux / residual / C_old already rounded), broadcastable
    to acc's shape."""
    d = lambda t: None if t is None else (t.double() if torch.is_tensor(t) else torch.tensor(float(t), dtype=torch.float64))
    acc, bias, aux, col_scale, residual, c_old = (d(t) for t in (acc, bias, aux, col_scale, residual, c_old))
    s = float(torch.tensor(alpha, dtype=torch.float32)) / (float(inv_scale.float().reshape(-1)[0]) if inv_scale is not None else 1.0)
    rel = U32 if inv_scale is not None else 0.0            # the division's rounding: relative on acc s
    p = acc * s
    v = p + bias if bias is not None else p
    e = (rel + U32) * p.abs() + (U32 * v.abs() if bias is not None else 0.0)
    pre, pre_bound = v, e * SECOND_ORDER
    if act == ACT_GELU:
        e = 1.13 * e + 2 * GELU_FWD_ERR * v.abs().clamp_min(1.0)
        v = gelu64(v)
    elif act == ACT_GELU_BWD:
        g = gelu_grad64(aux)
        v2 = v * g
        e = e * g.abs() + v.abs() * 2 * GELU_BWD_ERR * aux.abs().clamp_min(1.0) + U32 * v2.abs()
        v = v2
    if col_scale is not None:
        v = v * col_scale
        e = e * col_scale.abs() + U32 * v.abs()
    for t in (residual, c_old):
        if t is not None:
            v = v + t
            e = e + U32 * v.abs()
    return v, e * SECOND_ORDER, pre, pre_bound


# ------------------------------------------------------------------------------------------------- failure report
def failure_report(bad, plan, spec=None):
    """text for an assertion: the plan and the locate.locate histograms (tile / wave / strip) of the wrong elements;
    `bad`: boolean [b0, b1, M, N]"""
    import locate
    idx = bad.reshape(-1, bad.shape[-2], bad.shape[-1]).nonzero()
    lines = [f"{int(bad.sum())} wrong elements of {bad.numel()}", f"plan {dict(plan)}"]
    if spec is not None:
        lines.append(f"case {spec}")
    if idx.numel():
        first = idx[:20000]
        recs = []
        for z in first[:, 0].unique().tolist()[:64]:
            sel = first[first[:, 0] == z]
            for r in locate.locate(sel[:, 1].tolist(), sel[:, 2].tolist(), plan, batch_index=z):
                r["batch"] = z
                recs.append(r)
        lines.append(f"rows {int(idx[:, 1].min())}..{int(idx[:, 1].max())}, cols {int(idx[:, 2].min())}..{int(idx[:, 2].max())}, "
                     f"first (batch, row, col) {idx[0].tolist()}")
        for k in ("batch", "tile", "wave", "strip_mt", "strip_nt", "row_in_strip", "slot", "round"):
            if k in recs[0]:
                lines.append(f"  by {k}: {dict(Counter(r[k] for r in recs).most_common(8))}")
    return "\n".join(lines)


def compare_exact(got, ref64, plan=None, spec=None):
    """`got` (fp32 or bf16 CPU tensor) must be the float64 reference bit for bit (fp32: the value itself — an integer
    below 2^24; bf16: its round-to-nearest-even)."""
    want = ref64.to(got.dtype)
    if got.dtype == torch.float32:
        assert bool((want.double() == ref64).all()), "the reference is not representable: operands are not exact"
    bad = bits_of(got) != bits_of(want)
    if bool(bad.any()):
        raise AssertionError("not the float64 product bit for bit: " + (failure_report(bad, plan, spec) if plan else
                                                                       f"{int(bad.sum())} wrong elements"))


def compare_bounded(got, ref64, bound, plan=None, spec=None, what="C"):
    """fp32 `got` within the element-wise bound; bf16 `got` the rounding of an fp32 value within it: the rounded reference
    itself in at least 99 % of the elements whose fp32 bound is at most 1/32 of a bf16 ulp (attn16_f64.bf16_stage)"""
    if got.dtype == torch.bfloat16:
        try:
            assert bool(torch.isfinite(got.float()).all()), "non-finite elements"
            assert_bf16_rounding_of(got, ref64, bound, count=bound * 32 <= bf16_ulp(ref64))
        except AssertionError as e:
            r = ref64.to(torch.bfloat16)
            bad = (got.double() - ref64).abs() > bound + 2.0 ** -7 * ref64.abs() + (r.double() - ref64).abs()
            raise AssertionError(f"{what}: {e}; " + (failure_report(bad, plan, spec) if plan else "")) from None
        return
    err = (got.double() - ref64).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = tuple(int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"{what}: outside the fp32 bound, first at {i}: got {float(got[i])!r}, ref {float(ref64[i])!r}, "
                             f"bound {float(bound[i]):.3e}; " + (failure_report(bad, plan, spec) if plan else ""))


# ------------------------------------------------------------------------------- a case: one launch, described once
# A case is a dict (the committed table, tests/golden/gemm_f64_cases.json, holds such dicts):
#   M, N, K, b0, b1, akc, bkc          the product and the operand layouts
#   dtype, a_st, b_st, c_st            matrix pipe and storage types
#   pipe, pipe32, det                  the calm_gemm_set_option settings it runs under
#   split_k                            calm_gemm_args.split_k (1: never split)
#   scalar                             operands laid out so that 16-byte staging is impossible
#   key                                the Key it must plan
CASE_DEFAULTS = dict(b0=1, b1=1, dtype=F32, a_st=ST_F32, b_st=ST_F32, c_st=ST_F32, pipe=1, pipe32=0, det=0, split_k=1,
                     scalar=0)


def full_case(c):
    out = dict(CASE_DEFAULTS)
    out.update(c)
    return out


def binding():
    return import_module("calm_vit_dte_amd._lib")


class options:
    """calm_gemm_set_option settings of a case, restored on exit (`lib`: the ctypes library, or a backend with
    gemm_set_option)"""

    def __init__(self, lib, case):
        self.set = lib.gemm_set_option if hasattr(lib, "gemm_set_option") else lib.calm_gemm_set_option
        self.want = ((OPT_PIPE, case["pipe"]), (OPT_PIPE32, case["pipe32"]), (OPT_DET, case["det"]))

    def __enter__(self):
        self.prev = []
        for o, v in self.want:
            self.prev.append((o, self.set(o, v)))
        return self

    def __exit__(self, *exc):
        for o, v in reversed(self.prev):
            self.set(o, v)
        return False


_FAKE = {"A": 0x7f0000000000, "B": 0x7f1000000000, "C": 0x7f2000000000, "x": 0x7f3000000000}


def c_batches(c):
    """batch extents of C: a reduce_batch launch sums every batch entry into one matrix"""
    return (1, 1) if c.get("reduce_batch") else (c["b0"], c["b1"])


POINTERS = ("A", "B", "C", "a_dq", "b_dq", "inv_scale", "bias", "col_scale", "residual", "aux", "C_pre")


def fake_args(case, epi=None, ptrs=None):
    """calm_gemm_args of a case, laid out exactly as `Launch` lays the real tensors out (fence_geometry / guard_geometry).
    ptrs None: fake, 256-byte aligned base addresses (calm_gemm_describe never reads them); else {name of POINTERS: the
    address of the tensor's first element} of real tensors.  epi: optional dict of epilogue settings {alpha, bias,
    col_scale, inv_scale, residual (storage type), aux (storage type), C_pre, act, accumulate, shift}.  Case fields
    beyond CASE_DEFAULTS: reduce_batch (C = sum over the batch), grouped (every b0 entry passed as a group pointer)."""
    b = binding()
    c = full_case(case)
    g = b.GemmArgs()
    M, N, K, b0, b1 = c["M"], c["N"], c["K"], c["b0"], c["b1"]
    epi = epi or {}
    shift = epi.get("shift", 0)
    cb = c_batches(c)
    oa, sa, _ = fence_geometry(M, K, b0, b1, c["akc"], c["a_st"], c["scalar"])
    ob, sb, _ = fence_geometry(N, K, b0, b1, c["bkc"], c["b_st"], c["scalar"])
    oc, sc, _ = guard_geometry(*cb, M, N, shift, c["c_st"])
    x = _FAKE["x"] + 0x1000
    at = (lambda name, fake: fake) if ptrs is None else (lambda name, fake: ptrs[name])
    g.A = at("A", _FAKE["A"] + oa * ESIZE[c["a_st"]])
    g.B = at("B", _FAKE["B"] + ob * ESIZE[c["b_st"]])
    g.C = at("C", _FAKE["C"] + oc * ESIZE[c["c_st"]])
    g.M, g.N, g.K, g.batch0, g.batch1 = M, N, K, b0, b1
    g.a_rs, g.a_cs, g.a_b0, g.a_b1 = sa
    g.b_rs, g.b_cs, g.b_b0, g.b_b1 = sb
    g.c_rs, g.c_b0, g.c_b1 = sc
    g.alpha = epi.get("alpha", 1.0)
    g.dtype, g.a_type, g.b_type, g.c_type = c["dtype"], c["a_st"], c["b_st"], c["c_st"]
    g.split_k = c["split_k"]
    g.reduce_batch = int(c.get("reduce_batch", 0))
    if c.get("grouped"):
        g.n_group = b0
        for i in range(b0):
            g.A_group[i] = g.A + i * sa[2] * ESIZE[c["a_st"]]
            g.B_group[i] = g.B + i * sb[2] * ESIZE[c["b_st"]]
            if not g.reduce_batch:
                g.C_group[i] = g.C + i * sc[1] * ESIZE[c["c_st"]]
    if c["a_st"] >= ST_E4M3:
        g.a_dq, g.b_dq = at("a_dq", _FAKE["x"] + 0x100), at("b_dq", _FAKE["x"] + 0x200)
    if epi.get("inv_scale"):
        g.inv_scale = at("inv_scale", x)
    if epi.get("bias"):
        g.bias = at("bias", x + 0x10000 + 4 * shift)
    if epi.get("col_scale"):
        g.col_scale = at("col_scale", x + 0x20000 + 4 * shift)
    for name, tname, far in (("residual", "r_type", 0x100000000), ("aux", "aux_type", 0x200000000)):
        if epi.get(name) is not None:
            st = epi[name]
            o, s, _ = guard_geometry(*cb, M, N, shift, st)
            setattr(g, name, at(name, x + far + o * ESIZE[st]))
            setattr(g, tname, st)
            if name == "residual":
                g.r_rs, g.r_b0, g.r_b1 = s
    if epi.get("C_pre"):
        g.C_pre = at("C_pre", x + 0x300000000 + oc * ESIZE[c["c_st"]])
    g.act = epi.get("act", ACT_NONE)
    g.accumulate = int(epi.get("accumulate", 0))
    return g


class Launch:
    """The real tensors of a case on the device and its calm_gemm_args: exact operands between fences, C (and C_pre) in
    guard bands, the epilogue operands of `epi` with the alignment fake_args gives the fake ones — asserted, so that what
    test_gemm_f64_cpu.py proves about a table entry holds for the launch.  poison: ("A" | "B", (i0, i1, row, k)) puts one
    NaN into an operand.  `ops`: the values the kernel reads (CPU, float64-ready), `acc`: the float64 product."""

    def __init__(self, case, epi=None, seed=1, poison=None):
        c = self.case = full_case(case)
        e = self.epi = dict(epi or {})
        M, N, K, b0, b1 = c["M"], c["N"], c["K"], c["b0"], c["b1"]
        A, B = exact_operand(b0, b1, M, K, seed), exact_operand(b0, b1, N, K, seed + 1)
        dev = lambda t: t.to(DEVICE)
        acc = product64(dev(A), dev(B))
        self.acc = (acc.sum(dim=(0, 1), keepdim=True) if c.get("reduce_batch") else acc).cpu()
        if poison:
            (A if poison[0] == "A" else B)[poison[1]] = float("nan")
        self.A = Fenced(A, c["akc"], c["a_st"], c["scalar"])
        self.B = Fenced(B, c["bkc"], c["b_st"], c["scalar"])
        cb, shift, cdt = c_batches(c), e.get("shift", 0), TORCH_ST[c["c_st"]]
        gen = torch.Generator().manual_seed(seed + 10)
        rn = lambda *s: torch.randn(*s, generator=gen)
        self.ops, self.keep = {}, []
        if "alpha" not in e and e.get("inv_scale"):
            e["alpha"] = float(torch.tensor(1.3 / (25.5 * K ** 0.5), dtype=torch.float32))     # v1 of order one
        if e.get("accumulate"):
            self.ops["c_old"] = (8 * rn(*cb, M, N)).round().to(cdt)      # integers: exact through atomics as well
        self.C = Guarded(*cb, M, N, shift, init=self.ops.get("c_old"), dtype=cdt)
        ptrs = {"A": self.A.view.data_ptr(), "B": self.B.view.data_ptr(), "C": self.C.view.data_ptr()}

        def vector(name, values, shift=shift):
            buf = torch.zeros(values.numel() + 8, device=DEVICE)
            buf[shift:shift + values.numel()] = dev(values)
            self.keep.append(buf)
            self.ops[name] = values
            ptrs[name] = buf[shift:].data_ptr()
        one = torch.ones(1, device=DEVICE)
        self.keep.append(one)
        ptrs["a_dq"] = ptrs["b_dq"] = one.data_ptr()
        if e.get("inv_scale"):
            vector("inv_scale", torch.tensor([1.3]), 0)
        if e.get("bias"):
            vector("bias", rn(N))
        if e.get("col_scale"):
            vector("col_scale", rn(N))
        for name, scale in (("residual", 1.0), ("aux", 1.5)):
            if e.get(name) is not None:
                v = (scale * rn(*cb, M, N)).to(TORCH_ST[e[name]])
                t = Guarded(*cb, M, N, shift, init=v, dtype=TORCH_ST[e[name]])
                self.keep.append(t)
                self.ops[name] = v
                ptrs[name] = t.view.data_ptr()
        self.C_pre = Guarded(*cb, M, N, shift, dtype=cdt) if e.get("C_pre") else None
        if self.C_pre is not None:
            ptrs["C_pre"] = self.C_pre.view.data_ptr()
        self.g = fake_args(c, e, ptrs)
        fake = fake_args(c, e)
        for name in POINTERS:
            real, f = getattr(self.g, name), getattr(fake, name)
            assert (real is None) == (f is None) and (real is None or real % 16 == f % 16), name

    def plan(self, lib):
        rc, plan = describe(lib, self.g)
        assert rc == 0, (rc, self.case)
        return instance_key(self.g, plan), plan

    def run(self, lib, workspace=True):
        """calm_gemm on torch's current stream, with the workspace the library asks for (workspace=False: none offered,
        so k-slices are combined with atomics)"""
        g = self.g
        need = lib.calm_gemm_workspace_bytes(ctypes.byref(g)) if workspace and g.split_k != 1 else 0
        if need > 0:
            ws = torch.empty(need // 4, dtype=torch.float32, device=DEVICE)
            self.keep.append(ws)
            g.workspace, g.workspace_bytes = ws.data_ptr(), need
        rc = lib.calm_gemm(ctypes.byref(g), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, (rc, self.case)
        torch.cuda.synchronize()

    def reference(self):
        """epilogue_reference of this launch from the exact accumulator"""
        o = self.ops
        return epilogue_reference(self.acc, self.epi.get("alpha", 1.0), o.get("inv_scale"), o.get("bias"), self.epi.get("act", ACT_NONE),
                                  o.get("aux"), o.get("col_scale"), o.get("residual"), o.get("c_old"))


def describe(lib, g):
    """calm_gemm_describe -> (rc, plan dict)"""
    b = binding()
    plan = b.GemmPlan()
    rc = lib.calm_gemm_describe(ctypes.byref(g), ctypes.byref(plan))
    return rc, {n: getattr(plan, n) for n, _ in b.GemmPlan._fields_}


def macs(c):
    return c["M"] * c["N"] * c["K"] * c.get("b0", 1) * c.get("b1", 1)


# ------------------------------------------------------------------------------------------------- the case tables
_TABLE = None


def instance_cases():
    """tests/golden/gemm_f64_cases.json: one case per CENSUS entry, written by scripts/gemm_instance_sweep.py"""
    global _TABLE
    if _TABLE is None:
        import json
        import os
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_f64_cases.json")) as f:
            _TABLE = [full_case(c) for c in json.load(f)]
    return _TABLE


def table_case(kernel):
    for c in instance_cases():
        if tuple(c["key"][:-1]) == tuple(kernel):
            return c
    raise KeyError(kernel)


def case_id(c):
    k = c["key"]
    return "f%d-%dx%d-%s%s-st%d-a%db%d-p%d" % (k[0], k[1], k[2], "k" if k[3] else "m", "k" if k[4] else "m", k[5], k[6], k[7], k[8])


# Epilogue variants: each C-shaped epilogue operand on its own (plan_pipe takes at most one), alpha / inv_scale and bias
# throughout.  The values of `aux` / `residual` are storage types, filled in per storage variant.
EPI_VARIANTS = {
    "gelu_pre": dict(inv_scale=1, bias=1, act=ACT_GELU, C_pre=1),
    "gelu_bwd": dict(inv_scale=1, bias=1, act=ACT_GELU_BWD, aux=ST_F32),
    "scale_res": dict(inv_scale=1, bias=1, col_scale=1, residual=ST_F32),
    "accumulate": dict(inv_scale=1, bias=1, accumulate=1),
}
# (kernel of the instance table the launch is built on, storage variants, misaligned one-element fallback as well)
#   "f32": C / C_pre / aux / residual fp32     "bf16": all of them bf16     "mixed": C bf16, residual fp32 (scale_res only)
EPI_BASES = [
    ((0, 128, 128, 1, 0, 16, 0, 0, 1), ("f32",), True),
    ((0, 64, 80, 0, 0, 16, 0, 0, 1), ("f32",), True),
    ((1, 128, 128, 1, 1, 16, 1, 1, 1), ("f32", "bf16", "mixed"), True),
    ((1, 128, 96, 0, 0, 16, 0, 0, 3), ("f32",), False),
    ((2, 256, 128, 1, 0, 16, 1, 1, 1), ("f32", "bf16", "mixed"), True),
    ((3, 128, 160, 1, 1, 16, 1, 1, 1), ("f32", "bf16", "mixed"), False),
    ((3, 192, 128, 1, 0, 16, 1, 1, 1), ("f32", "bf16", "mixed"), False),
    ((3, 128, 224, 0, 0, 16, 1, 1, 1), ("f32", "bf16", "mixed"), False),
    ((4, 128, 128, 1, 1, 16, 0, 0, 1), ("f32",), False),
    ((4, 128, 160, 1, 0, 16, 0, 0, 1), ("f32",), False),
    ((4, 192, 128, 0, 0, 16, 0, 0, 1), ("f32",), False),
    ((5, 256, 128, 1, 1, 16, ST_E5M2, ST_E4M3, 1), ("f32", "bf16"), True),
]


def epilogue_cases():
    """[(id, case, epi dict, expected family, expected epilogue form)]"""
    out = []
    for kernel, storages, misaligned in EPI_BASES:
        base = table_case(kernel)
        fam = kernel[0]
        for stv in storages:
            for name, epi in EPI_VARIANTS.items():
                if stv == "mixed" and name != "scale_res":
                    continue
                c = dict(base, c_st=ST_F32 if stv == "f32" else ST_BF16)
                e = dict(epi)
                for t in ("aux", "residual"):
                    if t in e:
                        e[t] = ST_BF16 if stv == "bf16" else ST_F32
                form = (8 if stv == "bf16" and c["N"] % 8 == 0 else 4) if fam in (3, 4) else 4
                out.append(("f%d-%dx%d-%s-%s" % (kernel[0], kernel[1], kernel[2], stv, name), c, e, fam, form))
        if misaligned:
            for name in ("gelu_bwd", "scale_res"):
                out.append(("f%d-%dx%d-unaligned-%s" % (kernel[0], kernel[1], kernel[2], name), dict(base, c_st=ST_F32),
                            dict(EPI_VARIANTS[name], shift=1), fam, 1))
    return out


# k-split launches, one per family that splits (weight-gradient layout: both operands row-contiguous, or k-contiguous
# for variety): (id, case, expected family).  K has a tail against the k-tile; split_k = 0 lets plan_gemm decide, as the
# training step does.  Each runs with atomics, in deterministic mode (workspace + fixed-order reduction, twice) and
# accumulating; `shift` = 1 puts C off 16-byte alignment (splitk_reduce instead of splitk_reduce_vec).
SPLIT_CASES = [
    ("f0-128", dict(M=328, N=312, K=12292, akc=0, bkc=0, split_k=0), 0),     # 49 slices of a 102336-element output: the
                                                                                # workspace plan keeps the 128-row tile
    ("f0-64", dict(M=200, N=120, K=4100, akc=0, bkc=0, split_k=0), 0),
    ("f0-64-kk", dict(M=85, N=72, K=2052, akc=1, bkc=1, split_k=0), 0),
    ("f1", dict(M=264, N=200, K=4100, akc=0, bkc=0, split_k=0, dtype=BF16), 1),
    ("f1-x3", dict(M=136, N=104, K=2052, akc=1, bkc=0, split_k=0, dtype=BF16X3), 1),
    ("f2", dict(M=680, N=264, K=4104, akc=0, bkc=0, split_k=0, dtype=BF16, a_st=ST_BF16, b_st=ST_BF16, pipe=0), 2),
    ("f3", dict(M=264, N=488, K=4104, akc=0, bkc=0, split_k=0, dtype=BF16, a_st=ST_BF16, b_st=ST_BF16), 3),
    ("f3-kk", dict(M=213, N=232, K=2056, akc=1, bkc=1, split_k=3, dtype=BF16, a_st=ST_BF16, b_st=ST_BF16), 3),
    ("f4", dict(M=264, N=200, K=2052, akc=0, bkc=0, split_k=0, pipe32=1), 4),
]


def split_launches():
    """[(id, case, epi, family, workspace)]: every SPLIT_CASES entry in every way its k-slices can be combined.
      atomics               fp32 atomics onto a zeroed C (no workspace offered)
      atomics-accumulate    ... onto the old C
      workspace             deterministic option: per-slice partials + splitk_reduce_vec; run twice, bit-equal
      workspace-accumulate  ... adding the old C
      workspace-unaligned   C one element off 16-byte alignment: the one-element splitk_reduce, accumulating
    The pipelined families take 16-byte aligned epilogue tensors only (plan_pipe: `!p.epi_vec` declines), so the
    unaligned form is generated for the others."""
    modes = (("atomics", 0, {}, False), ("atomics-accumulate", 0, dict(accumulate=1), False), ("workspace", 1, {}, True),
             ("workspace-accumulate", 1, dict(accumulate=1), True), ("workspace-unaligned", 1, dict(accumulate=1, shift=1), True))
    out = []
    for name, c, family in SPLIT_CASES:
        for mode, det, epi, ws in modes:
            if epi.get("shift") and family in (3, 4):
                continue
            out.append((f"{name}-{mode}", dict(c, det=det), dict(epi), family, ws))
    return out


# Launches over groups and over a summed batch: (id, case, expected family, k-slices combined).  reduce_batch sums every
# batch entry into one C with atomics over the concatenated reduction; `grouped` passes every b0 entry as a group
# pointer: weight gradients k-split per group (split_k = 0), or, with reduce_batch and no split, one pass over the
# concatenated reduction with a plain epilogue.
GROUP_CASES = [
    ("f0-reduce_batch", dict(M=85, N=232, K=132, b0=16, akc=1, bkc=1, reduce_batch=1, split_k=0), 0, True),
    ("f1-reduce_batch", dict(M=136, N=200, K=132, b0=16, akc=1, bkc=1, reduce_batch=1, split_k=0, dtype=BF16), 1, True),
    ("f0-grouped-split", dict(M=200, N=120, K=4100, b0=3, akc=0, bkc=0, grouped=1, split_k=0), 0, True),
    ("f1-grouped-split", dict(M=136, N=200, K=4100, b0=3, akc=0, bkc=0, grouped=1, split_k=0, dtype=BF16), 1, True),
    ("f1-bf16-grouped-split", dict(M=264, N=232, K=4104, b0=3, akc=0, bkc=0, grouped=1, split_k=0, dtype=BF16, a_st=ST_BF16,
                                   b_st=ST_BF16), 1, True),
    ("f3-grouped-split", dict(M=264, N=488, K=4104, b0=3, akc=0, bkc=0, grouped=1, split_k=0, dtype=BF16, a_st=ST_BF16,
                              b_st=ST_BF16), 3, True),
    ("f4-grouped-split", dict(M=264, N=488, K=4100, b0=3, akc=0, bkc=0, grouped=1, split_k=0, pipe32=1), 4, True),
    ("f0-grouped-reduce", dict(M=213, N=120, K=132, b0=3, akc=1, bkc=0, grouped=1, reduce_batch=1, split_k=1), 0, False),
    ("f1-grouped-reduce", dict(M=213, N=200, K=132, b0=3, akc=1, bkc=0, grouped=1, reduce_batch=1, split_k=1, dtype=BF16), 1, False),
]

# one instance of the table per family (both fp32 tile heights) for the NaN propagation test
NAN_KERNELS = [base for base, _, _ in EPI_BASES if base[:3] in ((0, 128, 128), (0, 64, 80), (1, 128, 128), (2, 256, 128),
                                                                (3, 128, 160), (4, 128, 128), (5, 256, 128))]
