"""Float64 references, element-wise bounds, replicated host formulas and case tables for the RoPE kernels
(csrc/norm_act.hip: the table kernel, calm_rope_fwd, calm_rope_bwd, calm_part_rope_bwd) and the spectral-norm kernels
(csrc/spectral.hip: calm_sn_plan / calm_sn_power_iter, calm_sn_weight_bwd, calm_sn_weight_bwd_batch).

The module imports only torch and knows nothing about who produced the tensors it checks: the GPU tests
(test_rope_sn_f64_gpu.py) hand it the kernels' outputs, the CPU tests (test_rope_sn_f64_cpu.py) an fp32 emulation's and
planted faults.  Every checker takes CPU tensors and returns (worst, failures): worst[name] = max error / bound of an
output, failures = a list of (name, message); strict=True raises on a non-empty list.

The references are staged as in attn16_f64.py: a stage is referenced from the checked implementation's OWN output of the
stage before it (the table -> the rotation; t -> v -> s -> u -> sigma), so each bound is a pure fp32-rounding bound:

    U = 2^-24     unit roundoff of fp32: one operation errs by at most U |result|
    sums          a sum of serial depth d of terms whose absolute values sum to A errs by at most d U A (first order);
                  the depths come from the host launch formulas replicated below, with the source line named
    bf16          one round-to-nearest-even of the fp32 result (attn16_f64.assert_bf16_rounding_of)

The one bound that is not derived is the table's: it is the accuracy of the device's cosf / sinf, which the ROCm tree
documents nowhere (it ships OCML as bitcode only), so it was measured once: TABLE_ERR below, asserted at twice that.
"""
import math

import torch

from attn16_f64 import FILL, _Report, assert_bf16_rounding_of  # noqa: F401  (FILL re-exported for the tests)

U = 2.0 ** -24
F32, BF16 = torch.float32, torch.bfloat16

# rope_table_kernel against float64 cos / sin of the fp32 angle fl32(float(s) * inv_freq[j]), measured once on an MI355X
# over 3 x 2^20 (s, j) pairs with angles in [0, 512] rad (the figures by angle range: docstring of
# test_rope_sn_f64_gpu.py).  The largest absolute error of either function (1.53 ulp of the result; no growth with the
# angle):
TABLE_ERR = 7.03e-8


def cdiv(a, b):
    return -(-a // b)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def partials_depth(G):
    """calm_reduce_partials (common.h): ceil(G/64) adds into each of four running sums, three pairwise levels over the
    sums and the sixteen row lanes, and the add onto the output: ceil(G/64) + 7."""
    return cdiv(G, 64) + 7


class Report(_Report):
    def bounded(self, name, got, ref64, bound):
        super().bounded(name, got, ref64, bound)
        if not math.isfinite(self.worst[name]) and bool((got.double() == ref64).all()):
            self.worst[name] = 0.0                           # 0 / 0 everywhere (a zero weight): no error, not inf

    def exact(self, name, got, want):
        """bit for bit (no NaN on either side is expected: a NaN in got fails)"""
        if got.dtype != want.dtype or got.shape != want.shape:
            self.fail(name, f"{got.dtype} {tuple(got.shape)} where {want.dtype} {tuple(want.shape)} is expected")
            return
        bits = lambda t: t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)
        bad = bits(got) != bits(want)
        self.worst[name] = float(bad.sum())
        if bool(bad.any()):
            idx = tuple(int(i) for i in bad.nonzero()[0])
            self.fail(name, f"{int(bad.sum())} elements differ, first at {idx}: got {float(got[idx])!r}, "
                            f"want {float(want[idx])!r}")

    def equal64(self, name, got, want64):
        """got (any type) equals the float64 values exactly"""
        bad = ~(got.double() == want64)
        self.worst[name] = float(bad.sum())
        if bool(bad.any()):
            idx = tuple(int(i) for i in bad.nonzero()[0])
            self.fail(name, f"{int(bad.sum())} elements differ, first at {idx}: got {float(got[idx])!r}, "
                            f"want {float(want64[idx])!r}")

    def bf16(self, name, got, ref64, fp32_bound):
        """one RNE rounding of an fp32 result within fp32_bound of ref64: assert_bf16_rounding_of with its 0.99 share"""
        try:
            assert_bf16_rounding_of(got, ref64, fp32_bound)
        except AssertionError as e:
            self.fail(name, str(e))
        ratio = (got.double() - ref64).abs() / (fp32_bound + 2.0 ** -8 * ref64.abs())
        fin = torch.isfinite(ratio)
        self.worst[name] = float(ratio[fin].max()) if bool(fin.any()) else 0.0

    def typed(self, name, got, ref64, bound):
        if got.dtype == BF16:
            self.bf16(name, got, ref64, bound)
        else:
            self.bounded(name, got, ref64, bound)

    def merge(self, other, prefix=""):
        for k, v in other.worst.items():
            self.worst[k] = max(self.worst.get(k, 0.0), v)
        self.failures += [(n, prefix + m) for n, m in other.failures]


# ====================================================================================================== RoPE: host
NT = 256                       # norm_act.hip NT: threads of a RoPE workgroup
ROPE_MAX_HALF = 256            # norm_act.hip ROPE_MAX_HALF
ROPE_VEC_MAX_GRID = 256 * 16   # norm_act.hip ROPE_VEC_MAX_GRID
ROPE_BWD_GRID = 1024           # norm_act.hip CALM_ROPE_BWD_GRID
ROPE_BWD_MAX_GRID = 2048       # common.h ROPE_BWD_MAX_GRID
ROPE_SCRATCH_ROWS = 4096       # common.h ROPE_SCRATCH_ROWS (calm_reduce_scratch_floats: this many rows of dr/2 partials)


def rope_half(dr):
    """rope_plan: `const int half = dr / 2`"""
    return dr // 2


def rope_vw_shape(dc, dr):
    """rope_plan: `p.vw = ((dc & 3) == 0 && (half & 3) == 0 && CALM_ROPE_VW4) ? 4 : ((dc & 1) == 0 && (half & 1) == 0)
    ? 2 : 1` — the widest column group that does not straddle the content / half boundaries"""
    half = rope_half(dr)
    return 4 if dc % 4 == 0 and half % 4 == 0 else 2 if dc % 2 == 0 and half % 2 == 0 else 1


def rope_vw(dc, dr, tensors=()):
    """rope_plan's vw for a call: rope_vw_shape lowered by the loop over vec_tensors, `while (p.vw > 1 && (address &
    (p.vw * bytes - 1)) != 0) p.vw >>= 1`.  tensors: (address, element size in bytes) of every tensor the kernels access
    as vectors; fp32 needs 16 bytes for vw = 4 and 8 for vw = 2, bf16 8 and 4."""
    vw = rope_vw_shape(dc, dr)
    for addr, esize in tensors:
        while vw > 1 and addr % (vw * esize) != 0:
            vw //= 2
    return vw


def rope_fits(B, S, H, dc, dr):
    """rope_plan: `p.fits = half <= ROPE_MAX_HALF && half <= NT && p.nrows * (dc + dr) < (1L << 31)`"""
    half = rope_half(dr)
    return half <= ROPE_MAX_HALF and half <= NT and B * S * H * (dc + dr) < (1 << 31)


def rope_ir(dr, vw):
    """rope_fwd_vec_kernel / rope_bwd_vec_kernel: `ir = half / VW`, the threads that serve a row"""
    return rope_half(dr) // vw


def rope_rpb(dr, vw):
    """rope_plan: `const int rpb = NT / (half / p.vw)`, the rows of a workgroup pass (NT % ir threads stay idle)"""
    return NT // rope_ir(dr, vw)


def rope_grid(nrows, dr, vw):
    """rope_plan: `p.grid = min(ROPE_VEC_MAX_GRID, ceil(nrows / rpb))`"""
    return min(ROPE_VEC_MAX_GRID, cdiv(nrows, rope_rpb(dr, vw)))


def rope_bwd_grid(nrows, dr, vw):
    """rope_plan: `want = p.grid / 16; p.bwd_grid = want < CALM_ROPE_BWD_GRID ? min(p.grid, CALM_ROPE_BWD_GRID)
    : min(want, ROPE_BWD_MAX_GRID)`.
    The second branch is unreachable with the constants as they are: grid <= ROPE_VEC_MAX_GRID = 4096, so
    want <= 256 < CALM_ROPE_BWD_GRID = 1024 (asserted below and in test_rope_sn_f64_cpu.py); it is replicated as written."""
    grid = rope_grid(nrows, dr, vw)
    want = grid // 16
    if want < ROPE_BWD_GRID:
        return min(grid, ROPE_BWD_GRID)
    return min(want, ROPE_BWD_MAX_GRID)


assert ROPE_VEC_MAX_GRID // 16 < ROPE_BWD_GRID        # the `want` branch of bwd_grid cannot be taken


def rope_dif_depth(nrows, dr, vw):
    """Serial depth of a d_inv_freq element: a row lane's rows (rope_bwd_vec_kernel's row loop, stride bwd_grid * rpb),
    the block's rpb row lanes added in order (the loop over facc), then calm_reduce_partials over bwd_grid rows."""
    g, rpb = rope_bwd_grid(nrows, dr, vw), rope_rpb(dr, vw)
    return cdiv(nrows, g * rpb) + rpb + partials_depth(g)


# ==================================================================================================== RoPE: cases
ROPE_TYPES = {"f32": (F32, F32), "bf16": (BF16, BF16), "in16": (BF16, F32), "out16": (F32, BF16)}
# (content / xr / d_content / d_xr type, out / d_out type): all fp32 (TT = F32), all bf16 (TT = BF16), and the mixed
# combinations of the model (TT = -1): bf16 in -> fp32 out, fp32 in -> bf16 out; the backward of "out16" is the bf16
# d_out with fp32 d_xr


def rope_case(B, S, H, dc, dr, types="f32", note=""):
    return dict(B=B, S=S, H=H, dc=dc, dr=dr, types=types, note=note)


def rope_id(c):
    return "B{B}-S{S}-H{H}-dc{dc}-dr{dr}-{types}".format(**c)


ROPE_CASES = [
    # B, S, H, dc, dr                        vw, ir = half / vw, rpb, what it reaches
    rope_case(3, 11, 5, 32, 32, note="vw 4, ir 4, rpb 64: no idle threads, 3 workgroups"),
    rope_case(3, 11, 5, 8, 48, note="vw 4, ir 6, rpb 42: 4 idle threads"),
    rope_case(3, 11, 5, 4, 40, note="vw 4, ir 5, rpb 51: 1 idle thread"),
    rope_case(3, 11, 5, 6, 12, note="vw 2, ir 3, rpb 85: 1 idle thread"),
    rope_case(3, 11, 5, 18, 18, note="vw 1 (half 9), ir 9, rpb 28: 4 idle threads"),
    rope_case(3, 11, 5, 10, 20, note="vw 2, ir 5, rpb 51"),
    rope_case(3, 11, 5, 5, 6, note="vw 1 (dc odd), ir 3, rpb 85"),
    rope_case(3, 11, 5, 0, 32, note="dc 0, vw 4: content and d_content are None"),
    rope_case(3, 11, 5, 0, 6, note="dc 0, vw 1"),
    rope_case(2, 7, 3, 4, 512, note="half 256, vw 4, ir 64, rpb 4: 11 workgroups"),
    rope_case(2, 7, 3, 3, 512, note="half 256, vw 1, ir 256, rpb 1: every thread owns one pair"),
    rope_case(3, 11, 5, 0, 2, note="dr 2: half 1, rpb 256"),
    rope_case(3, 11, 5, 3, 2, note="dr 2 with content"),
    rope_case(5, 33, 29, 1, 512, note="4785 rows at rpb 1 > 4096: two forward passes (stride 4096, H and S odd: "
                                      "advance() carries), five backward passes of 1024 workgroups"),
    rope_case(3, 53, 53, 4, 256, note="half 128, vw 4, rpb 8, 8427 rows: 1054 workgroups forward, bwd_grid 1024 with a "
                                      "second pass (stride 8192)"),
    # types, on a vw = 4 and a vw = 1 shape
    rope_case(3, 11, 5, 8, 48, "bf16"), rope_case(3, 11, 5, 8, 48, "in16"), rope_case(3, 11, 5, 8, 48, "out16"),
    rope_case(3, 11, 5, 5, 6, "bf16"), rope_case(3, 11, 5, 5, 6, "in16"), rope_case(3, 11, 5, 5, 6, "out16"),
    rope_case(5, 33, 29, 1, 512, "bf16", note="the passes of a capped grid on bf16 tensors"),
]
ROPE_FALLBACK = rope_case(2, 5, 3, 3, 516, note="half 258 > 256: one-element forward; the backward refuses")
ROPE_ALIGN_SHAPE = dict(B=3, S=11, H=5, dc=8, dr=48)          # vw = 4 when every tensor is aligned
ROPE_ALIGN_FWD = ("content", "xr", "out", "table")
ROPE_ALIGN_BWD = ("d_out", "d_content", "d_xr", "table", "xr")


def rope_inputs(case, seed=0, exact=False):
    """content, xr, inv_freq, g (= d_out), d0 (the incoming d_inv_freq, non-zero).  exact: inv_freq = 0 (the table is
    exactly c = 1, sn = 0) and small integers, so that every result is an integer below 2^24, exact in any order."""
    B, S, H, dc, dr = (case[k] for k in ("B", "S", "H", "dc", "dr"))
    tin, tout = ROPE_TYPES[case["types"]]
    half, nrows = dr // 2, B * S * H
    g = gen(1000 * seed + 31 * dc + dr + nrows)
    if exact:
        hi = next(h for h in (8, 4, 2, 1) if nrows * S * 2 * h * h + 8 < (1 << 24))   # |sum s (g2 x1 - g1 x2)| < 2^24
        ints = lambda *s: torch.randint(-hi, hi + 1, s, generator=g).float()
        content, xr, dout = ints(B, S, H * dc), ints(B, S, H * dr), ints(B, S, H * (dc + dr))
        inv, d0 = torch.zeros(half), torch.randint(-8, 9, (half,), generator=g).float()
    else:
        rn = lambda *s: torch.randn(*s, generator=g)
        content, xr, dout = rn(B, S, H * dc), rn(B, S, H * dr), rn(B, S, H * (dc + dr))
        inv, d0 = torch.rand(half, generator=g) + 0.01, rn(half)
    return dict(content=content.to(tin) if dc else None, xr=xr.to(tin), inv_freq=inv, g=dout.to(tout), d0=d0)


# =============================================================================================== RoPE: references
def _rows(t, case, width):
    return t.double().reshape(case["B"], case["S"], case["H"], width)


def table_reference(inv_freq, S):
    """float64 cos / sin of the fp32 product fl32(float(s) * inv_freq[j]) (formed in fp32, then widened) -> [2, S, half]"""
    ang = (torch.arange(S, dtype=torch.float32)[:, None] * inv_freq.float()[None, :]).double()
    return torch.stack([ang.cos(), ang.sin()])


def check_rope_forward(case, ins, got, strict=True, exact=False):
    """got: table [2, S, half] and out [B, S, H (dc + dr)]"""
    B, S, H, dc, dr = (case[k] for k in ("B", "S", "H", "dc", "dr"))
    half = dr // 2
    rep = Report()
    table = got["table"].reshape(2, S, half)
    tref = table_reference(ins["inv_freq"], S)
    if exact:
        rep.equal64("table", table, tref)                    # cosf(0) = 1, sinf(0) = 0
    else:
        rep.bounded("table", table, tref, torch.full_like(tref, 2 * TABLE_ERR))
    out = got["out"].reshape(B, S, H, dc + dr)
    if dc:
        # fp32 -> fp32 and bf16 -> bf16 copies, bf16 -> fp32 exact widening, fp32 -> bf16 RNE: torch's .to() is each
        rep.exact("out:content", out[..., :dc], ins["content"].reshape(B, S, H, dc).to(out.dtype))
    x = _rows(ins["xr"], case, dr)
    x1, x2 = x[..., :half], x[..., half:]
    c, sn = table[0].double()[None, :, None, :], table[1].double()[None, :, None, :]      # the kernel's own table
    ref = torch.cat([x1 * c - x2 * sn, x2 * c + x1 * sn], -1)
    # two products and a sum, with or without contraction: three roundings, each of at most the sum of the |products|
    bound = 3 * U * torch.cat([(x1 * c).abs() + (x2 * sn).abs(), (x2 * c).abs() + (x1 * sn).abs()], -1)
    if exact:
        rep.equal64("out:rot", out[..., dc:], ref)
    else:
        rep.typed("out:rot", out[..., dc:], ref, bound)
    return rep.done(strict)


def dif_reference(case, ins, table):
    """(d_inv_freq reference without d0, sum over rows of |terms|) from the given table [2, S, half] (float64)"""
    B, S, H, dc, dr = (case[k] for k in ("B", "S", "H", "dc", "dr"))
    half = dr // 2
    g, x = _rows(ins["g"], case, dc + dr), _rows(ins["xr"], case, dr)
    g1, g2, x1, x2 = g[..., dc:dc + half], g[..., dc + half:], x[..., :half], x[..., half:]
    c, sn = table[0].double()[None, :, None, :], table[1].double()[None, :, None, :]
    s = torch.arange(S, dtype=torch.float64)[None, :, None, None]
    terms = s * (g1 * (-x1 * sn - x2 * c) + g2 * (-x2 * sn + x1 * c))
    return terms.sum((0, 1, 2)), terms.abs().sum((0, 1, 2))


def check_rope_backward(case, ins, table, got, vw, strict=True, exact=False, d0=True):
    """got: d_xr, d_content (absent when dc = 0), and d_inv_freq (which started from ins["d0"]; d0=False: from zero) or
    part [G, half], the rows of partials of calm_part_rope_bwd.  table: the [2, S, half] table the backward was given;
    vw: the instance the host chose (rope_vw), for the summation depth."""
    B, S, H, dc, dr = (case[k] for k in ("B", "S", "H", "dc", "dr"))
    half, nrows = dr // 2, B * S * H
    rep = Report()
    g = _rows(ins["g"], case, dc + dr)
    g1, g2 = g[..., dc:dc + half], g[..., dc + half:]
    c, sn = table[0].double()[None, :, None, :], table[1].double()[None, :, None, :]
    if dc:
        rep.exact("d_content", got["d_content"].reshape(B, S, H, dc),
                  ins["g"].reshape(B, S, H, dc + dr)[..., :dc].to(got["d_content"].dtype))
    ref = torch.cat([g1 * c + g2 * sn, g2 * c - g1 * sn], -1)
    bound = 3 * U * torch.cat([(g1 * c).abs() + (g2 * sn).abs(), (g2 * c).abs() + (g1 * sn).abs()], -1)   # as the forward
    d_xr = got["d_xr"].reshape(B, S, H, dr)
    if exact:
        rep.equal64("d_xr", d_xr, ref)
    else:
        rep.typed("d_xr", d_xr, ref, bound)
    dif, absterms = dif_reference(case, ins, table)
    d0v = ins["d0"].double() if d0 else torch.zeros(half, dtype=torch.float64)
    # (depth + 8) U (sum |terms| + |d0|): depth serial additions (rope_dif_depth), 8 for the operations inside a term
    # (four products, the two inner sums, the outer sum, the product with s) and the add onto d0
    dbound = (rope_dif_depth(nrows, dr, vw) + 8) * U * (absterms + d0v.abs())
    if "part" in got:
        G = rope_bwd_grid(nrows, dr, vw)
        if tuple(got["part"].shape) != (G, half):
            rep.fail("part", f"shape {tuple(got['part'].shape)} where ({G}, {half}) is expected")
        elif exact:
            rep.equal64("part", got["part"].double().sum(0), dif)
        else:
            rep.bounded("part", got["part"].double().sum(0), dif, dbound)
    if "d_inv_freq" in got:
        if exact:
            rep.equal64("d_inv_freq", got["d_inv_freq"], dif + d0v)
        else:
            rep.bounded("d_inv_freq", got["d_inv_freq"], dif + d0v, dbound)
    return rep.done(strict)


# ============================================================================================ spectral norm: power
SN_EPS = 1e-12                  # backend.SN_EPS, handed to the kernels as a float
SN_EPS32 = float(torch.tensor(SN_EPS, dtype=torch.float32))
SN_LAYERS = [
    # rows, cols        phase A: clamped lanes when cols % 64 != 0, waves without a row when rows < 4, the r + 12 < rows
    #                   unroll edge per wave (rows 12, 13, 16, 17, 29); phase B: a short last SnWork (rows % 16 != 0);
    #                   cols > 256: more than one pass of the norm loop; rows 272 > 256: two passes in phase C
    (1, 1), (2, 3), (3, 9), (4, 63), (5, 64), (12, 65), (13, 130), (16, 672), (17, 1), (29, 3), (272, 672), (272, 9),
    (1, 672), (64, 64), (5, 130),
]
SN_SQUARE = 13                  # the square layer (the transposition faults)


def sn_offsets(layers):
    """calm_sn_plan: `L[i].t_off = off; off += cols; L[i].s_off = off; off += rows` -> ([(t_off, s_off)], scratch floats)"""
    offs, off = [], 0
    for rows, cols in layers:
        offs.append((off, off + cols))
        off += cols + rows
    return offs, off


def sn_work_counts(layers):
    """calm_sn_plan: (n_work, n_work_a) = sums of ceil(rows / ROWS_PER_WORK = 16) and ceil(cols / COLS_PER_WORK_A = 64)"""
    return sum(cdiv(r, 16) for r, _ in layers), sum(cdiv(c, 64) for _, c in layers)


def sn_inputs(layers, seed=0, zero=()):
    """[(W, u, v)] fp32: W ~ N(0, 1 / cols), u and v unit vectors; layers listed in `zero` get W = 0"""
    out = []
    for i, (rows, cols) in enumerate(layers):
        g = gen(100 * seed + i)
        W = torch.randn(rows, cols, generator=g) / math.sqrt(cols)
        if i in zero:
            W.zero_()
        u = torch.nn.functional.normalize(torch.randn(rows, generator=g), dim=0)
        v = torch.nn.functional.normalize(torch.randn(cols, generator=g), dim=0)
        out.append((W, u, v))
    return out


def norm_rel(n):
    """Relative error of x[i] * (1 / max(sqrt(sum_n x^2), eps)) against float64 on the same x, in units of U.  The sum
    of squares: a square (1), a thread's ceil(n / 256) serial additions, block_sum_256's six shuffle levels and three
    adds of the wave sums -> (ceil(n / 256) + 10) U relative (all terms positive); the square root halves that and adds
    its own rounding, the reciprocal one, the product one; + 1 for second-order terms."""
    return (cdiv(n, 256) + 10) / 2 + 3 + 1


def check_sn_layer(W, u_in, v_in, got, training, strict=True):
    """One layer of one calm_sn_power_iter.  got: t (training), s, u, v, sigma as the kernels left them."""
    rows, cols = W.shape
    W64 = W.double()
    rep = Report()
    if not training:
        # u, v bit-unchanged; s = W v with inv = 1 (v * 1.0f is exact); sigma = u . s
        rep.exact("u", got["u"], u_in)
        rep.exact("v", got["v"], v_in)
        v64, u64 = v_in.double(), u_in.double()
    else:
        # 1. t = W^T u: a wave's fma chain over its ceil(rows / 16) rows per running sum, (s0 + s1) + (s2 + s3) and the
        # tail loop's rows on s0 (+ 1 + 4 covers both), the four waves, 8 for the products
        t64 = got["t"].double()
        terms = (W64.abs() * u_in.double().abs()[:, None]).sum(0)
        rep.bounded("t", got["t"], W64.t() @ u_in.double(), (cdiv(rows, 16) + 1 + 4 + 8) * U * terms)
        # 2. v = t / max(|t|, eps) on the kernel's own t
        vref = t64 / max(float(t64.norm()), SN_EPS32)
        rep.bounded("v", got["v"], vref, norm_rel(cols) * U * vref.abs())
        v64 = got["v"].double()          # = t[c] * inv as phase B forms it for the products below (the same expression)
    # 3. s = W v: a lane's ceil(cols / 64) serial multiply-adds, six shuffle levels; + 2 for the products
    sterms = (W64.abs() * v64.abs()[None, :]).sum(1)
    sbound = (cdiv(cols, 64) + 8) * U * sterms
    rep.bounded("s", got["s"], W64 @ v64, sbound)
    s64 = got["s"].double()
    if training:
        # 4. u = s / max(|s|, eps) on the kernel's own s
        uref = s64 / max(float(s64.norm()), SN_EPS32)
        rep.bounded("u", got["u"], uref, norm_rel(rows) * U * uref.abs())
        u64 = got["u"].double()
    # 5. sigma = u . s: a product, a thread's ceil(rows / 256) additions, block_sum_256 (6 + 3)
    sg_terms = (u64 * s64).abs().sum()
    rep.bounded("sigma", got["sigma"].reshape(()), (u64 * s64).sum(), (cdiv(rows, 256) + 10) * U * sg_terms)
    if not training:
        # and against u . (W v) in float64 without the kernel's s: stage 3's bound carried by |u|
        bound = (cdiv(rows, 256) + 10) * U * sg_terms + (u64.abs() * sbound).sum()
        rep.bounded("sigma:uWv", got["sigma"].reshape(()), u64 @ (W64 @ v64), bound)
    return rep.done(strict)


def check_sn_iter(ins, got, training, strict=True):
    """All layers of a plan.  ins: [(W, u_in, v_in)], got: [dict] per layer."""
    rep = Report()
    for i, ((W, u, v), g) in enumerate(zip(ins, got)):
        r = Report()
        r.worst, r.failures = check_sn_layer(W, u, v, g, training, strict=False)
        rep.merge(r, prefix=f"layer {i} {tuple(W.shape)}: ")
    return rep.done(strict)


def sn_spectrum_layer(rows, cols, seed=0):
    """W = Uo diag(2, 1, 0.5, ...) Vo^T from float64 orthonormal factors, rounded to fp32 -> (W, Uo[:, 0], Vo[:, 0])"""
    g = gen(seed)
    k = min(rows, cols)
    Uo, _ = torch.linalg.qr(torch.randn(rows, k, generator=g, dtype=torch.float64))
    Vo, _ = torch.linalg.qr(torch.randn(cols, k, generator=g, dtype=torch.float64))
    sv = 2.0 ** (1 - torch.arange(k, dtype=torch.float64))
    return (Uo * sv) @ Vo.t(), Uo[:, 0], Vo[:, 0]


def check_sn_converged(W64, u1, v1, got, strict=True):
    """After 20 training iterations on fl32(W64) (singular values 2, 1, 0.5, ...; contraction (1/2)^40): sigma = 2 and
    |u . u1| = |v . v1| = 1 within the float64 sum of the last iteration's stage bounds.
    With dW = fl32(W) - W (|dW| <= U |W| element-wise, so |dW|_2 <= U |W|_F), bt / bs the 2-norms of stage 1's / stage
    3's bounds: the computed sigma is u . s_got within stage 5's bound, s_got = W v within bs, and u^T W v = |W v| =
    2 |v| up to second order in the angle d between v and v1.  |v| = 1 within norm_rel(cols) U.  d is the fixed point of
    d' = d / 2 + (per-iteration perturbation <= (bt + bs) / 2 + |dW|_2 / gap), gap = 1: d <= 2 x that, and d^2 (1e-11)
    is what the vectors' projections lose."""
    rows, cols = W64.shape
    W = W64.float().double()
    rep = Report()
    u, v = got["u"].double(), got["v"].double()
    dW = U * float(W.norm())
    bt = float(((cdiv(rows, 16) + 13) * U * (W.abs() * u.abs()[:, None]).sum(0)).norm())
    bs = float(((cdiv(cols, 64) + 8) * U * (W.abs() * v.abs()[None, :]).sum(1)).norm())
    b5 = (cdiv(rows, 256) + 10) * U * 2.0
    d = 2 * ((bt + bs) / 2 + dW)
    one = torch.ones((), dtype=torch.float64)
    rep.bounded("sigma", got["sigma"].reshape(()), 2 * one, (b5 + bs + 2 * norm_rel(cols) * U + dW + 2 * d * d) * one)
    rep.bounded("u.u1", (u @ u1).abs(), one, (norm_rel(rows) * U + d * d) * one)
    rep.bounded("v.v1", (v @ v1).abs(), one, (norm_rel(cols) * U + d * d) * one)
    return rep.done(strict)


# =========================================================================================== spectral norm: weight
SN_BATCH_MAX = 32               # calm_sn_bwd_batch_max()
SN_APPLY_ELEMS = 4096           # spectral.hip: sn_apply_rows_per_block switches to one row per workgroup at this many columns


def snw_case(rows, cols, ls=True, d_ls=True, note=""):
    return dict(rows=rows, cols=cols, ls=ls, d_ls=d_ls, note=note)


def snw_id(c):
    return "r{rows}-c{cols}-ls{ls:d}-dls{d_ls:d}".format(**c)


SNW_CASES = [
    snw_case(1, 1), snw_case(3, 63, ls=False, d_ls=False), snw_case(4, 64), snw_case(5, 65, d_ls=False),
    snw_case(144, 1000), snw_case(144, 144, note="square"), snw_case(3, 1, ls=False),
    snw_case(4100, 8, note="row-dot grid capped at 1024 workgroups of four waves: two passes"),
    snw_case(3, 4096, note="batched apply: one row per workgroup from 4096 columns"),
    snw_case(5, 4100, ls=False), snw_case(4, 4100), snw_case(2, 4095, note="batched apply: one row per workgroup below"),
    snw_case(1100, 1000, note="rows cols > 1024 * 256 * 4: the single form's apply grid-stride runs a second pass"),
]
SNW_BATCH = [SNW_CASES[i % 12] for i in range(35)]            # 35 > 32 entries: two chunks; every case but the largest


def sn_apply_rows_per_block(cols):
    """spectral.hip: `cols >= SN_APPLY_ELEMS ? 1 : SN_APPLY_ELEMS / cols`"""
    return 1 if cols >= SN_APPLY_ELEMS else SN_APPLY_ELEMS // cols


def snw_inputs(case, seed=0):
    rows, cols = case["rows"], case["cols"]
    g = gen(10 * seed + rows + 7 * cols)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(G=rn(rows, cols), W=rn(rows, cols), u=torch.nn.functional.normalize(rn(rows), dim=0),
                v=torch.nn.functional.normalize(rn(cols), dim=0), sigma=torch.tensor([1.3]),
                ls=(1 + 0.1 * rn(rows)) if case["ls"] else None)


def snw_reference(ins):
    """The kernel's stated formula in float64 -> dict(rowdot, dot, dW)"""
    G, W, u, v = (ins[k].double() for k in ("G", "W", "u", "v"))
    sigma = float(ins["sigma"].double())
    ls = torch.ones(G.shape[0], dtype=torch.float64) if ins["ls"] is None else ins["ls"].double()
    rowdot = (G * W).sum(1) / sigma
    dot = (ls * rowdot).sum()
    return dict(rowdot=rowdot, dot=dot, dW=(ls[:, None] * G - dot * u[:, None] * v[None, :]) / sigma, ls=ls)


def check_sn_weight(ins, got, strict=True):
    """got: dW and, when asked for, d_ls"""
    rows, cols = ins["G"].shape
    G, W, u, v = (ins[k].double() for k in ("G", "W", "u", "v"))
    sigma = abs(float(ins["sigma"].double()))
    ref = snw_reference(ins)
    ls = ref["ls"]
    rep = Report()
    # rowdot = (sum_k G W) (1 / sigma): a lane's ceil(cols / 64) serial multiply-adds, six shuffle levels, + 1 for the
    # products, + 2 for the reciprocal and the product with it
    rd_bound = (cdiv(cols, 64) + 9) * U * (G * W).abs().sum(1) / sigma
    if "d_ls" in got:
        rep.bounded("d_ls", got["d_ls"], ref["rowdot"], rd_bound)
    # dot = sum_r ls rowdot: a product, a thread's ceil(rows / 256) additions, block_sum_256 (6 + 3), and rowdot's own error
    dot_bound = (cdiv(rows, 256) + 10) * U * (ls * ref["rowdot"]).abs().sum() + (ls.abs() * rd_bound).sum()
    # dW = (ls G - dot u v) (1 / sigma): the apply pass rounds dot u, (dot u) v and the difference (three), ls G when
    # there is an ls, the reciprocal of sigma and the product with it (three more); dot's error travels with |u v| / sigma
    uv = (u[:, None] * v[None, :]).abs()
    bound = 6 * U * ((ls[:, None] * G).abs() + ref["dot"].abs() * uv) / sigma + dot_bound * uv / sigma
    rep.bounded("dW", got["dW"], ref["dW"], bound)
    return rep.done(strict)


def nonfinite_pattern(t):
    """+1 / -1 for +-inf, 2 for NaN, 0 for finite elements"""
    t = t.double()
    return torch.where(torch.isnan(t), 2, torch.where(torch.isinf(t), torch.sign(t), 0).long())


def check_sn_weight_nonfinite(ins, got, strict=True):
    """G holds an inf: dW (and d_ls) must be non-finite where the float64 formula is, with its signs / NaNs"""
    ref = snw_reference(ins)
    rep = Report()
    for name, r in (("dW", ref["dW"]), ("d_ls", ref["rowdot"])):
        if name in got:
            bad = nonfinite_pattern(got[name]) != nonfinite_pattern(r)
            rep.worst[name] = float(bad.sum())
            if bool(bad.any()):
                rep.fail(name, f"{int(bad.sum())} elements differ from the float64 formula's inf / NaN pattern, first at "
                               f"{tuple(int(i) for i in bad.nonzero()[0])}")
    return rep.done(strict)
