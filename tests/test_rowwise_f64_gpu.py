"""Row, reduction, streaming and cast kernels of libcalmvit_hip.so (csrc/norm_act.hip, csrc/spectral.hip, the GELU of
common.h) against float64 references written here, independent of emulated_backend.py.

Every bound is element-wise (or, for sums, an absolute bound scaled by the float64 sum of absolute terms) and carries
its derivation from fp32 rounding, u = 2^-24, and the serial depth d of the reduction.  d is computed from the host's
launch formulas (ln_bwd_grid, colsum_grid, latent_grid, calm_reduce_partials), replicated below.  Every output is the
interior of a larger buffer whose guard elements, and the interior itself, are prefilled with a NaN bit pattern no
kernel produces: the interior must be overwritten everywhere and the guards must stay untouched.  The views'
offsets are also how the alignment fallbacks (the scalar kernels) are reached.

GELU (gelu_erf_f / gelu_erf_grad_f of common.h), measured once on an MI355X over 2^20 + 1 points of [-12, 12]:
    max |gelu(x) - gelu_f64(x)| / max(1, |x|)   = 1.39e-7   (at x = 4.107; largest absolute error 5.7e-7)
    max |gelu'(x) - gelu'_f64(x)| / max(1, |x|) = 2.85e-7   (at x = 0.073)
The forward is at the level of its log2(erfc) fit (1.6e-7).  The derivative's worst case sits near x = 0, where
erf = 1 - poly(t) e^{-x^2/2} cancels: poly e ~ 0.94 carries the rounding of the Horner steps, v_rcp_f32 and __expf,
a few u of 1, against erf ~ 0.06 (the Abramowitz-Stegun fit alone accounts for 0.75e-7 of the cdf).  The test
asserts no more than twice these.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import calm_vit_dte_amd as calm
from attn16_f64 import FILL, GELU_BWD_ERR, GELU_FWD_ERR, assert_bf16_rounding_of, bf16_ord  # shared with the attention checker
from helpers import rel_err_elem

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24                     # unit roundoff of fp32
EPS = 1e-6                         # the model's LayerNorm eps (oracle LN_EPS)
GUARD = 40                         # guard elements on either side of every output


@pytest.fixture(scope="module")
def hip():
    return calm.backend.get_backend()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=gen(seed))


def ints(*shape, seed=0, lo=-8, hi=8):
    """Small integers: exact in bf16, and every partial sum of the sizes used here stays below 2^24."""
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).float()


def _bits(t):
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)


class Out:
    """An output tensor `shape` placed `off` elements past GUARD guard elements of a larger buffer, guards behind it
    too; guards and interior are prefilled with FILL (or the interior with `init`, for outputs that accumulate)."""

    def __init__(self, shape, dtype=torch.float32, off=0, init=None):
        shape = tuple(shape)
        n = math.prod(shape)
        self.dtype = dtype
        self.buf = torch.empty(2 * GUARD + off + n, dtype=dtype, device=DEV)
        _bits(self.buf).fill_(FILL[dtype])
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.t = self.buf[self.lo:self.hi].view(shape)
        if init is not None:
            self.t.copy_(init)
        self.before = _bits(self.buf).cpu().clone()

    def check(self, written=True):
        """Guards unchanged; with `written`, no interior element still holds the fill.  Returns the interior (CPU)."""
        b = _bits(self.buf).cpu()
        assert torch.equal(b[:self.lo], self.before[:self.lo]), "write before the output"
        assert torch.equal(b[self.hi:], self.before[self.hi:]), "write past the output"
        if written:
            stale = int((b[self.lo:self.hi] == self.before[self.lo:self.hi]).sum())
            assert stale == 0, f"{stale} output elements never written"
        return self.t.cpu()


def place(t, off=0):
    """Device copy of t starting `off` elements into a fresh (>= 256-byte aligned) allocation."""
    buf = torch.empty(off + t.numel(), dtype=t.dtype, device=DEV)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


def cdiv(a, b):
    return -(-a // b)


def grid_for(work, per_block):                      # norm_act.hip grid_for
    return max(1, min(2048, cdiv(work, per_block)))


def partials_depth(G):
    """calm_reduce_partials: ceil(G/64) adds into each of four running sums, three pairwise levels over the sums and
    the sixteen row lanes, (a0+a1)+(a2+a3) -> 2 + 2 + 2, and the add onto the output: ceil(G/64) + 7."""
    return cdiv(G, 64) + 7


def ln_bwd_depth(rows):
    """dw: rows per wave (grid ln_bwd_grid = min(512, ceil(rows/4)) blocks of 4 waves), the block's 4 waves, then
    calm_reduce_partials over the grid."""
    g = min(512, grid_for(rows, 4))
    return cdiv(rows, 4 * g) + 4 + partials_depth(g)


def colsum_depth(rows, cols, vec):
    """colsum_grid's launch: rows per row lane (+2: the lane's four running sums meet pairwise), the block's row lanes
    added in order, then calm_reduce_partials."""
    if vec:
        c4n = cols >> 2
        tx = 32 if c4n <= 32 else 64 if c4n <= 64 else 128 if c4n <= 128 else 256
        ty = 1024 // tx
        g = max(1, min(128, cdiv(rows, ty * 8)))
        return cdiv(rows, g * ty) + 2 + ty + partials_depth(g)
    per = 1 if cols >= 256 else 256 // cols
    g = max(1, min(512, cdiv(rows, per * 8)))
    return cdiv(rows, g * per) + per + partials_depth(g)


def colsum_is_vec(rows, cols, x):
    return cols % 4 == 0 and x.data_ptr() % 16 == 0 and rows >= 64


def latent_depth(rows, mvh, vec):
    """kl: the thread's serial sum (4 elements per vector item), block_sum_256 (6 shuffle levels + 3 serial adds of the
    wave sums), then calm_reduce_partials over latent_grid's blocks."""
    n = rows * mvh
    g = grid_for(n, 1024)
    per = 4 * cdiv(n // 4, g * 256) if vec else cdiv(n, g * 256)
    return per + 9 + partials_depth(g)


# ================================================================================================= 1. LayerNorm
VEC_D = [96, 256, 384, 672, 768, 1024, 1152, 1280]     # NV = 1, 1, 2, 3, 3, 4, 5, 5
SCALAR_D = [30, 1302, 1536, 2048]                       # D % 4 != 0, and 1284 <= D <= 2048


def ln_inputs(rows, D, kind="well", seed=0):
    if kind == "well":
        x = rnd(rows, D, seed=seed) * 2 + 0.5
    elif kind == "offset":
        x = 1e3 + rnd(rows, D, seed=seed)
    elif kind == "flat":                                 # sigma = 1e-3 (var = eps: the eps term matters)
        x = 1.0 + 1e-3 * rnd(rows, D, seed=seed)
    w = 1 + 0.1 * rnd(D, seed=seed + 1)
    dy = rnd(rows, D, seed=seed + 2)
    add = rnd(rows, D, seed=seed + 3)
    dw0 = rnd(D, seed=seed + 4)
    return x, w, dy, add, dw0


def ln_ref(x, w, dy, add=None, eps=EPS):
    D = x.shape[1]
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.layer_norm(x64, (D,), weight=w64, bias=None, eps=eps)
    y.backward(dy.double())
    var, mu = torch.var_mean(x64.detach(), dim=1, unbiased=False)
    rstd = (var + eps).rsqrt()
    xhat = (x.double() - mu[:, None]) * rstd[:, None]
    dx = x64.grad + (0 if add is None else add.double())
    return dict(y=y.detach(), mean=mu, rstd=rstd, xhat=xhat, dx=dx, dw=w64.grad, sigma=var.sqrt())


def ln_run(hip, x, w, dy, y_dtype=torch.float32, add=None, dw0=None, offs=None, eps=EPS, bwd=True):
    offs = offs or {}
    rows, D = x.shape
    X, W = place(x, offs.get("x", 0)), place(w, offs.get("w", 0))
    Y, M, R = Out((rows, D), y_dtype, offs.get("y", 0)), Out((rows,)), Out((rows,))
    hip.layernorm_fwd(X, W, Y.t, M.t, R.t, rows, D, eps)
    out = dict(y=Y.check(), mean=M.check(), rstd=R.check())
    if bwd:
        DY = place(dy, offs.get("dy", 0))
        A = None if add is None else place(add, offs.get("dx_add", 0))
        DX, DW = Out((rows, D), off=offs.get("dx", 0)), Out((D,), init=dw0)
        hip.layernorm_bwd(DY, X, W, M.t, R.t, DX.t, DW.t, rows, D, dx_add=A)
        out.update(dx=DX.check(), dw=DW.check(written=dw0 is None))
    return out


def ln_check(out, ref, x, w, dy, dw0=None, kind="well"):
    rows, D = x.shape
    absx = x.double().abs().mean(1)
    # mean: a lane adds its <= 4 ceil(D/256) elements serially, six shuffle levels, one division: (4 ceil(D/256) + 8) u
    # relative to mean|x| (a dropped or doubled element moves the mean by ~ mean|x| / D, 30x above this at D = 2048)
    assert ((out["mean"].double() - ref["mean"]).abs() <= (4 * cdiv(D, 256) + 8) * U * absx).all()
    # E = absolute error of xhat = (x - mu) rstd that any fp32 two-pass LayerNorm carries from the mean's error just
    # bounded: (4 ceil(D/256) + 8) u mean|x| rstd (<= 40 u |mu| / sigma at D = 2048; ~2e-6 on well-conditioned rows)
    E = (4 * cdiv(D, 256) + 8) * U * absx * ref["rstd"]
    # on ill-conditioned rows the y bound below takes 64 u |mu| / sigma >= E (the same loss, with margin)
    Ey = 64 * U * ref["mean"].abs() / ref["sigma"] if kind != "well" else torch.zeros(rows, dtype=torch.float64)
    # rstd: the variance sum has relative error (ceil(D/64) + 7) u < 1e-6 plus (E)^2 from the mean's error (second
    # order: the variance is minimal at the true mean); rsqrt 1 ulp
    rel = (out["rstd"].double() - ref["rstd"]).abs() / ref["rstd"]
    assert (rel <= 1e-5 + E ** 2).all(), float(rel.max())
    # y = (x - mu) rstd w: rstd's ~1e-6 plus three roundings; 1e-5 relative down to 1e-2 of the largest element,
    # plus 64 u (|mu| / sigma) |w| on ill-conditioned rows (at |mu|/sigma = 1e3: 3.8e-3; a one-pass E[x^2] - mu^2
    # variance loses u E[x^2] / var = 6e-2 of the variance there, i.e. 3e-2 in y, eight times this bound)
    floor = torch.maximum(ref["y"].abs(), 1e-2 * ref["y"].abs().max())
    ybound = 1e-5 * floor + Ey[:, None] * w.double().abs()
    if out["y"].dtype == torch.bfloat16:
        assert_bf16_rounding_of(out["y"], ref["y"], ybound)
    else:
        err = (out["y"].double() - ref["y"]).abs()
        assert (err <= ybound).all(), float((err / floor).max())
    if "dx" not in out:
        return
    # dx = rstd (g w - c1 - xhat c2) + dx_add: 5e-5 relative down to 1e-2 of the largest (c1, c2 are wave sums of D
    # terms, ~(D/64 + 6) u; rstd ~1e-6; the cancellation inside the bracket costs at most ~10x that at the floor),
    # plus rstd E (|c2| + |xhat| mean|g w|) from xhat's error
    g = dy.double() * w.double()
    c2 = (g * ref["xhat"]).mean(1)
    extra = ref["rstd"][:, None] * E[:, None] * (c2.abs()[:, None] + ref["xhat"].abs() * g.abs().mean(1)[:, None])
    err = (out["dx"].double() - ref["dx"]).abs()
    floor = torch.maximum(ref["dx"].abs(), 1e-2 * ref["dx"].abs().max())
    assert (err <= 5e-5 * floor + extra).all(), float((err / floor).max())
    # dw[c] = dw0[c] + sum_rows dy xhat: d serial additions (rows per wave + block waves + calm_reduce_partials) of
    # terms each carrying ~5 u of their own (xhat's two roundings, rstd, the product): (d + 8) u sum |dy xhat|,
    # u |dw| for the add onto dw0, plus sum |dy| E from xhat's absolute error (a term with xhat ~ 0 has no relative
    # accuracy)
    d = ln_bwd_depth(rows)
    dw_ref = ref["dw"] + (0 if dw0 is None else dw0.double())
    bound = ((d + 8) * U * (dy.double() * ref["xhat"]).abs().sum(0) + U * dw_ref.abs()
             + (dy.double().abs() * E[:, None]).sum(0))
    err = (out["dw"].double() - dw_ref).abs()
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("D", VEC_D + SCALAR_D)
@pytest.mark.parametrize("y16,dy16", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("with_add", [False, True])
def test_layernorm_kernels_types(hip, D, y16, dy16, with_add):
    """Every vector instance (NV = 1..5) and the scalar kernels, fp32 / bf16 y x fp32 / bf16 dy, with and without
    the skip-connection gradient; dw is added onto a non-zero incoming dw (calm_vit.h)."""
    x, w, dy, add, dw0 = ln_inputs(37, D, seed=D)
    if dy16:
        dy = dy.to(torch.bfloat16)
    add = add if with_add else None
    out = ln_run(hip, x, w, dy, torch.bfloat16 if y16 else torch.float32, add=add, dw0=dw0)
    ln_check(out, ln_ref(x, w, dy, add), x, w, dy, dw0)


@pytest.mark.parametrize("ptr", ["x", "y", "w", "dy", "dx", "dx_add"])
@pytest.mark.parametrize("D", [672, 1024])
def test_layernorm_alignment_fallback(hip, ptr, D):
    """One pointer at a time one element off 16-byte alignment: the host must take the scalar kernel, same results."""
    for y16, dy16 in ((False, False), (True, True)):
        x, w, dy, add, dw0 = ln_inputs(37, D, seed=3)
        if dy16:
            dy = dy.to(torch.bfloat16)
        out = ln_run(hip, x, w, dy, torch.bfloat16 if y16 else torch.float32, add=add, dw0=dw0, offs={ptr: 1})
        ln_check(out, ln_ref(x, w, dy, add), x, w, dy, dw0)


@pytest.mark.parametrize("rows,D", [(1, 672), (5, 672), (1, 30), (5, 1302), (1, 2048), (5, 96),
                                    (2048 + 37, 672), (2048 + 37, 1302)])
def test_layernorm_row_counts(hip, rows, D):
    x, w, dy, add, dw0 = ln_inputs(rows, D, seed=rows)
    out = ln_run(hip, x, w, dy, add=add, dw0=dw0)
    ln_check(out, ln_ref(x, w, dy, add), x, w, dy, dw0)


@pytest.mark.parametrize("y16", [False, True])
def test_layernorm_many_grid_passes(hip, y16):
    """57 344 rows (Base-224 stage 0 at batch 256): 7 passes of the forward's 2048-block grid, 28 rows per wave of
    the backward's 512-block grid."""
    rows, D = 57344, 672
    x, w, dy, add, dw0 = ln_inputs(rows, D, seed=11)
    if y16:
        dy = dy.to(torch.bfloat16)
    out = ln_run(hip, x, w, dy, torch.bfloat16 if y16 else torch.float32, add=add if y16 else None, dw0=dw0)
    ln_check(out, ln_ref(x, w, dy, add if y16 else None), x, w, dy, dw0)


@pytest.mark.parametrize("kind", ["offset", "flat"])
@pytest.mark.parametrize("D", [672, 1280, 1302, 2048])
def test_layernorm_ill_conditioned_rows(hip, kind, D):
    """1e3 + N(0,1) and 1 + 1e-3 N(0,1) rows: the bounds scale with |mu| / sigma (see ln_check)."""
    x, w, dy, add, dw0 = ln_inputs(37, D, kind=kind, seed=D + 1)
    out = ln_run(hip, x, w, dy, add=add, dw0=dw0)
    ln_check(out, ln_ref(x, w, dy, add), x, w, dy, dw0, kind=kind)


@pytest.mark.parametrize("D", [672, 30])
def test_layernorm_constant_row(hip, D):
    """An exactly constant row: mean exact, y = 0, rstd = eps^-1/2, finite dx."""
    x, w, dy, add, dw0 = ln_inputs(5, D, seed=5)
    x[2] = 3.25
    out = ln_run(hip, x, w, dy, add=add, dw0=dw0)
    assert float(out["mean"][2]) == 3.25
    assert torch.equal(out["y"][2], torch.zeros(D))
    assert abs(float(out["rstd"][2]) * math.sqrt(EPS) - 1) < 1e-6
    assert torch.isfinite(out["dx"]).all() and torch.isfinite(out["dw"]).all()
    ln_check(out, ln_ref(x, w, dy, add), x, w, dy, dw0)


def nonfinite_pattern(t):
    """+1 / -1 for +-inf, 2 for NaN, 0 for finite elements."""
    t = t.double()
    return torch.where(torch.isnan(t), 2, torch.where(torch.isinf(t), torch.sign(t), 0).long())


@pytest.mark.parametrize("D", [96, 672, 1152, 30])
@pytest.mark.parametrize("dy16", [False, True])
def test_layernorm_non_finite_gradient(hip, D, dy16):
    """inf / NaN in dy (an overflowed loss-scaled step) stay in their row and propagate as in exact arithmetic of
    dx = rstd ((g - c1) - xhat c2), g = dy w, c1 = mean(g), c2 = mean(g xhat): the other elements of the row become
    -inf or NaN by the sign of xhat, not NaN throughout.  The +inf sits in the row's last 16-byte chunk, which the
    vector kernel's out-of-row lanes also load (clamped) and must zero; every other row stays finite and correct."""
    x, w, dy, add, dw0 = ln_inputs(6, D, seed=D + 2)
    dy[1, D - 3] = math.inf
    dy[3, D - 2] = -math.inf
    dy[4, 1] = math.nan
    if dy16:
        dy = dy.to(torch.bfloat16)
    out = ln_run(hip, x, w, dy, add=add, dw0=dw0)
    ref = ln_ref(x, w, dy.float().nan_to_num(0.0, 0.0, 0.0), add)
    g = dy.double() * w.double()
    c1, c2 = g.mean(1, keepdim=True), (g * ref["xhat"]).mean(1, keepdim=True)
    dx_f = ref["rstd"][:, None] * ((g - c1) - ref["xhat"] * c2) + add.double()
    assert torch.equal(nonfinite_pattern(out["dx"]), nonfinite_pattern(dx_f))
    dw_f = dw0.double() + (dy.double() * ref["xhat"]).sum(0)
    assert torch.equal(nonfinite_pattern(out["dw"]), nonfinite_pattern(dw_f))
    rows_ok = [0, 2, 5]
    assert torch.isfinite(out["dx"][rows_ok]).all()
    err = (out["dx"][rows_ok].double() - ref["dx"][rows_ok]).abs()
    assert (err <= 5e-5 * torch.maximum(ref["dx"][rows_ok].abs(), 1e-2 * ref["dx"][rows_ok].abs().max())).all()


def test_layernorm_limits(hip):
    """D = 2052: the backward keeps 32 columns per lane in registers and refuses (CALM_E_UNSUPP); the forward
    has no such limit and must stay correct."""
    x, w, dy, add, dw0 = ln_inputs(5, 2052, seed=7)
    out = ln_run(hip, x, w, dy, bwd=False)
    ln_check(out, ln_ref(x, w, dy), x, w, dy)
    X, W, DY = x.to(DEV), w.to(DEV), dy.to(DEV)
    mean, rstd = out["mean"].to(DEV), out["rstd"].to(DEV)
    with pytest.raises(RuntimeError, match="code -3"):
        hip.layernorm_bwd(DY, X, W, mean, rstd, torch.empty_like(X), torch.zeros(2052, device=DEV), 5, 2052)


# ================================================================================================= 2. reductions
COLSUM_CASES = [
    # rows, cols, x offset (elements)     vector kernel instance / scalar branch
    (200, 96, 0),                         # TX = 32
    (200, 240, 0),                        # TX = 64
    (300, 448, 0),                        # TX = 128
    (100, 1344, 0),                       # TX = 256, several 256-lane passes per row
    (64, 4096, 0),                        # TX = 256, COLSUM_MAXC
    (64, 96, 0),                          # TX = 32 at the rows >= 64 boundary
    (63, 96, 0),                          # scalar, rows < 64
    (500, 30, 0),                         # scalar, cols % 4 != 0, 8 row lanes per block
    (300, 301, 0),                        # scalar, cols >= 256
    (200, 448, 1),                        # scalar, misaligned x
    (57344, 448, 0),                      # 128 blocks x 8 row lanes: 56 rows per lane
    (57344, 30, 0),                       # scalar at many rows
]


@pytest.mark.parametrize("rows,cols,off", COLSUM_CASES)
@pytest.mark.parametrize("x16", [False, True])
def test_colsum(hip, rows, cols, off, x16):
    dt = torch.bfloat16 if x16 else torch.float32
    # exactness: small integers, every partial sum < 2^24 -> every summation order is exact; a dropped, doubled or
    # mis-strided row / column shows as an integer difference
    xi, o0 = ints(rows, cols, seed=cols).to(dt), ints(cols, seed=1)
    X = place(xi, off)
    O = Out((cols,), init=o0)
    hip.colsum(X, O.t, rows, cols)
    assert torch.equal(O.check(written=False).double(), o0.double() + xi.double().sum(0))
    # random: d serial additions, each rounding at most u |partial| <= u sum|x|
    xr = (rnd(rows, cols, seed=cols + 1) * 3 + 1).to(dt)
    X = place(xr, off)
    O = Out((cols,), init=o0)
    hip.colsum(X, O.t, rows, cols)
    d = colsum_depth(rows, cols, colsum_is_vec(rows, cols, X))
    ref = o0.double() + xr.double().sum(0)
    bound = d * U * (xr.double().abs().sum(0) + o0.double().abs())
    assert ((O.check(written=False).double() - ref).abs() <= bound).all()


def test_colsum_limits(hip):
    x = torch.zeros(8, 4097, device=DEV)
    with pytest.raises(RuntimeError, match="code -3"):
        hip.colsum(x, torch.zeros(4097, device=DEV), 8, 4097)


@pytest.mark.parametrize("B,H,per", [(2, 12, 224 * 80), (3, 6, 1001), (1, 1, 5)])
def test_sum_heads(hip, B, H, per):
    for dl in (ints(B, H, per, seed=per), rnd(B, H, per, seed=per + 1)):
        O = Out((B, per))
        hip.sum_heads(place(dl), O.t, B, H, per)
        got, ref = O.check().double(), dl.double().sum(1)
        if dl.eq(dl.round()).all():
            assert torch.equal(got, ref)
        else:                                              # H serial additions
            assert ((got - ref).abs() <= H * U * dl.double().abs().sum(1)).all()


@pytest.mark.parametrize("B,S,D", [(3, 48, 144), (2, 224, 672), (4, 7, 30)])
def test_mean_seq(hip, B, S, D):
    # forward: exact integer sum, then one correctly rounded division -> bit-exact against float64 rounded once
    x = ints(B, S, D, seed=S)
    Y = Out((B, D))
    hip.mean_seq_fwd(place(x), Y.t, B, S, D)
    assert torch.equal(Y.check(), (x.double().sum(1) / S).float())
    xr = rnd(B, S, D, seed=S + 1)
    Y = Out((B, D))
    hip.mean_seq_fwd(place(xr), Y.t, B, S, D)
    # S serial additions + the division
    assert ((Y.check().double() - xr.double().mean(1)).abs() <= (S + 1) * U * xr.double().abs().mean(1)).all()
    # backward: dy * fl(1/S), one product of two fp32 values rounded once
    dy = rnd(B, D, seed=S + 2)
    DX = Out((B, S, D))
    hip.mean_seq_bwd(place(dy), DX.t, B, S, D)
    inv = torch.tensor(1.0 / S, dtype=torch.float32).double()
    assert torch.equal(DX.check(), (dy.double() * inv).float()[:, None, :].expand(B, S, D))


@pytest.mark.parametrize("rows,cols", [(1344, 672), (40, 24), (7, 3)])
@pytest.mark.parametrize("o16", [False, True])
def test_row_scale(hip, rows, cols, o16):
    """out = x * s[row]: bit-exact against the fp32 product (exact in float64, rounded once), RNE to bf16 for a bf16
    output.  1344 x 672 exceeds one pass of the 2048-block grid."""
    x, s = rnd(rows, cols, seed=rows), rnd(rows, seed=cols)
    O = Out((rows, cols), torch.bfloat16 if o16 else torch.float32)
    hip.row_scale(place(x), place(s), O.t, rows, cols)
    ref = (x.double() * s.double()[:, None]).float()
    got = O.check()
    assert torch.equal(got.view(torch.int16) if o16 else got, ref.to(torch.bfloat16).view(torch.int16) if o16 else ref)


# ================================================================================================= 3. softmax
def softmax_logits(rows, cols, kind, seed):
    x = rnd(rows, cols, seed=seed) * 3
    if kind == "offset":          # no max-subtraction -> e^(1e4) overflows
        x = x + 1e4
    elif kind == "spread":        # x50: most of a row underflows, the max element carries it
        x = x * 50
    return x


@pytest.mark.parametrize("rows,cols", [(37, 1), (37, 63), (37, 65), (37, 224), (37, 1024), (8192 + 5, 224),
                                       (8192 + 5, 1024)])
@pytest.mark.parametrize("kind", ["plain", "offset", "spread"])
def test_softmax(hip, rows, cols, kind):
    x = softmax_logits(rows, cols, kind, seed=cols)
    P = Out((rows, cols), init=x)
    hip.softmax_fwd(P.t, rows, cols)
    p = P.check(written=False)
    ref = torch.softmax(x.double(), -1)
    # expf 1 ulp, the row sum ~(cols/64 + 6) u, the reciprocal and the product: < 2e-6 relative; 1e-5 down to 1e-3
    # of the largest element (e^(v - m) of elements below that carries the rounding of v - m, |v - m| u)
    assert rel_err_elem(p, ref, floor=1e-3) <= 1e-5
    # every element within a few u of p: the row sums to 1 within (cols/64 + 8) u < 2e-6
    assert float((p.double().sum(-1) - 1).abs().max()) <= 2e-6
    # backward, in place on dp: dp = p (g - sum_j p_j g_j) on the fp32 probabilities
    p32 = ref.float()
    g = rnd(rows, cols, seed=cols + 1)
    G = Out((rows, cols), init=g)
    hip.softmax_bwd(place(p32), G.t, rows, cols)
    pd, gd = p32.double(), g.double()
    s = (pd * gd).sum(-1, keepdim=True)
    dref = pd * (gd - s)
    # 1e-5 down to 1e-3 of the largest, and where g_i ~ s cancels: the wave sum s carries (cols/64 + 8) u sum|p g|,
    # the difference and the product two more roundings
    err = (G.check(written=False).double() - dref).abs()
    floor = torch.maximum(dref.abs(), 1e-3 * dref.abs().max())
    cancel = (cdiv(cols, 64) + 10) * U * pd * ((pd * gd).abs().sum(-1, keepdim=True) + gd.abs())
    assert (err <= 1e-5 * floor + cancel).all()


def test_softmax_limits(hip):
    x = torch.zeros(4, 1025, device=DEV)
    with pytest.raises(RuntimeError, match="code -3"):
        hip.softmax_fwd(x, 4, 1025)
    with pytest.raises(RuntimeError, match="code -3"):
        hip.softmax_bwd(x, x.clone(), 4, 1025)


@pytest.mark.parametrize("B,H,Sq,cols", [(2, 3, 48, 16), (1, 12, 80, 224), (3, 4, 5, 1024), (2, 12, 7, 65)])
def test_softmax_bwd_heads(hip, B, H, Sq, cols):
    # exactness: integer p, g -> s, dp and the head sum are integers below 2^24, exact in any order
    for p, g in ((ints(B, H, Sq, cols, seed=1, lo=-2, hi=2), ints(B, H, Sq, cols, seed=2, lo=-2, hi=2)),
                 (torch.softmax(rnd(B, H, Sq, cols, seed=3) * 3, -1), rnd(B, H, Sq, cols, seed=4))):
        G, M = Out((B, H, Sq, cols), init=g), Out((B, Sq, cols))
        hip.softmax_bwd_heads(place(p), G.t, M.t, B, H, Sq, cols)
        pd, gd = p.double(), g.double()
        s = (pd * gd).sum(-1, keepdim=True)
        dref = pd * (gd - s)
        got_d, got_m = G.check(written=False).double(), M.check().double()
        if p.eq(p.round()).all():
            assert torch.equal(got_d, dref) and torch.equal(got_m, dref.sum(1))
            continue
        cancel = (cdiv(cols, 64) + 10) * U * pd.abs() * ((pd * gd).abs().sum(-1, keepdim=True) + gd.abs())
        assert ((got_d - dref).abs() <= U * dref.abs() + cancel).all()
        # head sum: H serial additions of the per-head results, each within `cancel`
        bound = H * U * dref.abs().sum(1) + cancel.sum(1)
        assert ((got_m - dref.sum(1)).abs() <= bound).all()


# ================================================================================================= 4. GELU
def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def gelu_grad64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def gelu_points():
    edge = 5 * math.sqrt(2)
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, edge, -edge, 3e38, -3e38], dtype=torch.float32)
    edge32 = torch.tensor([edge, -edge], dtype=torch.float32)
    near = torch.cat([torch.nextafter(edge32, torch.full_like(edge32, math.inf)),
                      torch.nextafter(edge32, torch.full_like(edge32, -math.inf))])
    return torch.cat([torch.linspace(-12, 12, (1 << 20) + 1), special, near])


def test_gelu_accuracy(hip):
    """Forward and backward against the float64 erf GELU and its derivative; |error| <= 2 x the measured worst case
    (module docstring) x max(1, |x|) — the product x (...) rounds relative to x."""
    x = gelu_points()
    n = x.numel()
    Y = Out((n,))
    hip.gelu_fwd(place(x), Y.t, n)
    x64 = x.double()
    scale = x64.abs().clamp_min(1)
    err = (Y.check().double() - gelu64(x64)).abs() / scale
    assert float(err.max()) <= 2 * GELU_FWD_ERR, float(err.max())
    DZ = Out((n,))
    hip.gelu_bwd(place(torch.ones(n)), place(x), DZ.t, n)
    err = (DZ.check().double() - gelu_grad64(x64)).abs() / scale
    assert float(err.max()) <= 2 * GELU_BWD_ERR, float(err.max())
    # with an incoming gradient: one more rounding of the product
    dy = rnd(n, seed=9)
    DZ = Out((n,))
    hip.gelu_bwd(place(dy), place(x), DZ.t, n)
    ref = dy.double() * gelu_grad64(x64)
    err = (DZ.check().double() - ref).abs()
    assert (err <= dy.double().abs() * 2 * GELU_BWD_ERR * scale + U * ref.abs()).all()


def test_gelu_non_finite_inputs(hip):
    """+inf, -inf, NaN must stay non-finite through both directions (GradScaler's inf check relies on it).  The
    device values: forward +inf -> +inf, -inf -> NaN (-inf x erfc-rounded-to-0), NaN -> NaN; backward NaN for all
    three (x e^{-x^2/2} = inf x 0).  float64 torch gives +inf / NaN / NaN and NaN / NaN / NaN."""
    x = torch.tensor([math.inf, -math.inf, math.nan])
    Y, DZ = Out((3,)), Out((3,))
    hip.gelu_fwd(place(x), Y.t, 3)
    hip.gelu_bwd(place(torch.ones(3)), place(x), DZ.t, 3)
    y, dz = Y.check(), DZ.check()
    assert not torch.isfinite(y).any() and not torch.isfinite(dz).any()
    assert float(y[0]) == math.inf and math.isnan(float(y[1])) and math.isnan(float(y[2]))
    assert torch.isnan(dz).all()


# ================================================================================================= 5. latent + KL
def latent_inputs(rows, mvh, seed):
    mean = rnd(rows, mvh, seed=seed) * 2
    raw = torch.rand(rows, mvh, generator=gen(seed + 1)) * 130 - 90       # [-90, 40]
    flat = raw.view(-1)
    probes = torch.tensor([-90.0, -6.9, -6.91, -6.9077554, 0.0, 1e-3, -1e-3, 19.99, 20.0, 20.01, 40.0])
    flat[:probes.numel()] = probes[:flat.numel()]       # the t < 1e-3 switch (x ~ -6.9078) and the x > 20 threshold
    return torch.cat([mean, raw], 1), rnd(rows, mvh, seed=seed + 2)


def softplus64(x):
    return F.softplus(x.double())                        # oracle: F.softplus(raw) + SOFTPLUS_FLOOR


@pytest.mark.parametrize("rows,mvh,off", [(37, 24, 0), (20480, 240, 0), (37, 30, 0), (37, 240, 1), (1, 4, 0)])
@pytest.mark.parametrize("with_noise", [True, False])
def test_latent(hip, rows, mvh, off, with_noise):
    """mvh % 4 == 0 with aligned tensors: the vector kernel (softplus_fast, hardware exp / log); mvh = 30 or an
    misaligned mv: the scalar kernel."""
    mv, noise = latent_inputs(rows, mvh, seed=mvh + off)
    noise = noise if with_noise else None
    MV = place(mv, off)
    N = None if noise is None else place(noise)
    vec = mvh % 4 == 0 and off == 0
    Z, S = Out((rows, mvh)), Out((rows, mvh))
    kl0 = torch.tensor([0.75])
    K = Out((1,), init=kl0)
    hip.latent_fwd(MV, N, Z.t, S.t, K.t, rows, mvh)
    z, sd, kl = Z.check().double(), S.check().double(), K.check(written=False).double()
    m64, raw64 = mv[:, :mvh].double(), mv[:, mvh:].double()
    sd_ref = softplus64(raw64) + 1e-6
    # std to 4 significant digits (norm_act.hip above softplus_fast: <= 6e-5 relative), so log std within 1e-4
    assert float(((sd - sd_ref).abs() / sd_ref).max()) <= 1e-4
    assert float((sd.log() - sd_ref.log()).abs().max()) <= 1e-4
    # z = mean + noise std: the fma rounds once; std's own error carried by |noise|
    n64 = torch.zeros_like(m64) if noise is None else noise.double()
    z_ref = m64 + n64 * sd_ref
    assert ((z - z_ref).abs() <= 2 * U * (m64.abs() + (n64 * sd_ref).abs()) + n64.abs() * 1e-4 * sd_ref).all()
    # kl_sum += sum(1 + 2 log std - mean^2 - std^2), checked on the kernel's own std: each term carries ~4 u of its
    # parts plus the log's error (<= 2^-20 + 4 u |log std|), then d serial additions
    terms = 1 + 2 * sd.log() - m64 ** 2 - sd ** 2
    absterms = 1 + 2 * sd.log().abs() + m64 ** 2 + sd ** 2
    d = latent_depth(rows, mvh, vec)
    bound = (d + 8) * U * (absterms.sum() + 0.75) + 2 * (2.0 ** -20 * terms.numel() + 4 * U * sd.log().abs().sum())
    assert abs(float(kl) - (0.75 + float(terms.sum()))) <= float(bound)
    # backward on the fp32 std of the reference: dmean = dz - 2 dk mean; draw = (dz noise + dk (2/std - 2 std)) sigmoid
    std_in = sd_ref.float()
    dz, dk = rnd(rows, mvh, seed=5), torch.tensor([0.3])
    DMV = Out((rows, 2 * mvh), off=off)
    hip.latent_bwd(place(dz), place(dk), MV, N, place(std_in), DMV.t, rows, mvh)
    dmv = DMV.check().double()
    s64, dz64, dk64 = std_in.double(), dz.double(), float(dk.double())
    dmean = dz64 - 2 * dk64 * m64
    assert ((dmv[:, :mvh] - dmean).abs() <= 3 * U * (dz64.abs() + 2 * abs(dk64) * m64.abs())).all()
    sig = torch.sigmoid(raw64)
    parts = (dz64 * n64).abs() + abs(dk64) * (2 / s64 + 2 * s64)
    draw = ((dz64 * n64) + dk64 * (2 / s64 - 2 * s64)) * sig
    # five roundings of the parts, expf and the reciprocal in the sigmoid (<= 4 u); below raw = -87.3 the sigmoid is
    # an fp32 subnormal (fewer digits) and below -88.7 it is 0 (1 + e^-raw = inf): there the whole (tiny) value
    tiny = torch.where(raw64 < -87.3, parts * sig, torch.zeros_like(sig))
    assert ((dmv[:, mvh:] - draw).abs() <= 10 * U * parts * sig + tiny).all()


# ================================================================================================= 6. casts
def cast_values():
    """fp32 bit patterns: random values at many scales, exact ties (kept mantissa odd / even), values that round to
    +-inf, subnormals, +-0, +-inf and NaNs (one whose truncation would be inf)."""
    g = gen(21)
    rand = torch.randn(4096, generator=g) * torch.exp2(torch.randint(-30, 30, (4096,), generator=g).float())
    hi16 = torch.randint(0x0080, 0x7F7F, (512,), generator=g, dtype=torch.int32)
    ties = torch.cat([(hi16 << 16) | 0x8000, ((hi16 | 1) << 16) | 0x8000, ((hi16 & ~1) << 16) | 0x8000,
                      (hi16 << 16) | 0x7FFF, (hi16 << 16) | 0x8001])
    ties = torch.cat([ties, ties | (-(1 << 31))])
    sub = torch.cat([torch.randint(1, 0x007FFFFF, (512,), generator=g, dtype=torch.int32),
                     torch.tensor([1, 0x8000, 0x18000, 0x7FFF, 0x8001, 0x007FFFFF, 0x007F8000, 0x007FFFFF],
                                  dtype=torch.int32)])
    sub = torch.cat([sub, sub | (-(1 << 31))])
    edge = torch.tensor([0x7F7F8000, 0x7F7FFFFF, 0x7F7F7FFF, 0x7F7E8000, 0, 0x7F800000, 0x7FC00000,
                         0x7F800001, 0x7FBFFFFF, 0x7F80FFFF, 0x3F808000, 0x3F818000], dtype=torch.int32)
    edge = torch.cat([edge, edge | (-(1 << 31))])
    return torch.cat([edge.view(torch.float32), ties.view(torch.float32), sub.view(torch.float32), rand])


VALUES = None


def cast_src(n, seed=0):
    global VALUES
    if VALUES is None:
        VALUES = cast_values()
    idx = torch.randint(0, VALUES.numel(), (n,), generator=gen(seed))
    src = VALUES[idx]
    src[:min(n, VALUES.numel())] = VALUES[:min(n, VALUES.numel())]
    return src


def assert_rne(got16, src32):
    ref = src32.to(torch.bfloat16)            # torch: round to nearest even, NaN stays NaN
    nan = torch.isnan(src32)
    assert torch.isnan(got16.float()[nan]).all(), "NaN input lost its NaN"
    assert torch.equal(got16.view(torch.int16)[~nan], ref.view(torch.int16)[~nan])


CHUNK = 16384                                 # calm_cast_chunk_elems(), checked below


@pytest.mark.parametrize("n", list(range(1, 18)) + [CHUNK - 1, CHUNK + 1, 3 * (1 << 20) + 5])
def test_cast_bf16_one(hip, n):
    assert hip.lib.calm_cast_chunk_elems() == CHUNK
    src = cast_src(n, seed=n)
    for s_off, d_off in ((0, 0), (1, 0), (0, 1), (3, 5)):
        O = Out((n,), torch.bfloat16, off=d_off)
        hip.cast_bf16(place(src, s_off), O.t)
        assert_rne(O.check(), src)


def test_cast_plan_multi_entry(hip):
    """cast_plan + cast_run over entries whose sizes are not multiples of the chunk, one of them misaligned (the
    element-wise branch of cast_bf16_kernel)."""
    sizes = [1, CHUNK + 1, 40000, 7, 3 * CHUNK - 3, 2 * CHUNK]
    offs = [(0, 0), (0, 0), (1, 0), (0, 0), (0, 3), (0, 0)]
    srcs = [cast_src(n, seed=100 + i) for i, n in enumerate(sizes)]
    outs = [Out((n,), torch.bfloat16, off=do) for n, (_, do) in zip(sizes, offs)]
    dsrc = [place(s, so) for s, (so, _) in zip(srcs, offs)]
    plan = hip.cast_plan([(s, o.t) for s, o in zip(dsrc, outs)])
    hip.cast_run(plan)
    for s, o in zip(srcs, outs):
        assert_rne(o.check(), s)


@pytest.mark.parametrize("off", [0, 1])
def test_cast_f32_widens_every_bf16(hip, off):
    """All 65 536 bf16 bit patterns widen bit-exactly (NaNs stay NaN)."""
    src = torch.arange(-(1 << 15), 1 << 15, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    S = place(src, off)
    O = Out((src.numel(),), off=off)
    assert hip.lib.calm_cast_f32_one(S.data_ptr(), O.t.data_ptr(), src.numel(), calm.backend._stream()) == 0
    got = O.check()
    nan = torch.isnan(src.float())
    assert torch.isnan(got[nan]).all()
    assert torch.equal(got.view(torch.int32)[~nan], src.float().view(torch.int32)[~nan])
