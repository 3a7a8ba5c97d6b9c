"""Float64 references, element-wise bounds and case tables for the CNN tail (csrc/cnn_fused.hip, the dwconv3x3 and the
token permutations of csrc/tokens_conv.hip) and the optimizer-side step (csrc/optim.hip, calm_optim_step).

The module knows nothing about who produced the tensors it checks: the GPU tests hand it the kernels' outputs, the CPU
tests an fp32 emulation's (and planted faults).  It does not import emulated_backend.

Every bound is per element and derived from operation counts, never from what a kernel returned:

    U = 2^-24     unit roundoff of fp32.  A value computed by k fp32 operations from terms whose absolute values sum to
                  A carries at most k U A (first order).  An effective weight w / sigma is two operations (the
                  reciprocal, the product), each product with it one more, each addition of the chain one more.
    sums          d U (sum of |terms| + |initial content|) for a sum of serial depth d, plus the sum of the terms' own
                  errors.  d is replicated from the host launch formulas: cnn_grad_depth, optim_sum_depth,
                  dwconv_bwd_chain, and calm_reduce_partials' ceil(G / 64) + 7.
    GELU          2 GELU_FWD_ERR max(1, |z|) and 2 GELU_BWD_ERR max(1, |z|) (attn16_f64.py: the measured error of the
                  device GELU, asserted at twice that by test_rowwise_f64_gpu.py), on top of the argument's own error
                  times max |gelu'| = 1.13, max |gelu''| = 0.8.  The errors travel through the following layers by an
                  absolute-value pass of the same network (|w| in place of w, the error map in place of the activation).

The optimizer reference starts from the fp32 VALUES the ABI receives: calm_optim_hparams holds floats, so lr, the betas,
eps, weight_decay and max_norm are rounded to fp32 first and only then widened.  fl32(0.999) is not 0.999: in [0.5, 1) fp32
values are 2^-24 apart, so |fl32(beta) - beta| <= 2^-25 and 1 - beta is off by up to 2^-25 / (1 - beta) = 2.98e-5 relative
at beta = 0.999 (= u beta / (1 - beta) with u = 2^-25 the relative half-spacing there).  At t = 1 the bias correction
1 - beta^t IS 1 - beta, so a reference on double-precision betas would charge the kernel 3e-5 of relative error in
sqrt-bias-correction terms that it does not commit.  What the kernel does commit is powf's documented 1 ulp: beta^t in
[0.5, 1) is off by at most 2^-24 absolute, which _pow_err charges as 2 U beta^t.
"""
import math

import torch
import torch.nn.functional as F

from attn16_f64 import FILL, GELU_BWD_ERR, GELU_FWD_ERR, _Report  # noqa: F401  (FILL re-exported for the tests)

U = 2.0 ** -24
CH = 32                       # hidden channels of proj
TILE = 16                     # cnn_fused.hip T
CNN_FWD_MAX_GRID = 256 * 6    # calm_cnn_residual_fwd
CNN_BWD_MAX_GRID = 256        # common.h
CNN_BWD_GROUPS = 32           # BG: pixel groups of the backward's 512 threads
OPT_CHUNK = 16384             # calm_optim_chunk_elems()
OPT_NT = 256
DW_NT = 256
DW_BWD_MAX_GRID = 1024
DW_MAXC = 64
GELU_D1_MAX = 1.13            # max |gelu'|  (1.1289 at x = 1.41)
GELU_D2_MAX = 0.8             # max |gelu''| (2 phi(0) = 0.798)


def cdiv(a, b):
    return -(-a // b)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def partials_depth(G):
    """calm_reduce_partials (common.h): ceil(G/64) adds into each of four running sums, three pairwise levels over the
    sums and the sixteen row lanes, and the add onto the output: ceil(G/64) + 7."""
    return cdiv(G, 64) + 7


# ================================================================================================= 1. fused CNN tail
CNN_CASES = [
    # B, S, backward      what it reaches
    (1, 1, True),         # halo entirely outside the image
    (1, 2, True),
    (1, 15, True),        # just under one tile
    (1, 16, True),        # exactly one tile
    (1, 17, True),        # a second tile row / column one pixel wide
    (1, 33, True),        # 3 x 3 tiles
    (3, 20, True),        # batch stride
    (65, 17, True),       # 260 tiles > 256: the backward loops, workgroups 0-3 take two tiles
    (130, 17, True),      # 520 tiles: workgroups 0-7 take three tiles, the rest two
    (385, 17, False),     # 1540 tiles > 1536: the forward loops; forward only
]


def cnn_tiles(B, S):
    tps = cdiv(S, TILE)
    return B * tps * tps


def cnn_grids(B, S):
    """(forward grid, backward grid, most tiles one backward workgroup takes)"""
    n = cnn_tiles(B, S)
    g = min(n, CNN_BWD_MAX_GRID)
    return min(n, CNN_FWD_MAX_GRID), g, cdiv(n, g)


def cnn_grad_depth(B, S):
    """Serial depth of a weight-gradient element: a thread adds ceil(18 * 18 / 32) = 11 pixels per tile (the dh2p loop;
    the other loops add fewer) over its workgroup's tiles, the workgroup adds its 32 pixel groups in order, then
    calm_reduce_partials over the grid; + 2 for the products inside a term."""
    _, g, per_wg = cnn_grids(B, S)
    return cdiv((TILE + 2) ** 2, CNN_BWD_GROUPS) * per_wg + CNN_BWD_GROUPS + partials_depth(g) + 2


CNN_GRADS = (("g0", CH * 3), ("gb0", CH), ("g2", CH * 9), ("gb2", CH), ("g4", 3 * CH), ("gb4", 3))


def cnn_inputs(B, S, seed=0):
    """sigma in 0.7-1.3, biases of order 1 (gelu(b0) != 0: padding the wrong tensor shows), a few pixels that push the
    pre-activations beyond +-8, sample 1 all zero, distinct data per sample, non-zero initial gradient contents."""
    g = gen(1000 * seed + 7 * B + S)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    x, dy = rn(B, S, S, 3), rn(B, S, S, 3)
    for b in range(0, B, 2):                                  # |z1| ~ 0.6 * 1.7 * 14 / sigma > 8, and so z2 around it
        y0, x0 = (3 * b + 1) % S, (5 * b + 2) % S
        x[b, y0:y0 + 2, x0:x0 + 2] = 14.0 * torch.sign(x[b, y0:y0 + 2, x0:x0 + 2])
    if B > 1:
        x[1] = 0.0
    ins = dict(x=x.reshape(B, S, 3 * S).contiguous(), dy=dy.reshape(B, S, 3 * S).contiguous(),
               w0=rn(CH, 3, sc=0.6), b0=rn(CH), w2=rn(CH, 9, sc=0.4), b2=rn(CH), w4=rn(3, CH, sc=0.3), b4=rn(3))
    for k in ("s0", "s2", "s4"):
        ins[k] = 0.7 + 0.6 * torch.rand(1, generator=g)
    for name, n in CNN_GRADS:
        ins[name + "_init"] = rn(n)
    return ins


CNN_W = ("w0", "s0", "b0", "w2", "s2", "b2", "w4", "s4", "b4")


def _pad1(t):
    return F.pad(t, (0, 0, 1, 1, 1, 1))


def _tap(tp, S, ky, kx):
    """tp = _pad1(t): t[y + ky - 1, x + kx - 1] (zero outside the image) for every (y, x)"""
    return tp[:, ky:ky + S, kx:kx + S]


def cnn_reference(ins, B, S, residual, backward=True):
    """out = res x + conv1x1(gelu(dw3x3(gelu(conv1x1(x))))) on [B,S,S,3] and, with `backward`, dx and the gradients with
    respect to the EFFECTIVE weights w / sigma and the biases (calm_vit.h), added onto the initial contents.  Closed
    form in float64.  Returns (ref, bound), both keyed by output name."""
    d = lambda k: ins[k].double()
    x = d("x").view(B, S, S, 3)
    W0, W2, W4 = d("w0").view(CH, 3) / d("s0"), d("w2").view(CH, 9) / d("s2"), d("w4").view(3, CH) / d("s4")
    b0, b2, b4 = d("b0"), d("b2"), d("b4")
    A0, A2, A4 = W0.abs(), W2.abs(), W4.abs()
    res = 1.0 if residual else 0.0
    ref, bound = {}, {}
    taps = [(ky, kx) for ky in range(3) for kx in range(3)]
    # conv0: 3 products with 2-operation weights and 3 additions -> 6 U
    z1 = x @ W0.t() + b0
    e_z1 = 6 * U * (x.abs() @ A0.t() + b0.abs())
    h1 = gelu64(z1)
    e_h1 = GELU_D1_MAX * e_z1 + 2 * GELU_FWD_ERR * z1.abs().clamp_min(1.0)
    h1p, e_h1p = _pad1(h1), _pad1(e_h1)                       # zero padding applies to the dwconv INPUT (h1)
    # dwconv: 9 products, 9 additions -> 12 U, plus h1's error through |w2|
    z2, a2, e_z2 = b2.expand_as(h1).clone(), b2.abs().expand_as(h1).clone(), torch.zeros_like(h1)
    for k, (ky, kx) in enumerate(taps):
        z2 += W2[:, k] * _tap(h1p, S, ky, kx)
        a2 += A2[:, k] * _tap(h1p, S, ky, kx).abs()
        e_z2 += A2[:, k] * _tap(e_h1p, S, ky, kx)
    e_z2 += 12 * U * a2
    h2 = gelu64(z2)
    e_h2 = GELU_D1_MAX * e_z2 + 2 * GELU_FWD_ERR * z2.abs().clamp_min(1.0)
    # conv4 + skip: 32 products in a chain of 33 additions, the fma with res -> (CH + 6) U
    ref["out"] = (h2 @ W4.t() + b4 + res * x).reshape(B, S, 3 * S)
    bound["out"] = (e_h2 @ A4.t() + (CH + 6) * U * (h2.abs() @ A4.t() + b4.abs() + res * x.abs())).reshape(B, S, 3 * S)
    if not backward:
        return ref, bound
    dy = d("dy").view(B, S, S, 3)
    gz1, gz2 = gelu_grad64(z1), gelu_grad64(z2)
    e_gz1 = GELU_D2_MAX * e_z1 + 2 * GELU_BWD_ERR * z1.abs().clamp_min(1.0)
    e_gz2 = GELU_D2_MAX * e_z2 + 2 * GELU_BWD_ERR * z2.abs().clamp_min(1.0)
    dh2 = dy @ W4
    e_dh2 = 6 * U * (dy.abs() @ A4)
    dz2 = dh2 * gz2
    e_dz2 = e_dh2 * gz2.abs() + dh2.abs() * e_gz2 + U * dz2.abs()
    dz2p, e_dz2p = _pad1(dz2), _pad1(e_dz2)
    # dh1[y, x] = sum_k w2[ky, kx] dz2[y - ky + 1, x - kx + 1]
    dh1, a1, e_dh1 = torch.zeros_like(h1), torch.zeros_like(h1), torch.zeros_like(h1)
    for k, (ky, kx) in enumerate(taps):
        dh1 += W2[:, k] * _tap(dz2p, S, 2 - ky, 2 - kx)
        a1 += A2[:, k] * _tap(dz2p, S, 2 - ky, 2 - kx).abs()
        e_dh1 += A2[:, k] * _tap(e_dz2p, S, 2 - ky, 2 - kx)
    e_dh1 += 12 * U * a1
    dz1 = dh1 * gz1
    e_dz1 = e_dh1 * gz1.abs() + dh1.abs() * e_gz1 + 2 * U * dz1.abs()
    ref["dx"] = (res * dy + dz1 @ W0).reshape(B, S, 3 * S)
    bound["dx"] = (e_dz1 @ A0 + (CH + 6) * U * (res * dy.abs() + dz1.abs() @ A0)).reshape(B, S, 3 * S)
    # weight gradients: value, sum of |terms|, sum of the terms' own errors
    s3 = lambda t: t.sum((0, 1, 2))
    ein = lambda a, b: torch.einsum("bhwo,bhwc->oc", a, b)
    grads = {
        "gb4": (s3(dy), s3(dy.abs()), torch.zeros(3, dtype=torch.float64)),
        "g4": (ein(dy, h2), ein(dy.abs(), h2.abs()), ein(dy.abs(), e_h2)),
        "gb2": (s3(dz2), s3(dz2.abs()), s3(e_dz2)),
        "gb0": (s3(dz1), s3(dz1.abs()), s3(e_dz1)),
        "g0": (ein(dz1, x), ein(dz1.abs(), x.abs()), ein(e_dz1, x.abs())),
    }
    g2 = [torch.empty(CH, 9, dtype=torch.float64) for _ in range(3)]
    for k, (ky, kx) in enumerate(taps):
        t, te = _tap(h1p, S, ky, kx), _tap(e_h1p, S, ky, kx)
        g2[0][:, k], g2[1][:, k] = s3(dz2 * t), s3((dz2 * t).abs())
        g2[2][:, k] = s3(e_dz2 * t.abs() + dz2.abs() * te)
    grads["g2"] = tuple(g2)
    depth = cnn_grad_depth(B, S)
    for name, _ in CNN_GRADS:
        val, absterms, own = (t.reshape(-1) for t in grads[name])
        init = d(name + "_init")
        ref[name] = init + val                                 # the kernel ADDS onto the caller's tensors
        bound[name] = own + depth * U * (absterms + init.abs())
    return ref, bound


def check_cnn(got, ref, bound, strict=True):
    """got: the outputs present in ref (out; dx and the six gradients).  -> (worst, failures)"""
    rep = _Report()
    for name in ref:
        rep.bounded(name, got[name].reshape(ref[name].shape), ref[name], bound[name])
    return rep.done(strict)


# ================================================================================================= 2. dwconv3x3
def _dw_flags(i):
    return dict(act=i & 1, y_pre=bool(i & 2), inv_scale=bool(i & 4), bias=bool(i & 8))


# every C x S; the four options cycle through all sixteen combinations over the sixteen cases
DWCONV_CASES = [dict(B=2 if S < 17 else 1, S=S, C=C, **_dw_flags(4 * ci + si))
                for ci, C in enumerate((1, 4, 32, 64)) for si, S in enumerate((1, 2, 3, 17))]
DWCONV_CASES.append(dict(B=2, S=182, C=32, act=1, y_pre=True, inv_scale=True, bias=True))   # above the 1024-workgroup clamp
DWCONV_UNSUPPORTED_C = (3, 128)


def dwconv_bwd_grid(B, S, C):
    g = max(1, min(2048, cdiv(B * S * S * C, DW_NT * 8)))
    return min(g, DW_BWD_MAX_GRID)


def dwconv_bwd_chain(B, S, C):
    """Addends between a dw / db element and its terms, whatever order the atomics land in: a thread's serial sum over
    its elements, the block's 256 / C threads of that channel (LDS atomics), the grid's blocks (global atomics, onto the
    initial content); + 2 for the product inside a term and the first add."""
    g = dwconv_bwd_grid(B, S, C)
    return cdiv(B * S * S * C, g * DW_NT) + DW_NT // C + g + 2


def dwconv_inputs(case, seed=0):
    B, S, C = case["B"], case["S"], case["C"]
    g = gen(100 * seed + 13 * S + C)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    ins = dict(x=rn(B, S, S, C, sc=2.0), dz=rn(B, S, S, C), w=rn(C, 9, sc=0.4), dw_init=rn(C, 9), db_init=rn(C))
    ins["x"].view(-1)[::7] *= 5.0                              # pre-activations beyond +-8 here and there
    ins["inv_scale"] = (0.7 + 0.6 * torch.rand(1, generator=g)) if case["inv_scale"] else None
    ins["bias"] = rn(C) if case["bias"] else None
    return ins


def dwconv_reference(ins, case):
    B, S, C = case["B"], case["S"], case["C"]
    x, dz, w = ins["x"].double(), ins["dz"].double(), ins["w"].double()
    sg = ins["inv_scale"].double() if ins["inv_scale"] is not None else torch.ones(1, dtype=torch.float64)
    bias = ins["bias"].double() if ins["bias"] is not None else torch.zeros(C, dtype=torch.float64)
    xp, dzp = _pad1(x), _pad1(dz)
    acc, a, dx, adx = (torch.zeros_like(x) for _ in range(4))
    dw, adw = torch.empty(C, 9, dtype=torch.float64), torch.empty(C, 9, dtype=torch.float64)
    for k, (ky, kx) in enumerate((ky, kx) for ky in range(3) for kx in range(3)):
        t = _tap(xp, S, ky, kx)
        acc += w[:, k] * t
        a += w[:, k].abs() * t.abs()
        dx += w[:, k] / sg * _tap(dzp, S, 2 - ky, 2 - kx)
        adx += w[:, k].abs() / sg * _tap(dzp, S, 2 - ky, 2 - kx).abs()
        dw[:, k], adw[:, k] = (dz * t).sum((0, 1, 2)), (dz * t).abs().sum((0, 1, 2))
    z = acc / sg + bias
    # 9 products and additions, the reciprocal of sigma, the scale, the bias: 13 U
    e_z = 13 * U * (a / sg + bias.abs())
    ref, bound = dict(y_pre=z), dict(y_pre=e_z)
    if case["act"]:
        ref["y"], bound["y"] = gelu64(z), GELU_D1_MAX * e_z + 2 * GELU_FWD_ERR * z.abs().clamp_min(1.0)
    else:
        ref["y"], bound["y"] = z, e_z
    ref["dx"], bound["dx"] = dx, 13 * U * adx
    chain = dwconv_bwd_chain(B, S, C)
    ref["dw"] = ins["dw_init"].double() + dw
    bound["dw"] = chain * U * (adw + ins["dw_init"].double().abs())
    ref["db"] = ins["db_init"].double() + dz.sum((0, 1, 2))
    bound["db"] = chain * U * (dz.abs().sum((0, 1, 2)) + ins["db_init"].double().abs())
    return ref, bound


def check_dwconv(got, ref, bound, strict=True):
    rep = _Report()
    for name in got:
        rep.bounded(name, got[name].reshape(ref[name].shape), ref[name], bound[name])
    return rep.done(strict)


# ================================================================================================= 3. token permutations
PERM_S = (1, 3, 31, 32, 33, 36)
PERM_B = (1, 3)
TRANSPOSE_MISALIGNED = [(2, 36, 1, 0), (2, 36, 0, 1), (1, 32, 1, 1)]     # B, S (S % 4 == 0), source / destination offset


def _bijc(B, S):
    return torch.meshgrid(torch.arange(B), torch.arange(S), torch.arange(S), torch.arange(3), indexing="ij")


def perm_index(kind, B, S):
    """The permutation as an index map over flat tensors: dst.flatten()[i] = src.flatten()[index[i]].
    image_to_rows : rows[b, i, 3 j + c] = img[b, c, i, j]
    rows_to_image : img[b, c, i, j]     = rows[b, i, 3 j + c]
    grid_transpose: out[b, j, 3 i + c]  = in[b, i, 3 j + c]"""
    b, i, j, c = _bijc(B, S)
    rows_at = ((b * S + i) * S + j) * 3 + c
    img_at = ((b * 3 + c) * S + i) * S + j
    rows_t_at = ((b * S + j) * S + i) * 3 + c
    dst, src = {"image_to_rows": (rows_at, img_at), "rows_to_image": (img_at, rows_at),
                "grid_transpose": (rows_t_at, rows_at)}[kind]
    index = torch.empty(B * S * S * 3, dtype=torch.long)
    index[dst.reshape(-1)] = src.reshape(-1)
    return index


def perm_shapes(kind, B, S):
    """(source shape, destination shape)"""
    rows, img = (B, S, 3 * S), (B, 3, S, S)
    return {"image_to_rows": (img, rows), "rows_to_image": (rows, img), "grid_transpose": (rows, rows)}[kind]


# ================================================================================================= 4. optimizer step
def optim_table():
    """One entry per tensor: dict(numel, sn = None | (rows, cols), goff = gradient offset in floats, kind).  The 300 tiny
    tensors sit in the middle, so tensors 256 onwards hold most of the gradient norm."""
    C = OPT_CHUNK
    t = [dict(numel=n, sn=None) for n in (1, 255, 257, C - 1)]
    t += [dict(numel=1 + (5 * k) % 7, sn=None) for k in range(300)]
    t += [dict(numel=n, sn=None) for n in (C, C + 1, 3 * C + 5)]
    t += [dict(numel=r * c, sn=(r, c)) for r, c in ((3, 32), (200, 1), (1, 300), (144, 288), (300, 260))]
    t += [dict(numel=64 * 48, sn=(64, 48), kind="cancel")]                   # G = alpha u v^T + 1e-3 noise
    t += [dict(numel=1000 + k, sn=None) for k in range(12)]
    for k, e in enumerate(t):
        e.setdefault("kind", "sn" if e["sn"] else "plain")
        e["goff"] = 1 if k % 3 == 1 else 0
    return t


def optim_chunks(table):
    """first chunk of every tensor and the number of chunks (OptimPlan's table)"""
    first, n = [], 0
    for e in table:
        first.append(n)
        n += cdiv(e["numel"], OPT_CHUNK)
    return first, n


def optim_row_split(e):
    """True when a chunk boundary of a spectral-norm tensor falls inside a row"""
    return e["sn"] is not None and e["numel"] > OPT_CHUNK and OPT_CHUNK % e["sn"][1] != 0


OPTIM_SCENARIOS = [
    # t_prev: plan.step_dev before the first of the two calls
    dict(name="no_clip_t1", max_norm=0.0, wd=0.0, t_prev=0, grad_scale=None, lr_dev=None),
    dict(name="clip_t1000", max_norm=1.0, wd=0.05, t_prev=999, grad_scale=None, lr_dev=None),
    dict(name="below_t2", max_norm=1000.0, wd=0.05, t_prev=1, grad_scale=None, lr_dev=None),
    dict(name="scaled_t100000", max_norm=1.0, wd=0.0, t_prev=99999, grad_scale=1024.0, lr_dev=None),
    dict(name="lr_dev", max_norm=1.0, wd=0.05, t_prev=0, grad_scale=None, lr_dev=3e-4),
]
OPT_LR, OPT_BETA1, OPT_BETA2, OPT_EPS = 1e-3, 0.9, 0.999, 1e-8
OPT_WRONG_LR = 0.5            # hp.lr when lr_dev is set: the device scalar must win
GRAD_SIGMA = 0.02             # ~235k elements: |g| ~ 10, so max_norm = 1 clips and max_norm = 1000 does not


def optim_hp(sc):
    """(lr, beta1, beta2, eps, weight_decay, max_norm, step) as handed to backend.optim_step"""
    return (OPT_WRONG_LR if sc["lr_dev"] is not None else OPT_LR, OPT_BETA1, OPT_BETA2, OPT_EPS, sc["wd"], sc["max_norm"], 0)


def optim_state(table, seed=0):
    """param, exp_avg (non-zero), exp_avg_sq (>= 0) and, for spectral-norm tensors, unit u and v and sigma in 0.7-1.3.
    The cancelling tensor's weight is sigma u v^T + noise, so that c = <G, W> / sigma ~ alpha."""
    g = gen(seed)
    recs = []
    for e in table:
        n = e["numel"]
        r = dict(param=torch.randn(n, generator=g) * 0.05, exp_avg=torch.randn(n, generator=g) * 0.01,
                 exp_avg_sq=(torch.randn(n, generator=g) * 0.01) ** 2, sn=None)
        if e["sn"]:
            rows, cols = e["sn"]
            u, v = torch.randn(rows, generator=g), torch.randn(cols, generator=g)
            u, v = u / u.norm(), v / v.norm()
            sigma = 0.7 + 0.6 * torch.rand(1, generator=g)
            if e["kind"] == "cancel":
                r["param"] = (sigma * torch.outer(u, v) + 0.01 * torch.randn(rows, cols, generator=g)).reshape(-1)
            r["sn"] = (u, v, sigma, rows, cols)
        recs.append(r)
    return recs


def optim_grads(table, recs, seed, scale=1.0):
    g = gen(seed)
    out = []
    for e, r in zip(table, recs):
        t = torch.randn(e["numel"], generator=g) * GRAD_SIGMA
        if e["kind"] == "cancel":
            u, v = r["sn"][0], r["sn"][1]
            t = (2.0 * torch.outer(u, v)).reshape(-1) + 1e-3 * torch.randn(e["numel"], generator=g)
        out.append(t * scale)
    return out


def f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))


def optim_sum_depth(numel):
    """A per-tensor sum: a thread's 64 serial adds of its chunk, the block (six shuffle levels and three adds of the
    wave sums), the tensor's chunks in order."""
    return OPT_CHUNK // OPT_NT + 9 + cdiv(numel, OPT_CHUNK)


def _pow_err(b, t):
    """1 - b^t in fp32: powf within one ulp (<= 2 U relative, or one flush to zero), the subtraction"""
    return 2 * U * b ** t + 2.0 ** -126 + U * (1 - b ** t)


def optim_reference(recs, grads, hp, grad_scale, step, lr_dev=None):
    """calm_optim_step in float64 from the fp32 values the ABI receives.  recs: the state BEFORE the call (fp32 CPU
    tensors), step: plan.step_dev before the call.  -> (ref, bound): ref holds gcorr (the corrected gradient per tensor),
    norm, clip, found_inf, step, and p, m, v as flat concatenations over the tensors; bound holds norm, p, m, v."""
    lr, b1, b2, eps, wd, max_norm = (f32(v) for v in hp[:6])
    if lr_dev is not None:
        lr = f32(lr_dev)
    inv_scale = 1.0 / f32(grad_scale) if grad_scale is not None else 1.0
    e_inv = U * inv_scale if grad_scale is not None else 0.0
    n = len(recs)
    gcorr, e_gcorr, n2s, e_n2s = [], [], [], []
    finite = True
    for r, g in zip(recs, grads):
        G = g.double().reshape(-1)
        finite = finite and bool(torch.isfinite(G).all())
        d = optim_sum_depth(G.numel())
        if r["sn"] is None:
            gc, e_gc = G, torch.zeros_like(G)
            n2 = (G * G).sum()
            e_n2 = (d + 1) * U * n2
        else:
            u, v, sigma, rows, cols = r["sn"]
            u, v, sg = u.double(), v.double(), float(sigma.double())
            G2, W = G.view(rows, cols), r["param"].double().view(rows, cols)
            uv = torch.outer(u, v)
            c = float((G2 * W).sum()) / sg                     # <G, W_orig / sigma>
            e_c = (d + 3) * U * float((G2 * W).abs().sum()) / sg
            guv, aguv = float((G2 * uv).sum()), float((G2 * uv).abs().sum())
            uu, vv, s2 = float(u @ u), float(v @ v), float((G2 * G2).sum())
            gc = ((G2 - c * uv) / sg).reshape(-1)
            # (G_ij - c u_i v_j) / sigma: c's error, two products, the difference, the reciprocal and the scale
            e_gc = ((e_c * uv.abs() + 4 * U * (G2.abs() + abs(c) * uv.abs())) / sg).reshape(-1) + 2 * U * gc.abs()
            n2 = (gc * gc).sum()
            # the kernel evaluates (|G|^2 - 2 c u^T G v + c^2 |u|^2 |v|^2) / sigma^2, which cancels: every part's error
            # counts against the parts' magnitudes (|G|^2 + 2 |c u^T G v| + c^2 |u|^2 |v|^2) / sigma^2, never against
            # their difference; the summation error of u^T G v itself against sum |g_ij u_i v_j| >= |u^T G v|
            du, dv = cdiv(rows, OPT_NT) + 10, cdiv(cols, OPT_NT) + 10
            parts = s2 + 2 * abs(c) * aguv + c * c * uu * vv
            e_n2 = ((d + 1) * U * s2 + 2 * e_c * abs(guv) + 2 * abs(c) * (d + 3) * U * aguv + 2 * abs(c) * e_c * uu * vv
                    + c * c * (du + dv) * U * uu * vv + 8 * U * parts) / (sg * sg)
        gcorr.append(gc), e_gcorr.append(e_gc), n2s.append(float(n2)), e_n2s.append(float(e_n2))
    total = sum(n2s)
    ref = dict(gcorr=gcorr, p=torch.cat([r["param"].double().reshape(-1) for r in recs]),
               m=torch.cat([r["exp_avg"].double() for r in recs]), v=torch.cat([r["exp_avg_sq"].double() for r in recs]))
    if not finite or not math.isfinite(total):
        ref.update(norm=math.nan, clip=math.nan, found_inf=1.0, step=step)
        return ref, {}
    # the tensors' norms: ceil(n / 256) serial adds per thread, then the block
    e_total = sum(e_n2s) + (cdiv(n, OPT_NT) + 9) * U * total
    root = math.sqrt(total)
    # |sqrt a - sqrt b| <= |a - b| / sqrt b and <= sqrt |a - b|
    e_root = min(e_total / root if root > 0 else 0.0, math.sqrt(e_total)) + U * root
    norm = root * inv_scale
    e_norm = e_root * inv_scale + root * e_inv + U * norm
    clip, e_clip = 1.0, 0.0
    if max_norm > 0:
        den = norm + f32(1e-6)
        ratio = max_norm / den
        e_ratio = ratio * (e_norm / den + 3 * U)
        clip = min(1.0, ratio)
        e_clip = e_ratio if ratio - e_ratio < 1.0 else 0.0     # min(1, .) is 1-Lipschitz
    mul = clip * inv_scale
    e_mul = e_clip * inv_scale + clip * e_inv + U * mul
    t = step + 1
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    r_bc1, r_bc2 = _pow_err(b1, t) / bc1, _pow_err(b2, t) / bc2
    step_size = lr / bc1
    r_step = r_bc1 / (1 - r_bc1) + U
    isb2 = 1 / math.sqrt(bc2)
    r_isb2 = (1 - r_bc2) ** -0.5 - 1 + 2 * U
    gc, e_gc = torch.cat(gcorr), torch.cat(e_gcorr)
    p0, m0, v0 = ref["p"], ref["m"], ref["v"]
    g = gc * mul
    e_g = e_gc * mul + gc.abs() * e_mul + U * g.abs()
    # m = m0 + (g - m0)(1 - b1): the difference, the product, the sum
    m = m0 + (g - m0) * (1 - b1)
    e_m = (1 - b1) * e_g + 4 * U * (m0.abs() + (1 - b1) * (g.abs() + m0.abs()))
    # v = v0 b2 + g^2 (1 - b2)
    v = v0 * b2 + g * g * (1 - b2)
    e_v = (1 - b2) * (2 * g.abs() * e_g + e_g * e_g) + 4 * U * v
    sv = v.sqrt()
    e_sv = torch.minimum(torch.where(sv > 0, e_v / sv.clamp_min(1e-300), torch.zeros_like(sv)), e_v.sqrt()) + U * sv
    denom = sv * isb2 + eps
    e_den = e_sv * isb2 + sv * isb2 * (r_isb2 + U) + U * denom
    upd = step_size * (m / denom)
    e_upd = step_size * (e_m / denom + m.abs() * e_den / (denom * (denom - e_den).clamp_min(1e-300))) \
        + upd.abs() * (r_step + 3 * U)
    # p = p0 (1 - lr wd) - upd: lr wd, the decay, the product, the difference
    p = p0 * (1 - lr * wd) - upd
    e_p = 4 * U * p0.abs() + e_upd + U * p.abs()
    ref.update(norm=norm, clip=clip, found_inf=0.0, step=t, p=p, m=m, v=v)
    return ref, dict(norm=e_norm, p=e_p, m=e_m, v=e_v)


def optim_flat(recs):
    """p, m, v of a list of records as flat concatenations (CPU)"""
    cat = lambda k: torch.cat([r[k].detach().cpu().reshape(-1) for r in recs])
    return dict(p=cat("param"), m=cat("exp_avg"), v=cat("exp_avg_sq"))


def check_optim(got, ref, bound, strict=True):
    """got: p, m, v (flat), norm, found_inf, step — of a step that was NOT skipped.  -> (worst, failures)"""
    rep = _Report()
    if got["found_inf"] != ref["found_inf"]:
        rep.fail("found_inf", f"got {got['found_inf']}, expected {ref['found_inf']}")
    if got["step"] != ref["step"]:
        rep.fail("step", f"step count {got['step']}, expected {ref['step']}")
    one = lambda x: torch.tensor([float(x)], dtype=torch.float64)
    rep.bounded("norm", one(got["norm"]), one(ref["norm"]), one(bound["norm"]))
    for k in ("p", "m", "v"):
        rep.bounded(k, got[k], ref[k], bound[k])
    return rep.done(strict)


def check_optim_skipped(got, before, step_before, strict=True):
    """A step with a non-finite gradient: found_inf raised, the step count and every bit of p, m, v as before."""
    rep = _Report()
    if got["found_inf"] != 1.0:
        rep.fail("found_inf", f"got {got['found_inf']}, expected 1")
    if got["step"] != step_before:
        rep.fail("step", f"step count {got['step']} after a skipped step, was {step_before}")
    for k in ("p", "m", "v"):
        if not torch.equal(got[k].view(torch.int32), before[k].view(torch.int32)):
            rep.fail(k, "changed by a skipped step")
    return rep.done(strict)


def optim_nonfinite_cases(table):
    """(name, tensor index, element index, value): inf as the last element of the last chunk of the multi-chunk tensor,
    NaN inside a spectral-norm tensor, -inf in a one-element tensor."""
    multi = next(i for i, e in enumerate(table) if e["numel"] == 3 * OPT_CHUNK + 5)
    sn = next(i for i, e in enumerate(table) if e["sn"] == (144, 288))
    single = next(i for i, e in enumerate(table) if e["numel"] == 1)
    return [("inf_last", multi, 3 * OPT_CHUNK + 4, math.inf), ("nan_sn", sn, 20000, math.nan),
            ("neg_inf_single", single, 0, -math.inf)]
