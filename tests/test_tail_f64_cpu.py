"""The checkers of tail_f64.py, proven without a GPU: an fp32 emulation of each kernel (torch fp32, with the kernel's
reduction grouping where the bound depends on it) must sit inside every bound at every case of the GPU tables, and every
planted fault must be rejected by the output it corrupts.  The float64 references themselves are compared with
independent float64 formulations (torch.optim.AdamW + clip_grad_norm_, EmulatedBackend._cnn and autograd)."""
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import tail_f64 as tf
from tail_f64 import CH, OPT_CHUNK, cdiv


def names(failures):
    return {n for n, _ in failures}


# ================================================================================================= emulations
def gelu32(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def gelu_grad32(x):
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]


def _tile_multiplicity(S, rows_only):
    """How many tiles count a pixel when the halo is not masked out of the weight gradients: every tile whose 18 x 18
    region holds it (rows_only: an `own` mask one pixel too wide at the top edge only)."""
    y = torch.arange(S)
    above = ((y % 16 == 15) & (y + 1 < S)).float()          # also in the halo of the tile below
    below = ((y % 16 == 0) & (y >= 16)).float()             # also in the halo of the tile above
    if rows_only:
        return (1 + above)[:, None] * torch.ones(S)[None, :]
    c = 1 + above + below
    return c[:, None] * c[None, :]


def emu_cnn(ins, B, S, residual, backward=True, fault=None):
    """fp32 emulation of calm_cnn_residual_fwd / _bwd: the kernel's formulas in torch fp32, the weight gradients summed
    per tile, the tiles of a workgroup in the order of its tile loop, then over the workgroups."""
    f = lambda k: ins[k].float()
    x = f("x").view(B, S, S, 3)
    W0, W2, W4 = f("w0").view(CH, 3) * (1 / f("s0")), f("w2").view(CH, 9) * (1 / f("s2")), f("w4").view(3, CH) * (1 / f("s4"))
    b0, b2, b4 = f("b0"), f("b2"), f("b4")
    res = 1.0 if residual else 0.0
    z1 = x @ W0.t() + b0
    h1 = gelu32(z1)
    if fault == "pad_x":                                       # zero padding applied to x: the border holds gelu(b0)
        h1p = gelu32(F.pad(x, (0, 0, 1, 1, 1, 1)) @ W0.t() + b0)
    else:
        h1p = tf._pad1(h1)
    W2f = W2.clone()
    if fault == "swap_taps":
        W2f[5] = W2[5].view(3, 3).t().reshape(9)
    z2 = b2.expand_as(h1).clone()
    for k, (ky, kx) in enumerate(TAPS):
        z2 = z2 + W2f[:, k] * tf._tap(h1p, S, ky, kx)
    h2 = gelu32(z2)
    got = dict(out=(h2 @ W4.t() + b4 + res * x).reshape(B, S, 3 * S))
    if not backward:
        return got
    dy = f("dy").view(B, S, S, 3)
    dz2 = (dy @ W4) * gelu_grad32(z2)
    dz2p = tf._pad1(dz2)
    dh1 = torch.zeros_like(h1)
    for k, (ky, kx) in enumerate(TAPS):
        dh1 = dh1 + W2[:, k] * tf._tap(dz2p, S, 2 - ky, 2 - kx)
    dz1 = dh1 * gelu_grad32(z1)
    res_dx = 1.0 - res if fault == "dx_skip" else res
    got["dx"] = (res_dx * dy + dz1 @ W0).reshape(B, S, 3 * S)
    cnt = torch.ones(S, S)
    if fault == "halo_counted":
        cnt = _tile_multiplicity(S, rows_only=False)
    elif fault == "own_wide":
        cnt = _tile_multiplicity(S, rows_only=True)
    cnt = cnt[None, :, :, None]
    dz2c = dz2 * cnt
    terms = torch.cat([
        (dz1[..., :, None] * x[..., None, :]).reshape(B, S, S, CH * 3),                               # g0[c, i]
        dz1,                                                                                           # gb0
        torch.stack([dz2c * tf._tap(h1p, S, ky, kx) for ky, kx in TAPS], -1).reshape(B, S, S, CH * 9),   # g2[c, k]
        dz2c,                                                                                          # gb2
        (dy[..., :, None] * h2[..., None, :]).reshape(B, S, S, 3 * CH),                               # g4[o, c]
        dy], -1)                                                                                       # gb4
    if fault == "drop_pixel":                                  # the last pixel of the last tile left out of every sum
        terms[B - 1, S - 1, S - 1] = 0.0
    tps = cdiv(S, 16)
    pad = tps * 16 - S
    per_tile = F.pad(terms, (0, 0, 0, pad, 0, pad)).view(B, tps, 16, tps, 16, -1).sum((2, 4)).reshape(B * tps * tps, -1)
    _, grid, per_wg = tf.cnn_grids(B, S)
    per_tile = F.pad(per_tile, (0, 0, 0, per_wg * grid - per_tile.shape[0])).view(per_wg, grid, -1)
    acc = torch.zeros(grid, per_tile.shape[-1])
    for k in range(per_wg):                                    # tile = workgroup + k * grid
        acc = acc + per_tile[k]
    total, at = acc.sum(0), 0
    for name, n in tf.CNN_GRADS:
        got[name] = f(name + "_init") + total[at:at + n]
        at += n
    return got


def emu_dwconv(ins, case):
    B, S, C = case["B"], case["S"], case["C"]
    x, dz, w = ins["x"], ins["dz"], ins["w"]
    sc = 1 / ins["inv_scale"] if ins["inv_scale"] is not None else torch.ones(1)
    xp, dzp = tf._pad1(x), tf._pad1(dz)
    acc, dx = torch.zeros_like(x), torch.zeros_like(x)
    dw = torch.empty(C, 9)
    for k, (ky, kx) in enumerate(TAPS):
        acc = acc + w[:, k] * tf._tap(xp, S, ky, kx)
        dx = dx + (w[:, k] * sc) * tf._tap(dzp, S, 2 - ky, 2 - kx)
        dw[:, k] = (dz * tf._tap(xp, S, ky, kx)).sum((0, 1, 2))
    z = acc * sc + (ins["bias"] if ins["bias"] is not None else 0.0)
    got = dict(y=gelu32(z) if case["act"] else z, dx=dx, dw=ins["dw_init"] + dw, db=ins["db_init"] + dz.sum((0, 1, 2)))
    if case["y_pre"]:
        got["y_pre"] = z
    return got


def emu_optim(recs, grads, hp, grad_scale, step, lr_dev=None, fault=None):
    """fp32 emulation of calm_optim_step: per-chunk partials added in chunk order, the tensors' norms, the update."""
    T = lambda v: torch.tensor(float(v), dtype=torch.float32)
    lr, b1, b2, eps, wd, max_norm = (T(v) for v in hp[:6])
    if lr_dev is not None:
        lr = T(lr_dev)
    inv_scale = 1 / T(grad_scale) if grad_scale is not None else T(1.0)
    serial = lambda parts: functools.reduce(lambda a, b: a + b, parts, T(0.0))
    n2s, cs, uvs, bad = [], [], [], False
    for r, g in zip(recs, grads):
        g = g.float().reshape(-1)
        bad = bad or not bool(torch.isfinite(g).all())
        parts = [(c * c).sum() for c in g.split(OPT_CHUNK)]
        if fault == "neighbour_chunk" and len(parts) > 2:
            parts[1] = parts[2]
        n2, c, uv = serial(parts), None, None
        if r["sn"] is not None:
            u, v, sigma, rows, cols = r["sn"]
            uv = torch.outer(u, v).reshape(-1)
            if fault == "swap_rc" and rows != cols and min(rows, cols) > 1:
                uv = torch.outer(v, u).reshape(-1)             # element i takes v[i // rows] u[i % rows]
            gw = serial([(a * b).sum() for a, b in zip(g.split(OPT_CHUNK), r["param"].reshape(-1).split(OPT_CHUNK))])
            guv = serial([(a * b).sum() for a, b in zip(g.split(OPT_CHUNK), uv.split(OPT_CHUNK))])
            uu, vv, sg = (u * u).sum(), (v * v).sum(), sigma[0]
            c = gw / sg
            n2 = (n2 - 2 * c * guv + (0.0 if fault == "drop_uuvv" else c * c * uu * vv)) / (sg * sg)
        n2s.append(n2.clamp_min(0.0)), cs.append(c), uvs.append(uv)
    acc = torch.stack(n2s[:256] if fault == "first_256" else n2s).sum()
    norm = acc.sqrt() * inv_scale
    bad = bad or not bool(torch.isfinite(norm))
    state = copy.deepcopy(recs)
    if bad:
        return dict(tf.optim_flat(state), norm=float(norm), found_inf=1.0, step=step + (1 if fault == "step_on_skip" else 0))
    clip = torch.minimum(T(1.0), max_norm / (norm + T(1e-6))) if float(max_norm) > 0 else T(1.0)
    mul = clip if fault == "no_inv_scale" else clip * inv_scale
    t = step + 1
    te = T(t - 1 if fault == "t_minus_1" else t)
    decay = 1 - lr * wd
    bc1, bc2 = 1 - torch.pow(b1, te), 1 - torch.pow(b2, te)
    step_size, isb2 = lr / bc1, 1 / bc2.sqrt()
    for r, g, c, uv in zip(state, grads, cs, uvs):
        g = g.float().reshape(-1)
        if c is not None:
            g = (g - c * uv) * (1 / r["sn"][2][0])
        gv = g * inv_scale if fault == "v_unclipped" else g * mul
        g = g * mul
        old = {k: r[k].clone() for k in ("param", "exp_avg", "exp_avg_sq")}
        p = r["param"].reshape(-1) * decay
        m = r["exp_avg"] + (g - r["exp_avg"]) * (1 - b1)
        v = r["exp_avg_sq"] * b2 + gv * gv * (1 - b2)
        p = p - step_size * (m / (v.sqrt() * isb2 + eps))
        r["param"], r["exp_avg"], r["exp_avg_sq"] = p, m, v
        if fault == "skip_last" and g.numel() == OPT_CHUNK + 1:
            for k in old:
                r[k][-1] = old[k].reshape(-1)[-1]
    return dict(tf.optim_flat(state), norm=float(norm), found_inf=0.0, step=t)


# ================================================================================================= CNN tail
@functools.lru_cache(maxsize=None)
def cnn_case(B, S, residual, backward=True):
    ins = tf.cnn_inputs(B, S)
    return (ins,) + tf.cnn_reference(ins, B, S, residual, backward)


CPU_CNN_CASES = tf.CNN_CASES          # the large-B cases too: the whole file takes well under a minute


@pytest.mark.parametrize("residual", [1, 0])
@pytest.mark.parametrize("B,S,backward", CPU_CNN_CASES)
def test_cnn_emulation_inside_every_bound(B, S, backward, residual):
    ins, ref, bound = cnn_case(B, S, residual, backward)
    worst, _ = tf.check_cnn(emu_cnn(ins, B, S, residual, backward), ref, bound)
    print(f"cnn B={B} S={S} res={residual}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert set(worst) == set(ref)


CNN_FAULTS = [
    # fault, (B, S), residual, outputs that must reject it
    ("pad_x", (1, 15), 1, {"out"}),
    ("swap_taps", (1, 15), 1, {"out"}),
    ("halo_counted", (1, 17), 1, {"g2", "gb2"}),
    ("own_wide", (1, 33), 1, {"g2", "gb2"}),
    ("dx_skip", (1, 15), 1, {"dx"}),
    ("dx_skip", (1, 15), 0, {"dx"}),
]


@pytest.mark.parametrize("fault,shape,residual,rejected_by", CNN_FAULTS)
def test_cnn_planted_fault_in_the_emulation(fault, shape, residual, rejected_by):
    B, S = shape
    ins, ref, bound = cnn_case(B, S, residual)
    _, failures = tf.check_cnn(emu_cnn(ins, B, S, residual, fault=fault), ref, bound, strict=False)
    assert rejected_by <= names(failures), failures


def test_cnn_one_pixel_of_520_tiles_left_out_of_the_weight_gradients():
    """The depth of the sums grows with the tile count and the bound with it: at the largest backward case one pixel
    of 37 570 missing from the sums must still be rejected by each of the six gradients."""
    ins, ref, bound = cnn_case(130, 17, 1)
    _, failures = tf.check_cnn(emu_cnn(ins, 130, 17, 1, fault="drop_pixel"), ref, bound, strict=False)
    assert names(failures) == {n for n, _ in tf.CNN_GRADS}, failures


def test_cnn_swapped_taps_in_the_weight_gradient():
    ins, ref, bound = cnn_case(1, 17, 1)
    got = emu_cnn(ins, 1, 17, 1)
    g2 = got["g2"].clone().view(CH, 9)
    g2[5] = g2[5].view(3, 3).t().reshape(9)
    _, failures = tf.check_cnn(dict(got, g2=g2.reshape(-1)), ref, bound, strict=False)
    assert names(failures) == {"g2"}


def test_cnn_second_tile_of_a_workgroup_from_the_first_tiles_region():
    """Tile t >= gridDim.x computed from the region prefetched for tile t - gridDim.x: backward at 260 tiles (grid 256:
    sample 64 from sample 0's x and dy), forward at 1540 tiles (grid 1536: sample 384 from sample 0's x)."""
    B, S = 65, 17
    ins, ref, bound = cnn_case(B, S, 1)
    stale = dict(ins, x=ins["x"].clone(), dy=ins["dy"].clone())
    stale["x"][64], stale["dy"][64] = ins["x"][0], ins["dy"][0]
    _, failures = tf.check_cnn(emu_cnn(stale, B, S, 1), ref, bound, strict=False)
    assert {"out", "dx"} <= names(failures)
    B = 385
    ins, ref, bound = cnn_case(B, S, 1, False)
    stale = dict(ins, x=ins["x"].clone())
    stale["x"][384] = ins["x"][0]
    _, failures = tf.check_cnn(emu_cnn(stale, B, S, 1, False), ref, bound, strict=False)
    assert names(failures) == {"out"}


@pytest.mark.parametrize("name", [n for n, _ in tf.CNN_GRADS])
def test_cnn_gradient_overwritten_instead_of_added(name):
    ins, ref, bound = cnn_case(3, 20, 1)
    got = emu_cnn(ins, 3, 20, 1)
    got[name] = got[name] - ins[name + "_init"]
    _, failures = tf.check_cnn(got, ref, bound, strict=False)
    assert names(failures) == {name}


def test_cnn_one_stale_element():
    """An element of out never written (still the NaN fill), and one that holds its neighbour pixel's value."""
    ins, ref, bound = cnn_case(1, 17, 1)
    got = emu_cnn(ins, 1, 17, 1)
    for value in (torch.tensor(tf.FILL[torch.float32], dtype=torch.int32).view(torch.float32), got["out"][0, 16, 45]):
        out = got["out"].clone()
        out[0, 16, 48] = value
        _, failures = tf.check_cnn(dict(got, out=out), ref, bound, strict=False)
        assert names(failures) == {"out"}


def test_cnn_one_tile_edge_pixel_off_by_one_percent():
    ins, ref, bound = cnn_case(1, 33, 1)
    got = emu_cnn(ins, 1, 33, 1)
    for name in ("out", "dx"):
        t = got[name].clone()
        t[0, 16, 3 * 15 + 1] *= 1.01
        _, failures = tf.check_cnn({**got, name: t}, ref, bound, strict=False)
        assert names(failures) == {name}


@pytest.mark.parametrize("residual", [1, 0])
def test_cnn_reference_against_the_emulated_backend_in_float64(residual):
    """The closed-form float64 reference against EmulatedBackend._cnn (conv2d) and its autograd, both in float64."""
    from emulated_backend import EmulatedBackend
    B, S = 3, 20
    ins, ref, bound = cnn_case(B, S, residual)
    zero = {k + "_init": torch.zeros_like(ins[k + "_init"]) for k, _ in tf.CNN_GRADS}
    ref, _ = tf.cnn_reference({**ins, **zero}, B, S, residual)
    d = {k: ins[k].double() for k in tf.CNN_W}
    x = ins["x"].double().requires_grad_(True)
    eff = {k: (d[k] / d["s" + k[1]]).requires_grad_(True) for k in ("w0", "w2", "w4")}
    bias = {k: d[k].clone().requires_grad_(True) for k in ("b0", "b2", "b4")}
    one = torch.ones(1, dtype=torch.float64)
    out = EmulatedBackend._cnn(x, eff["w0"], one, bias["b0"], eff["w2"], one, bias["b2"], eff["w4"], one, bias["b4"],
                               B, S, CH, bool(residual))
    plain = EmulatedBackend._cnn(x.detach(), *(d[k] for k in tf.CNN_W), B, S, CH, bool(residual))
    rel = lambda a, b: float((a.reshape(-1) - b.reshape(-1)).abs().max() / b.abs().max())
    assert rel(plain, ref["out"]) <= 1e-12 and rel(out.detach(), ref["out"]) <= 1e-12
    gr = torch.autograd.grad(out, (x, eff["w0"], bias["b0"], eff["w2"], bias["b2"], eff["w4"], bias["b4"]), ins["dy"].double())
    for name, g in zip(("dx", "g0", "gb0", "g2", "gb2", "g4", "gb4"), gr):
        assert rel(g, ref[name]) <= 1e-12, name


def test_cnn_table_reaches_what_it_claims():
    tiles = {(B, S): tf.cnn_tiles(B, S) for B, S, _ in tf.CNN_CASES}
    assert tiles[(1, 15)] == tiles[(1, 16)] == 1 and tiles[(1, 17)] == 4 and tiles[(1, 33)] == 9
    assert tiles[(65, 17)] == 260 > tf.CNN_BWD_MAX_GRID and tf.cnn_grids(65, 17) == (260, 256, 2)
    assert tiles[(130, 17)] == 520 and tf.cnn_grids(130, 17)[2] == 3 and 520 - 2 * 256 == 8     # workgroups 0-7: three
    assert tiles[(385, 17)] == 1540 > tf.CNN_FWD_MAX_GRID and tf.cnn_grids(385, 17)[0] == 1536
    assert all(bwd for B, S, bwd in tf.CNN_CASES if B != 385)
    # the inputs hold what the cases are about: pre-activations beyond +-8, an all-zero sample, gelu(b0) != 0
    ins = tf.cnn_inputs(3, 20)
    z1 = ins["x"].view(3, 20, 20, 3).double() @ (ins["w0"].double() / ins["s0"].double()).t() + ins["b0"].double()
    assert float(z1.abs().max()) > 8 and not ins["x"][1].any() and float(ins["b0"].abs().min()) > 0
    assert all(0.7 <= float(ins[k]) <= 1.3 for k in ("s0", "s2", "s4"))


# ================================================================================================= dwconv3x3
@pytest.mark.parametrize("case", tf.DWCONV_CASES, ids=lambda c: "B{B}-S{S}-C{C}-a{act}".format(**c))
def test_dwconv_emulation_inside_every_bound(case):
    ins = tf.dwconv_inputs(case)
    ref, bound = tf.dwconv_reference(ins, case)
    got = emu_dwconv(ins, case)
    worst, _ = tf.check_dwconv(got, ref, bound)
    print("dwconv {B}x{S}x{C}: ".format(**case) + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    if case["S"] == 17 and case["C"] == 32:
        # planted: ky / kx swapped in one channel's weight gradient, the bias gradient overwritten, a stale dx element
        dw = got["dw"].clone()
        dw[3] = dw[3].view(3, 3).t().reshape(9)
        dx = got["dx"].clone()
        dx[0, 16, 16, 31] = got["dx"][0, 16, 15, 31]
        for name, t in (("dw", dw), ("db", got["db"] - ins["db_init"]), ("dx", dx)):
            _, failures = tf.check_dwconv({**got, name: t}, ref, bound, strict=False)
            assert names(failures) == {name}


def test_dwconv_table_reaches_what_it_claims():
    flags = {(c["act"], c["y_pre"], c["inv_scale"], c["bias"]) for c in tf.DWCONV_CASES}
    assert len(flags) == 16
    assert {(c["C"], c["S"]) for c in tf.DWCONV_CASES} >= {(C, S) for C in (1, 4, 32, 64) for S in (1, 2, 3, 17)}
    assert cdiv(2 * 182 * 182 * 32, tf.DW_NT * 8) > tf.DW_BWD_MAX_GRID == tf.dwconv_bwd_grid(2, 182, 32)
    assert all(C > tf.DW_MAXC or tf.DW_NT % C for C in tf.DWCONV_UNSUPPORTED_C)


# ================================================================================================= permutations
@pytest.mark.parametrize("kind", ["image_to_rows", "rows_to_image", "grid_transpose"])
def test_permutation_index_maps(kind):
    for B in tf.PERM_B:
        for S in tf.PERM_S:
            src_shape, dst_shape = tf.perm_shapes(kind, B, S)
            src = torch.arange(B * S * S * 3, dtype=torch.float32).view(src_shape)
            dst = src.reshape(-1)[tf.perm_index(kind, B, S)].view(dst_shape)
            if kind == "image_to_rows":
                want = src.permute(0, 2, 3, 1).reshape(dst_shape)
            elif kind == "rows_to_image":
                want = src.view(B, S, S, 3).permute(0, 3, 1, 2)
            else:
                want = src.view(B, S, S, 3).transpose(1, 2).reshape(dst_shape)
            assert torch.equal(dst, want)
    assert all(S % 4 == 0 and (so or do) for _, S, so, do in tf.TRANSPOSE_MISALIGNED)


# ================================================================================================= optimizer
TABLE = tf.optim_table()


@functools.lru_cache(maxsize=None)
def optim_case(name):
    """(scenario, state before, gradients, reference, bound) of a scenario's first call"""
    sc = next(s for s in tf.OPTIM_SCENARIOS if s["name"] == name)
    recs = tf.optim_state(TABLE)
    grads = tf.optim_grads(TABLE, recs, seed=1, scale=sc["grad_scale"] or 1.0)
    ref, bound = tf.optim_reference(recs, grads, tf.optim_hp(sc), sc["grad_scale"], sc["t_prev"], sc["lr_dev"])
    return sc, recs, grads, ref, bound


def run_emu(name, fault=None):
    sc, recs, grads, ref, bound = optim_case(name)
    return emu_optim(recs, grads, tf.optim_hp(sc), sc["grad_scale"], sc["t_prev"], sc["lr_dev"], fault)


@pytest.mark.parametrize("name", [s["name"] for s in tf.OPTIM_SCENARIOS])
def test_optim_emulation_inside_every_bound(name):
    """Two consecutive calls; the reference of the second starts from the emulation's state after the first."""
    sc, recs, grads, ref, bound = optim_case(name)
    got = run_emu(name)
    worst, _ = tf.check_optim(got, ref, bound)
    print(f"optim {name} call 1: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    at, state = 0, copy.deepcopy(recs)
    for r in state:
        n = r["param"].numel()
        r["param"], r["exp_avg"], r["exp_avg_sq"] = (got[k][at:at + n].clone() for k in ("p", "m", "v"))
        at += n
    grads2 = tf.optim_grads(TABLE, state, seed=2, scale=sc["grad_scale"] or 1.0)
    hp = tf.optim_hp(sc)
    ref2, bound2 = tf.optim_reference(state, grads2, hp, sc["grad_scale"], got["step"], sc["lr_dev"])
    worst, _ = tf.check_optim(emu_optim(state, grads2, hp, sc["grad_scale"], got["step"], sc["lr_dev"]), ref2, bound2)
    print(f"optim {name} call 2: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert ref2["step"] == sc["t_prev"] + 2


OPTIM_FAULTS = [
    # fault, scenario, outputs that must reject it
    ("skip_last", "clip_t1000", {"p", "m", "v"}),
    ("neighbour_chunk", "clip_t1000", {"norm"}),
    ("swap_rc", "no_clip_t1", {"p", "m", "v"}),
    ("drop_uuvv", "clip_t1000", {"norm"}),
    ("no_inv_scale", "scaled_t100000", {"p", "m", "v"}),
    ("t_minus_1", "clip_t1000", {"p"}),
    ("t_minus_1", "below_t2", {"p"}),
    ("v_unclipped", "clip_t1000", {"v"}),
    ("first_256", "clip_t1000", {"norm"}),
]


@pytest.mark.parametrize("fault,name,rejected_by", OPTIM_FAULTS)
def test_optim_planted_fault(fault, name, rejected_by):
    sc, recs, grads, ref, bound = optim_case(name)
    _, failures = tf.check_optim(run_emu(name, fault), ref, bound, strict=False)
    assert rejected_by <= names(failures), failures


def test_optim_lr_dev_must_override_hp_lr():
    sc, recs, grads, ref, bound = optim_case("lr_dev")
    got = emu_optim(recs, grads, tf.optim_hp(sc), None, sc["t_prev"], None)        # hp.lr (wrong on purpose) used
    assert "p" in names(tf.check_optim(got, ref, bound, strict=False)[1])


@pytest.mark.parametrize("kinds", [("sn", "cancel"), ("cancel",)], ids=["spectral_only", "cancelling_only"])
def test_optim_deferred_correction_norm_alone(kinds):
    """Plans of spectral-norm tensors only: the reported norm is the deferred-correction norm on its own.  With the
    cancelling tensor alone the parts cancel to 1e-3 of themselves; the bound, relative to the parts, still rejects a
    norm without its |u|^2 |v|^2 term (which the kernel's clamp would turn into 0)."""
    keep = [i for i, e in enumerate(TABLE) if e["kind"] in kinds]
    sc, recs, grads, _, _ = optim_case("clip_t1000")
    recs, grads, hp = [recs[i] for i in keep], [grads[i] for i in keep], tf.optim_hp(sc)
    ref, bound = tf.optim_reference(recs, grads, hp, None, sc["t_prev"])
    worst, _ = tf.check_optim(emu_optim(recs, grads, hp, None, sc["t_prev"]), ref, bound)
    print(f"optim {'+'.join(kinds)}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()) +
          f" (norm {ref['norm']:.4g} +- {bound['norm']:.2g})")
    _, failures = tf.check_optim(emu_optim(recs, grads, hp, None, sc["t_prev"], fault="drop_uuvv"), ref, bound, strict=False)
    assert "norm" in names(failures)


@pytest.mark.parametrize("case", tf.optim_nonfinite_cases(TABLE), ids=lambda c: c[0])
def test_optim_skipped_step(case):
    _, tensor, element, value = case
    sc, recs, grads, _, _ = optim_case("clip_t1000")
    grads = [g.clone() for g in grads]
    grads[tensor][element] = value
    before = tf.optim_flat(recs)
    ref, _ = tf.optim_reference(recs, grads, tf.optim_hp(sc), None, sc["t_prev"])
    assert ref["found_inf"] == 1.0 and ref["step"] == sc["t_prev"]
    tf.check_optim_skipped(emu_optim(recs, grads, tf.optim_hp(sc), None, sc["t_prev"]), before, sc["t_prev"])
    got = emu_optim(recs, grads, tf.optim_hp(sc), None, sc["t_prev"], fault="step_on_skip")
    assert names(tf.check_optim_skipped(got, before, sc["t_prev"], strict=False)[1]) == {"step"}
    got = dict(got, step=sc["t_prev"], p=before["p"].clone())
    got["p"][-1] = torch.nextafter(got["p"][-1], torch.tensor(math.inf))
    assert names(tf.check_optim_skipped(got, before, sc["t_prev"], strict=False)[1]) == {"p"}


@pytest.mark.parametrize("name", [s["name"] for s in tf.OPTIM_SCENARIOS])
def test_optim_reference_against_torch_adamw_in_float64(name):
    """torch.optim.AdamW + clip_grad_norm_ in float64 on the corrected gradients and the same fp32-rounded
    hyper-parameters: 1e-12 relative."""
    sc, recs, grads, ref, _ = optim_case(name)
    lr, b1, b2, eps, wd, max_norm = (tf.f32(v) for v in tf.optim_hp(sc)[:6])
    if sc["lr_dev"] is not None:
        lr = tf.f32(sc["lr_dev"])
    params = [torch.nn.Parameter(r["param"].double().reshape(-1).clone()) for r in recs]
    opt = torch.optim.AdamW(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    for p, r, g in zip(params, recs, ref["gcorr"]):
        p.grad = g / (tf.f32(sc["grad_scale"]) if sc["grad_scale"] else 1.0)
        opt.state[p] = dict(step=torch.tensor(float(sc["t_prev"])), exp_avg=r["exp_avg"].double().clone(),
                            exp_avg_sq=r["exp_avg_sq"].double().clone())
    if max_norm > 0:
        norm = torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
    else:
        norm = torch.cat([p.grad for p in params]).norm()
    opt.step()
    assert abs(float(norm) - ref["norm"]) <= 1e-12 * ref["norm"]
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    assert rel(torch.cat([p.detach() for p in params]), ref["p"]) <= 1e-12
    assert rel(torch.cat([opt.state[p]["exp_avg"] for p in params]), ref["m"]) <= 1e-12
    assert rel(torch.cat([opt.state[p]["exp_avg_sq"] for p in params]), ref["v"]) <= 1e-12
    assert int(opt.state[params[0]]["step"]) == ref["step"]
    assert (ref["clip"] < 1) == (sc["max_norm"] == 1.0)


def test_optim_table_reaches_what_it_claims():
    first, n_chunks = tf.optim_chunks(TABLE)
    assert len(TABLE) > 256 and 300 <= len(TABLE) <= 350 and 200_000 <= sum(e["numel"] for e in TABLE) <= 300_000
    plain = {e["numel"] for e in TABLE if e["sn"] is None}
    assert {1, 255, 257, OPT_CHUNK - 1, OPT_CHUNK, OPT_CHUNK + 1, 3 * OPT_CHUNK + 5} <= plain
    sn = {e["sn"]: e for e in TABLE if e["sn"]}
    assert {(3, 32), (200, 1), (1, 300), (144, 288), (300, 260)} <= set(sn)
    assert tf.optim_row_split(sn[(144, 288)]) and tf.optim_row_split(sn[(300, 260)])
    assert any(r > 256 and c > 256 for r, c in sn)
    # tensors past the finalize kernel's 256 threads hold most of the norm, gradients at a one-float offset exist
    assert sum(e["numel"] for e in TABLE[256:]) > sum(e["numel"] for e in TABLE[:256])
    assert any(e["goff"] for e in TABLE) and any(e["goff"] and e["sn"] for e in TABLE)
    assert {s["t_prev"] + 1 for s in tf.OPTIM_SCENARIOS} >= {1, 2, 1000, 100000}
    # the cancelling tensor cancels: its corrected norm is far below the parts the kernel subtracts
    sc, recs, grads, ref, _ = optim_case("no_clip_t1")
    i = next(i for i, e in enumerate(TABLE) if e["kind"] == "cancel")
    assert float((ref["gcorr"][i] ** 2).sum()) < 1e-2 * float((grads[i].double() ** 2).sum())
