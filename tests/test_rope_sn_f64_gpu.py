"""The RoPE kernels (rope_table_kernel, calm_rope_fwd, calm_rope_bwd, calm_part_rope_bwd of csrc/norm_act.hip) and the
spectral-norm kernels (calm_sn_plan / calm_sn_power_iter, calm_sn_weight_bwd, calm_sn_weight_bwd_batch of
csrc/spectral.hip) of libcalmvit_hip.so against the float64 references of rope_sn_f64.py, element by element, at the case
tables defined there.  tests/test_rope_sn_f64_cpu.py proves the same checkers on an fp32 emulation and on planted faults.
Every output (the scratch buffers and rows of partials included) sits between NaN-pattern guards; outputs that accumulate
start from non-zero contents.  Each case prints its worst error / bound per output.

cosf / sinf of the table kernel against float64 cos / sin of the fp32 angle, measured once on an MI355X over 3 x 2^20
(s, j) pairs (S = 4096, 256 frequencies up to 0.125: angles in [0, 512] rad); the ROCm tree documents no bound for them:
    max |cos - cos_f64| = 6.94e-8 (1.53 ulp of the result), max |sin - sin_f64| = 7.03e-8 (1.53 ulp)
    by angle range, the larger of the two:  [0, 1) 5.97e-8   [1, 8) 6.66e-8   [8, 64) 6.77e-8   [64, 128) 6.97e-8
                                            [128, 256) 7.03e-8   [256, 384) 6.84e-8   [384, 512] 6.75e-8
No growth with the angle: the argument reduction holds over the whole range (in ulps of the result 1.50 - 1.53 from 1 rad
on, 1.0 below).  The test asserts no more than twice rope_sn_f64.TABLE_ERR = 7.03e-8.

Worst error / bound per output over all cases of the one run on an MI355X:
    RoPE    table 0.444   out (fp32) 0.646   d_xr (fp32) 0.649   d_inv_freq 0.088   partials' sum 0.055
            content / d_content bit-exact; bf16 out / d_xr 0.996 of (fp32 bound + half a bf16 ulp), i.e. the rounding
            itself, with at least 99 % of the elements equal to the rounded reference
            (d_inv_freq's bound is a worst case over a depth of 29 - 73 where signed errors add like a square root)
    power iteration, training   t 0.117   v 0.211   s 0.219   u 0.190   sigma 0.173
    power iteration, eval       s 0.223   sigma 0.087 (on the kernel's s)   sigma 0.045 (against u . (W v))
    known spectrum, 20 iterations   sigma 0.060   |u . u1| 0.106   |v . v1| 0.109
    weight gradient   dW 0.391   d_ls 0.250   (the batched form: the same bits)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import rope_sn_f64 as rs
from rope_sn_f64 import F32
from test_rowwise_f64_gpu import DEV, Out, _bits, place

pytestmark = pytest.mark.gpu
L = calm.backend._lib
_st, _stream = calm.backend._st, calm.backend._stream


@pytest.fixture(scope="module")
def hip():
    return calm.backend.get_backend()


def show(label, worst):
    print(f"\n[rope_sn_f64] {label}: " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))


def untouched(*outs):
    torch.cuda.synchronize()
    return all(torch.equal(_bits(o.buf).cpu(), o.before) for o in outs if o is not None)


def ptr(t):
    return None if t is None else t.data_ptr()


# ================================================================================================= RoPE
def dims(case):
    return tuple(case[k] for k in ("B", "S", "H", "dc", "dr"))


def rope_forward(hip, case, ins, offs=None):
    """-> (got, device tensors the backward takes, vw the host must have chosen)"""
    offs = offs or {}
    B, S, H, dc, dr = dims(case)
    _, tout = rs.ROPE_TYPES[case["types"]]
    content = place(ins["content"], offs.get("content", 0)) if dc else None
    xr, inv = place(ins["xr"], offs.get("xr", 0)), place(ins["inv_freq"])
    T, O = Out((2, S, dr // 2), off=offs.get("table", 0)), Out((B, S, H * (dc + dr)), tout, off=offs.get("out", 0))
    hip.rope_fwd(content, xr, inv, T.t, O.t, B, S, H, dc, dr)
    vw = rs.rope_vw(dc, dr, [(t.data_ptr(), t.element_size()) for t in (content, xr, O.t, T.t) if t is not None])
    return dict(table=T.check(), out=O.check()), dict(xr=xr, table=T.t), vw


def rope_backward(hip, case, ins, dev, offs=None, part=False):
    """calm_rope_bwd (d_inv_freq onto d0) or, part=True, calm_part_rope_bwd into guarded rows of partials"""
    offs = offs or {}
    B, S, H, dc, dr = dims(case)
    tin, _ = rs.ROPE_TYPES[case["types"]]
    half, nrows = dr // 2, B * S * H
    g = place(ins["g"], offs.get("d_out", 0))
    DC = Out((B, S, H * dc), tin, off=offs.get("d_content", 0)) if dc else None
    DX = Out((B, S, H * dr), tin, off=offs.get("d_xr", 0))
    dct = DC.t if dc else None
    vw = rs.rope_vw(dc, dr, [(t.data_ptr(), t.element_size()) for t in (g, dev["xr"], dev["table"], dct, DX.t)
                             if t is not None])
    got = {}
    if part:
        need = int(hip.lib.calm_reduce_scratch_floats(L.RED_ROPE_BWD, nrows, dr))
        assert need == rs.ROPE_SCRATCH_ROWS * half
        P, shape = Out((need,)), L.ReduceShape()
        rc = hip.lib.calm_part_rope_bwd(ptr(g), ptr(dev["xr"]), ptr(dev["table"]), ptr(dct), ptr(DX.t), B, S, H, dc, dr,
                                        _st(g), _st(dev["xr"]), _st(dct), _st(DX.t), ptr(P.t), C.byref(shape), _stream())
        assert rc == 0
        assert (shape.G, shape.n, shape.stride, shape.nseg) == (rs.rope_bwd_grid(nrows, dr, vw), half, half, 1)
        flat = P.check(written=False)
        fill = torch.full((1,), rs.FILL[F32], dtype=torch.int32)
        assert not bool((flat[:shape.G * half].view(torch.int32) == fill).any()), "a row of partials not written"
        assert bool((flat[shape.G * half:].view(torch.int32) == fill).all()), "a write past the rows of partials"
        got["part"] = flat[:shape.G * half].view(shape.G, half)
    else:
        DF = Out((half,), init=ins["d0"])
        hip.rope_bwd(g, dev["xr"], dev["table"], dct, DX.t, DF.t, B, S, H, dc, dr)
        got["d_inv_freq"] = DF.check(written=False)
    got["d_xr"] = DX.check()
    if dc:
        got["d_content"] = DC.check()
    return got, vw


def rope_all(hip, case, ins, label, exact=False, offs=None):
    """forward, calm_rope_bwd, calm_part_rope_bwd; every checker; -> the vw of the forward and of the backward"""
    got, dev, vw_f = rope_forward(hip, case, ins, offs)
    worst, failures = rs.check_rope_forward(case, ins, got, strict=False, exact=exact)
    table = got["table"]
    full, vw_b = rope_backward(hip, case, ins, dev, offs)
    w, f = rs.check_rope_backward(case, ins, table, full, vw_b, strict=False, exact=exact)
    worst.update(w)
    failures += f
    part, vw_p = rope_backward(hip, case, ins, dev, offs, part=True)
    w, f = rs.check_rope_backward(case, ins, table, part, vw_p, strict=False, exact=exact, d0=False)
    worst["part"] = w.get("part", float("inf"))
    failures += [x for x in f if x[0] == "part"]
    show(label, worst)
    assert not failures, failures
    assert vw_p == vw_b
    for k in ("d_xr", "d_content"):                          # the two backward entry points share the first launch
        if k in full:
            assert torch.equal(_bits(full[k]), _bits(part[k])), f"{k} of calm_part_rope_bwd differs from calm_rope_bwd's"
    return vw_f, vw_b


@pytest.mark.parametrize("case", rs.ROPE_CASES, ids=rs.rope_id)
def test_rope(hip, case):
    vw_f, vw_b = rope_all(hip, case, rs.rope_inputs(case), "rope " + rs.rope_id(case))
    assert vw_f == vw_b == rs.rope_vw_shape(case["dc"], case["dr"])          # aligned tensors: the instance of the shape


@pytest.mark.parametrize("case", [c for c in rs.ROPE_CASES if c["types"] in ("f32", "bf16")], ids=rs.rope_id)
def test_rope_exact_on_integers(hip, case):
    """inv_freq = 0 and small integers: out, d_xr, the partials' sum and d_inv_freq = d0 + sum s (g2 x1 - g1 x2) are
    integers, exact in any order: a dropped, doubled or mis-positioned row is an integer difference."""
    rope_all(hip, case, rs.rope_inputs(case, exact=True), "rope exact " + rs.rope_id(case), exact=True)


def test_rope_one_element_fallback(hip):
    """half = 258 > 256: the forward takes the one-element kernel and must be correct; both backward entry points return
    CALM_E_UNSUPP and write nothing."""
    case = rs.ROPE_FALLBACK
    B, S, H, dc, dr = dims(case)
    ins = rs.rope_inputs(case)
    got, dev, _ = rope_forward(hip, case, ins)
    worst, failures = rs.check_rope_forward(case, ins, got, strict=False)
    show("rope fallback", worst)
    assert not failures, failures
    g = place(ins["g"])
    DC, DX, DF = Out((B, S, H * dc)), Out((B, S, H * dr)), Out((dr // 2,), init=ins["d0"])
    with pytest.raises(RuntimeError, match="code -3"):
        hip.rope_bwd(g, dev["xr"], dev["table"], DC.t, DX.t, DF.t, B, S, H, dc, dr)
    with pytest.raises(RuntimeError, match="code -3"):
        hip.rope_bwd_part(g, dev["xr"], dev["table"], DC.t, DX.t, B, S, H, dc, dr)
    assert untouched(DC, DX, DF)


@pytest.mark.parametrize("dc,dr,with_content", [(4, 7, True), (4, 0, True), (4, 8, False)],
                         ids=["dr_odd", "dr_zero", "no_content"])
def test_rope_refusals(hip, dc, dr, with_content):
    """CALM_E_INVAL, and not a bit of any output written"""
    B, S, H = 2, 3, 2
    n = B * S * H
    content = place(torch.randn(n * dc)) if with_content else None
    xr, inv, g = place(torch.randn(n * 8)), place(torch.rand(4)), place(torch.randn(n * 12))
    T, O = Out((2 * S * 4,)), Out((n * 12,))
    with pytest.raises(RuntimeError, match="code -1"):
        hip.rope_fwd(content, xr, inv, T.t, O.t, B, S, H, dc, dr)
    table = place(torch.randn(2 * S * 4))
    DC, DX, DF = Out((n * dc,)), Out((n * 8,)), Out((4,), init=torch.ones(4))
    with pytest.raises(RuntimeError, match="code -1"):
        hip.rope_bwd(g, xr, table, DC.t if with_content else None, DX.t, DF.t, B, S, H, dc, dr)
    assert untouched(T, O, DC, DX, DF)


@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("types", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["content", "xr", "out", "d_out", "d_content", "d_xr", "table"])
def test_rope_alignment(hip, name, types, off):
    """One tensor at a time 1 or 2 elements into its allocation at a vw = 4 shape: rope_plan lowers vw to what the
    pointer allows (fp32: 16 bytes for 4, 8 for 2; bf16: 8 and 4), same bounds, same guards.  The grid of
    calm_part_rope_bwd shows the instance that ran."""
    case = dict(rs.ROPE_ALIGN_SHAPE, types=types)
    assert rs.rope_vw_shape(case["dc"], case["dr"]) == 4
    vw_f, vw_b = rope_all(hip, case, rs.rope_inputs(case, seed=3), f"rope align {name}+{off} {types}", offs={name: off})
    esize = 4 if types == "f32" or name == "table" else 2
    lowered = 2 if off * esize % (2 * esize) == 0 else 1
    assert vw_f == (lowered if name in rs.ROPE_ALIGN_FWD else 4)
    assert vw_b == (lowered if name in rs.ROPE_ALIGN_BWD else 4)


# ================================================================================================= spectral norm
def sn_run(hip, ins, training, iters=1):
    """calm_sn_plan + calm_sn_power_iter over all layers of ins with a guarded scratch buffer of the test's own ->
    [dict(t, s, u, v, sigma)] per layer"""
    layers = [tuple(W.shape) for W, _, _ in ins]
    n = len(layers)
    offs, total = rs.sn_offsets(layers)
    Wd = [place(W) for W, _, _ in ins]
    Us, Vs = [Out(u.shape, init=u) for _, u, _ in ins], [Out(v.shape, init=v) for _, _, v in ins]
    Sg = [Out((1,)) for _ in ins]
    arr = (L.SnLayer * n)()
    for i, (rows, cols) in enumerate(layers):
        arr[i].w, arr[i].u, arr[i].v, arr[i].sigma = ptr(Wd[i]), ptr(Us[i].t), ptr(Vs[i].t), ptr(Sg[i].t)
        arr[i].rows, arr[i].cols = rows, cols
    info = L.SnPlanInfo()
    assert hip.lib.calm_sn_plan(arr, n, None, C.byref(info)) == 0
    assert (info.n_layers, info.scratch_floats) == (n, total)
    assert (info.n_work, info.n_work_a) == rs.sn_work_counts(layers)
    blob = np.zeros(info.blob_bytes, dtype=np.uint8)
    assert hip.lib.calm_sn_plan(arr, n, blob.ctypes.data, C.byref(info)) == 0
    blob_dev = torch.from_numpy(blob).to(DEV)
    scratch = Out((total,))
    for _ in range(iters):
        assert hip.lib.calm_sn_power_iter(blob_dev.data_ptr(), C.byref(info), int(training), rs.SN_EPS, ptr(scratch.t),
                                          _stream()) == 0
    sc = scratch.check(written=training)                       # eval: phase A does not run, t stays as it was
    if not training:
        assert untouched(*Us, *Vs)
    got = []
    fill = torch.full((1,), rs.FILL[F32], dtype=torch.int32)
    for i, (rows, cols) in enumerate(layers):
        t_off, s_off = offs[i]
        t, s = sc[t_off:t_off + cols], sc[s_off:s_off + rows]
        assert not bool((s.view(torch.int32) == fill).any()), "an element of s not written"
        if not training:
            assert bool((t.view(torch.int32) == fill).all()), "eval mode wrote t"
        got.append(dict(t=t, s=s, u=Us[i].check(written=False), v=Vs[i].check(written=False), sigma=Sg[i].check()))
    return got


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_sn_power_iteration(hip, training):
    """All of SN_LAYERS in one plan (mixed sizes in the scratch offsets and both work tables), staged t -> v -> s -> u ->
    sigma; eval: u, v bit-unchanged, sigma = u . (W v).  Two layers of the second set have W = 0: t = s = 0, so v, u and
    sigma are exactly 0 and finite (the kernels divide by max(norm, eps))."""
    for seed, zero in ((0, ()), (1, (4, 7))):
        ins = rs.sn_inputs(rs.SN_LAYERS, seed=seed, zero=zero)
        got = sn_run(hip, ins, training)
        worst, failures = rs.check_sn_iter(ins, got, training, strict=False)
        show(f"sn power iteration training={training} seed={seed}", worst)
        assert not failures, failures
        for i in zero:
            keys = ("t", "s", "u", "v", "sigma") if training else ("s", "sigma")
            assert all(bool((got[i][k] == 0).all()) for k in keys)


def test_sn_converges_on_a_known_spectrum(hip):
    """W = Uo diag(2, 1, 0.5, ...) Vo^T rounded to fp32: after 20 training iterations from a random start sigma = 2 and
    u, v are the leading singular vectors, within the float64 sum of the stage bounds (rope_sn_f64.check_sn_converged)."""
    shapes = [(29, 130), (272, 672)]
    spec = [rs.sn_spectrum_layer(r, c, seed=3 + i) for i, (r, c) in enumerate(shapes)]
    start = rs.sn_inputs(shapes, seed=5)
    got = sn_run(hip, [(W64.float(), u, v) for (W64, _, _), (_, u, v) in zip(spec, start)], True, iters=20)
    for (W64, u1, v1), g, shape in zip(spec, got, shapes):
        worst, failures = rs.check_sn_converged(W64, u1, v1, g, strict=False)
        show(f"sn converged {shape}", {"conv:" + k: v for k, v in worst.items()})
        assert not failures, failures


def snw_single(hip, ins, case):
    """calm_sn_weight_bwd with a guarded row-dot scratch -> dict(dW, d_ls)"""
    rows, cols = case["rows"], case["cols"]
    dev = {k: (None if ins[k] is None else place(ins[k])) for k in ("G", "W", "u", "v", "sigma", "ls")}
    DW, DL, SC = Out((rows, cols)), Out((rows,)) if case["d_ls"] else None, Out((rows,))
    rc = hip.lib.calm_sn_weight_bwd(ptr(dev["G"]), ptr(dev["W"]), ptr(dev["u"]), ptr(dev["v"]), ptr(dev["sigma"]),
                                    ptr(dev["ls"]), ptr(DW.t), ptr(DL.t) if DL else None, rows, cols, ptr(SC.t), _stream())
    assert rc == 0
    SC.check()
    got = dict(dW=DW.check())
    if DL:
        got["d_ls"] = DL.check()
    return got


@pytest.fixture(scope="module")
def snw_singles(hip):
    """inputs and the single form's result of a case, computed once (the batched form must repeat it bit for bit)"""
    cache = {}

    def get(case):
        key = rs.snw_id(case)
        if key not in cache:
            ins = rs.snw_inputs(case)
            cache[key] = (ins, snw_single(hip, ins, case))
        return cache[key]
    return get


@pytest.mark.parametrize("case", rs.SNW_CASES, ids=rs.snw_id)
def test_sn_weight_bwd(hip, snw_singles, case):
    ins, got = snw_singles(case)
    worst, failures = rs.check_sn_weight(ins, got, strict=False)
    show("sn weight bwd " + rs.snw_id(case), {"w:" + k: v for k, v in worst.items()})
    assert not failures, failures


def test_sn_weight_bwd_batch(hip, snw_singles):
    """35 entries (two chunks of calm_sn_bwd_batch_max() = 32) of mixed shapes, 1-, 4096- and 4100-column ones among
    them: every dW and d_ls inside guards, inside the float64 bounds, and bit-identical to the single form's."""
    assert hip.lib.calm_sn_bwd_batch_max() == rs.SN_BATCH_MAX
    cases = rs.SNW_BATCH
    ent = (L.SnBwdEntry * len(cases))()
    RD = Out((sum(c["rows"] for c in cases),))
    outs, keep, at = [], [], 0
    for e, case in zip(ent, cases):
        ins, _ = snw_singles(case)
        rows, cols = case["rows"], case["cols"]
        dev = {k: (None if ins[k] is None else place(ins[k])) for k in ("G", "W", "u", "v", "sigma", "ls")}
        DW, DL = Out((rows, cols)), Out((rows,)) if case["d_ls"] else None
        e.G, e.w_orig, e.u, e.v, e.sigma, e.ls = (ptr(dev[k]) for k in ("G", "W", "u", "v", "sigma", "ls"))
        e.d_w_orig, e.d_ls, e.rowdot = ptr(DW.t), ptr(DL.t) if DL else None, RD.t.data_ptr() + 4 * at
        e.rows, e.cols = rows, cols
        at += rows
        outs.append((DW, DL))
        keep.append(dev)
    assert hip.lib.calm_sn_weight_bwd_batch(ent, len(cases), _stream()) == 0
    RD.check()
    worst_all = {}
    for case, (DW, DL) in zip(cases, outs):
        ins, single = snw_singles(case)
        got = dict(dW=DW.check())
        if DL:
            got["d_ls"] = DL.check()
        worst, failures = rs.check_sn_weight(ins, got, strict=False)
        assert not failures, (rs.snw_id(case), failures)
        for k, v in got.items():
            assert torch.equal(_bits(v), _bits(single[k])), f"{rs.snw_id(case)}: {k} differs from the single form's"
        for k, v in worst.items():
            worst_all["wb:" + k] = max(worst_all.get("wb:" + k, 0.0), v)
    show("sn weight bwd batch", worst_all)


@pytest.mark.parametrize("ls", [True, False])
def test_sn_weight_bwd_non_finite_gradient(hip, ls):
    """+inf in one element of G: that row's dot product, hence dot, is infinite and dW is non-finite throughout (NaN
    where inf - inf meets), as exact arithmetic of the formula gives; d_ls is infinite in that row alone."""
    case = rs.snw_case(5, 65, ls=ls)
    ins = rs.snw_inputs(case)
    ins["G"][2, 7] = float("inf")
    got = snw_single(hip, ins, case)
    assert not torch.isfinite(got["dW"][2]).any() and not torch.isfinite(got["dW"]).any()
    assert torch.isfinite(got["d_ls"][[0, 1, 3, 4]]).all() and not torch.isfinite(got["d_ls"][2])
    worst, failures = rs.check_sn_weight_nonfinite(ins, got, strict=False)
    assert not failures, failures


def test_sn_weight_bwd_refusals(hip):
    """rows = 0 or a missing G: CALM_E_INVAL from both forms, nothing written"""
    case = rs.snw_case(4, 64)
    ins = rs.snw_inputs(case)
    dev = {k: place(ins[k]) for k in ("G", "W", "u", "v", "sigma", "ls")}
    DW, DL, SC = Out((4, 64)), Out((4,)), Out((4,))
    for G, rows in ((dev["G"], 0), (None, 4)):
        rc = hip.lib.calm_sn_weight_bwd(ptr(G), ptr(dev["W"]), ptr(dev["u"]), ptr(dev["v"]), ptr(dev["sigma"]),
                                        ptr(dev["ls"]), ptr(DW.t), ptr(DL.t), rows, 64, ptr(SC.t), _stream())
        assert rc == -1
        ent = (L.SnBwdEntry * 1)()
        e = ent[0]
        e.G, e.w_orig, e.u, e.v, e.sigma, e.ls = ptr(G), ptr(dev["W"]), ptr(dev["u"]), ptr(dev["v"]), ptr(dev["sigma"]), ptr(dev["ls"])
        e.d_w_orig, e.d_ls, e.rowdot, e.rows, e.cols = ptr(DW.t), ptr(DL.t), ptr(SC.t), rows, 64
        assert hip.lib.calm_sn_weight_bwd_batch(ent, 1, _stream()) == -1
    assert untouched(DW, DL, SC)
