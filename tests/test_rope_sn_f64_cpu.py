"""The checkers of rope_sn_f64.py, proven without a GPU: an fp32 emulation of each kernel (torch fp32, with the kernel's
reduction grouping where the bound depends on it) must sit inside every bound at every case of the GPU tables, and every
planted fault must be rejected by the output it corrupts.  The replicated host formulas are checked against values
computed by hand, the weight-gradient reference against autograd of the independent formulation."""
import math

import pytest
import torch

import rope_sn_f64 as rs
from rope_sn_f64 import F32, cdiv


def names(failures):
    return {n for n, _ in failures}


# ================================================================================================= emulations
def reduce_partials32(part):
    """calm_reduce_partials_block: row lane rg = g mod 16 with four running sums (g mod 64 picks the sum) in increasing
    g, (a0 + a1) + (a2 + a3), the sixteen lanes pairwise -> the total that is added onto the output"""
    G, n = part.shape
    p = torch.cat([part, torch.zeros(cdiv(G, 64) * 64 - G, n)]).reshape(-1, 4, 16, n)
    a = torch.zeros(4, 16, n)
    for i in range(p.shape[0]):
        a = a + p[i]
    red = (a[0] + a[1]) + (a[2] + a[3])
    t = [(red[4 * q] + red[4 * q + 1]) + (red[4 * q + 2] + red[4 * q + 3]) for q in range(4)]
    return (t[0] + t[1]) + (t[2] + t[3])


def emu_rope(case, ins, fault=None):
    """calm_rope_fwd, calm_rope_bwd and the partials of calm_part_rope_bwd in torch fp32; d_inv_freq summed as
    rope_bwd_vec_kernel does: a row lane's rows, the block's row lanes in order, calm_reduce_partials."""
    B, S, H, dc, dr = (case[k] for k in ("B", "S", "H", "dc", "dr"))
    tin, tout = rs.ROPE_TYPES[case["types"]]
    half, nrows = dr // 2, B * S * H
    ang = torch.arange(S, dtype=F32)[:, None] * ins["inv_freq"][None, :]
    table = torch.stack([ang.cos(), ang.sin()])
    row = torch.arange(nrows)
    pos = row % S if fault == "pos" else (row // H) % S
    c, sn = table[0][pos], table[1][pos]
    x = ins["xr"].float().reshape(nrows, dr)
    x1, x2 = x[:, :half], x[:, half:]
    x2f = x[:, half - 1:dr - 1] if fault == "x2_off" else x2
    rot = torch.cat([x1 * c - x2f * sn, x2f * c + x1 * sn], 1)
    if fault == "trunc":
        rot = (rot.view(torch.int32) & -65536).view(F32)
    out = torch.zeros(nrows, dc + dr, dtype=tout)
    out[:, dc:] = rot.to(tout)
    if dc:
        out[:, :dc] = ins["content"].reshape(nrows, dc).to(tout)
        if fault == "content_col":
            out[:, dc - 1] = 0
    got = dict(table=table, out=out.reshape(B, S, -1))
    g = ins["g"].float().reshape(nrows, dc + dr)
    g1, g2 = g[:, dc:dc + half], g[:, dc + half:]
    if dc:
        got["d_content"] = g[:, :dc].to(tin).reshape(B, S, -1)
    sg = -1.0 if fault == "dxr_sign" else 1.0
    got["d_xr"] = torch.cat([g1 * c + sg * (g2 * sn), g2 * c - sg * (g1 * sn)], 1).to(tin).reshape(B, S, -1)
    if rs.rope_fits(B, S, H, dc, dr):
        term = (g1 * (-x1 * sn - x2 * c) + g2 * (-x2 * sn + x1 * c)) * pos.float()[:, None]
        if fault == "last_row":
            term[-1] = 0
        vw = rs.rope_vw(dc, dr)
        rpb, G = rs.rope_rpb(dr, vw), rs.rope_bwd_grid(nrows, dr, vw)
        npass = cdiv(nrows, G * rpb)
        t = torch.cat([term, torch.zeros(npass * G * rpb - nrows, half)]).reshape(npass, G, rpb, half)
        acc = torch.zeros(G, rpb, half)
        for p in range(npass):
            acc = acc + t[p]
        part = torch.zeros(G, half)
        for r in range(rpb):
            part = part + acc[:, r]
        got["part"] = part
        total = reduce_partials32(part)
        got["d_inv_freq"] = total if fault == "overwrite" else ins["d0"] + total
    return got


def check_rope(case, ins, got, exact=False):
    """forward and backward checkers on one emulation's outputs -> the names of the outputs that failed"""
    vw = rs.rope_vw(case["dc"], case["dr"])
    table = got["table"]
    bad = set()
    _, f = rs.check_rope_forward(case, ins, got, strict=False, exact=exact)
    bad |= names(f)
    full = {k: v for k, v in got.items() if k != "part"}
    _, f = rs.check_rope_backward(case, ins, table, full, vw, strict=False, exact=exact)
    bad |= names(f)
    part = {k: v for k, v in got.items() if k != "d_inv_freq"}
    _, f = rs.check_rope_backward(case, ins, table, part, vw, strict=False, exact=exact, d0=False)
    return bad | names(f)


def wave_sum32(x):
    """wave_sum (common.h): the xor butterfly over the last axis of 64 lanes"""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lane ^ o]
    return x[..., 0]


def block_sum32(x):
    """block_sum_256: wave sums, then red[0] + red[1] + red[2] + red[3]"""
    w = wave_sum32(x.reshape(*x.shape[:-1], 4, 64))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def serial32(x, threads):
    """thread t adds elements t, t + threads, ... of the last axis in order -> [..., threads]"""
    n = x.shape[-1]
    x = torch.cat([x, torch.zeros(*x.shape[:-1], cdiv(n, threads) * threads - n)], -1).reshape(*x.shape[:-1], -1, threads)
    acc = torch.zeros(*x.shape[:-2], threads)
    for k in range(x.shape[-2]):
        acc = acc + x[..., k, :]
    return acc


def emu_sn_layer(W, u, v, training, fault=None):
    """sn_phase_a / _b / _c in torch fp32 with their groupings (phase A's rows past the unrolled groups go to the four
    running sums in turn rather than to s0: no deeper than the kernel's chain)"""
    rows, cols = W.shape
    eps = torch.tensor(rs.SN_EPS, dtype=F32)
    got = {}
    if training:
        Wa = W.t() if fault == "t_layout" else W
        prod = Wa * u[:, None]
        prod = torch.cat([prod, torch.zeros(cdiv(rows, 16) * 16 - rows, cols)]).reshape(-1, 4, 4, cols)   # r = 16 i + 4 j + g
        s = torch.zeros(4, 4, cols)
        for i in range(prod.shape[0]):
            s = s + prod[i]
        wave = (s[0] + s[1]) + (s[2] + s[3])
        t = (wave[0] + wave[1]) + (wave[2] + wave[3])
        if fault == "t_tail" and cols % 64:
            t[cols - cols % 64:] = 0
        inv = 1.0 / torch.maximum(block_sum32(serial32(t * t, 256)).sqrt(), eps)
        vnew = t * inv
        got.update(t=t, v=v.clone() if fault == "v_stale" else vnew)
    else:
        vnew = v
        got["v"] = v.clone()
    s = wave_sum32(serial32(W * vnew[None, :], 64))
    got["s"] = s
    if training:
        inv = 1.0 / torch.maximum(block_sum32(serial32(s * s, 256)).sqrt(), eps)
        unew = s * inv
        got["u"] = unew
        got["sigma"] = block_sum32(serial32((u if fault == "sigma_old_u" else unew) * s, 256)).reshape(1)
    else:
        got["u"] = u.clone()
        got["sigma"] = block_sum32(serial32(u * s, 256)).reshape(1)
        if fault == "eval_u":
            got["u"][0] = torch.nextafter(got["u"][0], torch.tensor(2.0))
        if fault == "eval_v":
            got["v"][-1] = torch.nextafter(got["v"][-1], torch.tensor(2.0))
    return got


def emu_sn_weight(ins, want_dls, fault=None):
    """sn_rowdot_row, sn_apply_dot, sn_apply_elem in torch fp32"""
    G, W, u, v = ins["G"], ins["W"], ins["u"], ins["v"]
    rows = G.shape[0]
    inv = 1.0 / ins["sigma"][0]
    rowdot = wave_sum32(serial32(G * W, 64)) * inv
    ls = torch.ones(rows) if ins["ls"] is None else ins["ls"]
    dot = block_sum32(serial32((torch.ones(rows) if fault == "ls_ignored" else ls) * rowdot, 256))
    uv = v[:, None] * u[None, :] if fault == "uv_T" else u[:, None] * v[None, :]
    got = dict(dW=(ls[:, None] * G - dot * uv) * inv)
    if want_dls:
        got["d_ls"] = rowdot * ls if fault == "dls_ls" else rowdot
    return got


# ================================================================================================= host formulas
def test_rope_host_formulas_by_hand():
    # (dc, dr) = (32, 32), 165 rows: half 16, vw 4, ir 4, rpb 64, 3 workgroups both ways, depth 1 + 64 + (1 + 7)
    assert (rs.rope_half(32), rs.rope_vw(32, 32), rs.rope_rpb(32, 4)) == (16, 4, 64)
    assert (rs.rope_grid(165, 32, 4), rs.rope_bwd_grid(165, 32, 4), rs.rope_dif_depth(165, 32, 4)) == (3, 3, 73)
    # (8, 48), 165 rows: half 24, vw 4, ir 6, rpb 42, 4 workgroups, depth 1 + 42 + 8
    assert (rs.rope_vw(8, 48), rs.rope_rpb(48, 4), rs.rope_grid(165, 48, 4), rs.rope_dif_depth(165, 48, 4)) == (4, 42, 4, 51)
    # (1, 512), 4785 rows: vw 1, rpb 1, forward grid capped at 4096, backward at 1024: depth 5 + 1 + (16 + 7)
    assert (rs.rope_vw(1, 512), rs.rope_rpb(512, 1), rs.rope_grid(4785, 512, 1)) == (1, 1, 4096)
    assert (rs.rope_bwd_grid(4785, 512, 1), rs.rope_dif_depth(4785, 512, 1)) == (1024, 29)
    # (4, 256), 8427 rows: vw 4, ir 32, rpb 8, 1054 workgroups forward, 1024 backward: depth 2 + 8 + 23
    assert (rs.rope_vw(4, 256), rs.rope_rpb(256, 4), rs.rope_grid(8427, 256, 4)) == (4, 8, 1054)
    assert (rs.rope_bwd_grid(8427, 256, 4), rs.rope_dif_depth(8427, 256, 4)) == (1024, 33)
    assert (rs.rope_vw(18, 18), rs.rope_rpb(18, 1)) == (1, 28) and (rs.rope_vw(6, 12), rs.rope_rpb(12, 2)) == (2, 85)
    assert (rs.rope_vw(10, 20), rs.rope_vw(5, 6), rs.rope_vw(0, 2), rs.rope_vw(3, 512)) == (2, 1, 1, 1)
    assert rs.rope_fits(2, 5, 3, 3, 512) and not rs.rope_fits(2, 5, 3, 3, 516)
    assert not rs.rope_fits(1 << 10, 1 << 10, 1 << 5, 0, 64)          # 2^31 elements


def test_rope_want_branch_is_unreachable():
    """bwd_grid's `want = grid / 16` branch needs want >= 1024 while grid <= 4096: never taken, at any shape"""
    assert rs.ROPE_VEC_MAX_GRID // 16 < rs.ROPE_BWD_GRID
    for nrows in (1, 4096, 1 << 20, (1 << 31) - 1):
        for dr, vw in ((2, 1), (512, 1), (512, 4), (32, 4)):
            assert rs.rope_bwd_grid(nrows, dr, vw) == min(rs.rope_grid(nrows, dr, vw), rs.ROPE_BWD_GRID)


def test_rope_alignment_formula():
    """fp32: 16 bytes for vw 4, 8 for vw 2; bf16: 8 and 4.  Aligned tensors keep the instance of the shape."""
    assert [rs.rope_vw(8, 48, [(a, 4)]) for a in (4, 8, 12, 16, 32)] == [1, 2, 1, 4, 4]
    assert [rs.rope_vw(8, 48, [(a, 2)]) for a in (2, 4, 6, 8, 16)] == [1, 2, 1, 4, 4]
    assert rs.rope_vw(8, 48, [(256, 4), (256, 2), (8, 4)]) == 2 and rs.rope_vw(6, 12, [(4, 2)]) == 2
    assert rs.rope_vw(6, 12, [(4, 4)]) == 1 and rs.rope_vw(5, 6, [(2, 2)]) == 1
    for c in rs.ROPE_CASES:
        for esize in (2, 4):
            assert rs.rope_vw(c["dc"], c["dr"], [(0, esize), (256, esize), (1 << 20, 4)]) == rs.rope_vw_shape(c["dc"], c["dr"])


def test_rope_case_table_reaches_its_paths():
    reach = {(rs.rope_vw(c["dc"], c["dr"]), c["dr"] // 2 // rs.rope_vw(c["dc"], c["dr"])) for c in rs.ROPE_CASES}
    assert {(4, 4), (4, 6), (4, 5), (2, 3), (1, 9), (2, 5), (1, 3), (4, 64), (1, 256), (1, 1), (4, 32)} <= reach
    multi_fwd = [c for c in rs.ROPE_CASES
                 if cdiv(c["B"] * c["S"] * c["H"], rs.rope_rpb(c["dr"], rs.rope_vw(c["dc"], c["dr"]))) > rs.ROPE_VEC_MAX_GRID]
    multi_bwd = [c for c in rs.ROPE_CASES
                 if cdiv(c["B"] * c["S"] * c["H"], rs.rope_rpb(c["dr"], rs.rope_vw(c["dc"], c["dr"]))) > rs.ROPE_BWD_GRID]
    assert multi_fwd and len(multi_bwd) > len(multi_fwd)
    for c in multi_bwd:                                     # H and S coprime to the pass stride: advance() carries
        stride = rs.ROPE_BWD_GRID * rs.rope_rpb(c["dr"], rs.rope_vw(c["dc"], c["dr"]))
        assert math.gcd(c["H"], stride) == 1 and math.gcd(c["S"], stride) == 1
    assert all(c["B"] * c["S"] * c["H"] * (c["dc"] + c["dr"]) <= 3_000_000 for c in rs.ROPE_CASES)
    assert not rs.rope_fits(*(rs.ROPE_FALLBACK[k] for k in ("B", "S", "H", "dc", "dr")))


def test_sn_host_formulas_by_hand():
    assert rs.sn_offsets([(2, 3), (5, 64), (17, 1)]) == ([(0, 3), (5, 69), (74, 75)], 92)
    assert rs.sn_work_counts([(2, 3), (5, 64), (17, 1)]) == (4, 3)
    assert rs.sn_work_counts([(272, 672)]) == (17, 11) and rs.sn_offsets([(272, 672)]) == ([(0, 672)], 944)
    assert [rs.sn_apply_rows_per_block(c) for c in (1, 1000, 4095, 4096, 4100)] == [4096, 4, 1, 1, 1]
    assert len(rs.SNW_BATCH) == 35 > rs.SN_BATCH_MAX
    assert {4096, 4100, 1} <= {c["cols"] for c in rs.SNW_BATCH}
    assert rs.partials_depth(1024) == 23 and rs.partials_depth(3) == 8


# ================================================================================================= RoPE
@pytest.mark.parametrize("case", rs.ROPE_CASES + [rs.ROPE_FALLBACK], ids=rs.rope_id)
def test_rope_emulation_inside_every_bound(case):
    ins = rs.rope_inputs(case)
    got = emu_rope(case, ins)
    if "part" not in got:                                   # the fallback shape: the forward alone
        assert rs.check_rope_forward(case, ins, got, strict=False)[1] == []
        return
    assert check_rope(case, ins, got) == set()


@pytest.mark.parametrize("case", [c for c in rs.ROPE_CASES if c["types"] in ("f32", "bf16")], ids=rs.rope_id)
def test_rope_emulation_exact_on_integers(case):
    ins = rs.rope_inputs(case, exact=True)
    assert check_rope(case, ins, emu_rope(case, ins), exact=True) == set()


ROPE_FAULTS = [
    # fault, the case it is planted in, the outputs that must reject it
    ("pos", 1, {"out:rot", "d_xr", "d_inv_freq", "part"}),
    ("x2_off", 1, {"out:rot"}),
    ("dxr_sign", 1, {"d_xr"}),
    ("last_row", 1, {"d_inv_freq", "part"}),
    ("last_row", 14, {"d_inv_freq", "part"}),               # one row of 8427
    ("overwrite", 1, {"d_inv_freq"}),
    ("trunc", 15, {"out:rot"}),
    ("trunc", 17, {"out:rot"}),
    ("content_col", 1, {"out:content"}),
    ("content_col", 15, {"out:content"}),
]


@pytest.mark.parametrize("fault,idx,rejected_by", ROPE_FAULTS)
def test_rope_planted_fault_is_rejected(fault, idx, rejected_by):
    case = rs.ROPE_CASES[idx]
    ins = rs.rope_inputs(case)
    assert check_rope(case, ins, emu_rope(case, ins, fault)) == rejected_by


@pytest.mark.parametrize("fault,idx,rejected_by", [
    # on the integer inputs (c = 1, sn = 0): what the exact comparison alone must see
    ("pos", 1, {"d_inv_freq", "part"}), ("x2_off", 1, {"out:rot"}), ("last_row", 14, {"d_inv_freq", "part"}),
    ("overwrite", 13, {"d_inv_freq"}), ("content_col", 15, {"out:content"})])
def test_rope_planted_fault_is_rejected_by_the_exact_case(fault, idx, rejected_by):
    case = rs.ROPE_CASES[idx]
    ins = rs.rope_inputs(case, exact=True)
    assert check_rope(case, ins, emu_rope(case, ins, fault), exact=True) == rejected_by


# ================================================================================================= spectral norm
def test_sn_emulation_inside_every_bound():
    for seed, zero in ((0, ()), (1, (4, 7))):
        ins = rs.sn_inputs(rs.SN_LAYERS, seed=seed, zero=zero)
        for training in (True, False):
            got = [emu_sn_layer(W, u, v, training) for W, u, v in ins]
            worst, failures = rs.check_sn_iter(ins, got, training, strict=False)
            assert failures == [], failures
        for i in zero:                                       # zero weight: v, u, sigma exactly 0 and finite
            g = emu_sn_layer(*ins[i], True)
            assert all(bool((g[k] == 0).all()) for k in ("t", "v", "s", "u", "sigma"))


# (v_stale: s is referenced from the stored v, which phase B then did not use, so s rejects it as well)
SN_FAULTS = [
    ("t_layout", rs.SN_SQUARE, True, {"t"}), ("t_tail", 6, True, {"t"}), ("t_tail", 10, True, {"t"}),
    ("v_stale", 7, True, {"v", "s"}), ("sigma_old_u", 10, True, {"sigma"}), ("sigma_old_u", 2, True, {"sigma"}),
    ("eval_u", 7, False, {"u"}), ("eval_v", 7, False, {"v"}),
]


@pytest.mark.parametrize("fault,layer,training,rejected_by", SN_FAULTS)
def test_sn_planted_fault_is_rejected(fault, layer, training, rejected_by):
    W, u, v = rs.sn_inputs(rs.SN_LAYERS)[layer]
    _, failures = rs.check_sn_layer(W, u, v, emu_sn_layer(W, u, v, training, fault), training, strict=False)
    assert names(failures) == rejected_by, failures


def test_sn_converges_on_a_known_spectrum():
    W64, u1, v1 = rs.sn_spectrum_layer(29, 130, seed=3)
    W = W64.float()
    _, u, v = rs.sn_inputs([(29, 130)], seed=5)[0]
    for _ in range(20):
        got = emu_sn_layer(W, u, v, True)
        u, v = got["u"], got["v"]
    worst, failures = rs.check_sn_converged(W64, u1, v1, got, strict=False)
    assert failures == [], failures
    got["sigma"] = got["sigma"] * (1 + 1e-5)                # a sigma 1e-5 off is outside
    assert names(rs.check_sn_converged(W64, u1, v1, got, strict=False)[1]) == {"sigma"}


def test_sn_weight_reference_against_autograd():
    """dW, d_ls of the kernel's stated formula = autograd of sum(G * ls[:, None] W / (u^T W v)), u and v constant"""
    for case in (rs.snw_case(5, 65), rs.snw_case(144, 144), rs.snw_case(3, 63, ls=False)):
        ins = rs.snw_inputs(case)
        W = ins["W"].double().requires_grad_(True)
        ls = (torch.ones(case["rows"], dtype=torch.float64) if ins["ls"] is None else ins["ls"].double()).requires_grad_(True)
        u, v, G = ins["u"].double(), ins["v"].double(), ins["G"].double()
        sigma = u @ W @ v
        (G * (ls[:, None] * W / sigma)).sum().backward()
        ins["sigma"] = sigma.detach().reshape(1)            # float64: the reference widens it exactly
        ref = rs.snw_reference(ins)
        assert torch.allclose(ref["dW"], W.grad, rtol=1e-12, atol=1e-13)
        assert torch.allclose(ref["rowdot"], ls.grad, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("case", rs.SNW_CASES, ids=rs.snw_id)
def test_sn_weight_emulation_inside_every_bound(case):
    ins = rs.snw_inputs(case)
    _, failures = rs.check_sn_weight(ins, emu_sn_weight(ins, case["d_ls"]), strict=False)
    assert failures == [], failures


@pytest.mark.parametrize("fault,idx,rejected_by", [("ls_ignored", 4, {"dW"}), ("ls_ignored", 5, {"dW"}),
                                                   ("dls_ls", 4, {"d_ls"}), ("dls_ls", 2, {"d_ls"}), ("uv_T", 5, {"dW"})])
def test_sn_weight_planted_fault_is_rejected(fault, idx, rejected_by):
    ins = rs.snw_inputs(rs.SNW_CASES[idx])
    _, failures = rs.check_sn_weight(ins, emu_sn_weight(ins, True, fault), strict=False)
    assert names(failures) == rejected_by, failures


def test_sn_weight_nonfinite_pattern():
    """+inf in G: that row's rowdot is +-inf, dot with it, and dW is non-finite throughout (NaN where inf - inf meets)"""
    ins = rs.snw_inputs(rs.snw_case(5, 65))
    ins["G"][2, 7] = float("inf")
    got = emu_sn_weight(ins, True)
    assert not torch.isfinite(got["dW"]).any()
    assert rs.check_sn_weight_nonfinite(ins, got, strict=False)[1] == []
    got["dW"][0, 0] = 1.0
    assert names(rs.check_sn_weight_nonfinite(ins, got, strict=False)[1]) == {"dW"}
