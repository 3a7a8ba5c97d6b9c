"""The CNN tail (calm_cnn_residual_fwd / _bwd, calm_dwconv3x3_fwd / _bwd, the three token permutations) and the
optimizer-side step (calm_optim_step) of libcalmvit_hip.so against the float64 references of tail_f64.py, element by
element, at the case tables defined there.  tests/test_tail_f64_cpu.py proves the same checkers on an fp32 emulation and
on planted faults.  Every output sits between NaN-pattern guards; outputs that accumulate start from non-zero contents.
Each case prints its worst error / bound per output (DESIGN.md records them)."""
import functools

import pytest
import torch

import calm_vit_dte_amd as calm
import tail_f64 as tf
from tail_f64 import CH
from test_rowwise_f64_gpu import DEV, GUARD, Out, _bits, place

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return calm.backend.get_backend()


def show(label, worst):
    print(f"\n[tail_f64] {label}: " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))


# ================================================================================================= fused CNN tail
@pytest.fixture(scope="module")
def cnn_case():
    """inputs, float64 reference and bounds of a case, computed once per (B, S, residual)"""
    @functools.lru_cache(maxsize=None)
    def case(B, S, residual, backward):
        ins = tf.cnn_inputs(B, S)
        return (ins,) + tf.cnn_reference(ins, B, S, residual, backward)
    return case


@pytest.mark.parametrize("residual", [1, 0])
@pytest.mark.parametrize("B,S,backward", tf.CNN_CASES)
def test_cnn_residual(hip, cnn_case, B, S, backward, residual):
    ins, ref, bound = cnn_case(B, S, residual, backward)
    x = place(ins["x"])
    w = [place(ins[k]) for k in tf.CNN_W]
    O = Out((B, S, 3 * S))
    hip.cnn_fwd(x, *w, O.t, B, S, CH, residual=bool(residual))
    got = dict(out=O.check())
    if backward:
        DX = Out((B, S, 3 * S))
        grads = {name: Out((n,), init=ins[name + "_init"]) for name, n in tf.CNN_GRADS}
        hip.cnn_bwd(place(ins["dy"]), x, *w, DX.t, *(grads[name].t for name, _ in tf.CNN_GRADS), B, S, CH,
                    residual=bool(residual))
        got["dx"] = DX.check()
        got.update({name: o.check(written=False) for name, o in grads.items()})
    worst, failures = tf.check_cnn(got, ref, bound, strict=False)
    show(f"cnn B={B} S={S} res={residual}", worst)
    assert not failures, failures


# ================================================================================================= dwconv3x3
@pytest.mark.parametrize("case", tf.DWCONV_CASES, ids=lambda c: "B{B}-S{S}-C{C}-a{act}".format(**c))
def test_dwconv3x3(hip, case):
    B, S, C = case["B"], case["S"], case["C"]
    ins = tf.dwconv_inputs(case)
    ref, bound = tf.dwconv_reference(ins, case)
    opt = lambda k: place(ins[k]) if ins[k] is not None else None
    x, w, sg, bias = place(ins["x"]), place(ins["w"]), opt("inv_scale"), opt("bias")
    Y, YP = Out((B, S, S, C)), Out((B, S, S, C)) if case["y_pre"] else None
    hip.dwconv_fwd(x, w, sg, bias, Y.t, YP.t if YP else None, case["act"], B, S, C)
    got = dict(y=Y.check())
    if YP:
        got["y_pre"] = YP.check()
    DX, DW, DB = Out((B, S, S, C)), Out((C, 9), init=ins["dw_init"]), Out((C,), init=ins["db_init"])
    hip.dwconv_bwd(place(ins["dz"]), x, w, sg, DX.t, DW.t, DB.t, B, S, C)
    got.update(dx=DX.check(), dw=DW.check(written=False), db=DB.check(written=False))
    worst, failures = tf.check_dwconv(got, ref, bound, strict=False)
    show("dwconv B={B} S={S} C={C} act={act}".format(**case), worst)
    assert not failures, failures


@pytest.mark.parametrize("C", tf.DWCONV_UNSUPPORTED_C)
def test_dwconv3x3_bwd_unsupported_channels(hip, C):
    """C > 64 or 256 % C != 0: CALM_E_UNSUPP, and not a bit of dx, dw, db written."""
    B, S = 1, 5
    x, dz, w = (place(torch.randn(*s)) for s in ((B, S, S, C), (B, S, S, C), (C, 9)))
    DX, DW, DB = Out((B, S, S, C)), Out((C, 9), init=torch.ones(C, 9)), Out((C,), init=torch.ones(C))
    with pytest.raises(RuntimeError, match="code -3"):
        hip.dwconv_bwd(dz, x, w, None, DX.t, DW.t, DB.t, B, S, C)
    torch.cuda.synchronize()
    for o in (DX, DW, DB):
        assert torch.equal(_bits(o.buf).cpu(), o.before)


# ================================================================================================= permutations
def _permute(hip, kind, src, dst, B, S):
    getattr(hip, kind)(src, dst, B, S)


@pytest.mark.parametrize("kind", ["image_to_rows", "rows_to_image", "grid_transpose"])
@pytest.mark.parametrize("B", tf.PERM_B)
@pytest.mark.parametrize("S", tf.PERM_S)
def test_token_permutation(hip, kind, B, S):
    src_shape, dst_shape = tf.perm_shapes(kind, B, S)
    src = torch.randn(*src_shape, generator=tf.gen(S))
    O = Out(dst_shape)
    _permute(hip, kind, place(src), O.t, B, S)
    want = src.reshape(-1)[tf.perm_index(kind, B, S)]
    assert torch.equal(O.check().reshape(-1).view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("B,S,src_off,dst_off", tf.TRANSPOSE_MISALIGNED)
def test_grid_transpose_misaligned(hip, B, S, src_off, dst_off):
    """S % 4 == 0 with the source or the destination one float off 16-byte alignment: the scalar kernel."""
    src = torch.randn(B, S, 3 * S, generator=tf.gen(S + 1))
    X, O = place(src, src_off), Out((B, S, 3 * S), off=dst_off)
    assert (X.data_ptr() % 16 != 0) == bool(src_off) and (O.t.data_ptr() % 16 != 0) == bool(dst_off)
    hip.grid_transpose(X, O.t, B, S)
    want = src.reshape(-1)[tf.perm_index("grid_transpose", B, S)]
    assert torch.equal(O.check().reshape(-1).view(torch.int32), want.view(torch.int32))


# ================================================================================================= optimizer step
class Arena:
    """Tensors laid out in ONE device buffer, each behind a gap of GUARD + offset fill elements (a NaN pattern no kernel
    produces): one upload, one download, and every gap must come back bit for bit."""

    def __init__(self, tensors, offsets=None):
        offsets = offsets or [0] * len(tensors)
        self.spans, at = [], 0
        for t, off in zip(tensors, offsets):
            at += GUARD + off
            self.spans.append((at, at + t.numel()))
            at += t.numel()
        host = torch.full((at + GUARD,), tf.FILL[torch.float32], dtype=torch.int32)
        self.gap = torch.ones(at + GUARD, dtype=torch.bool)
        for t, (lo, hi) in zip(tensors, self.spans):
            host[lo:hi] = t.reshape(-1).view(torch.int32)
            self.gap[lo:hi] = False
        self.before = host
        self.buf = host.view(torch.float32).to(DEV)
        self.views = [self.buf[lo:hi] for lo, hi in self.spans]

    def read(self):
        """the tensors now (CPU, flat, concatenated); the gaps must be untouched"""
        now = self.buf.cpu()
        assert torch.equal(now.view(torch.int32)[self.gap], self.before[self.gap]), "write outside a tensor"
        return now[~self.gap].clone()


class Device:
    """A table's state on the device: p, m, v in guarded arenas, the plan, one optim_step per call of step()."""

    def __init__(self, hip, table, recs):
        self.hip, self.table = hip, table
        self.p, self.m, self.v = (Arena([r[k] for r in recs]) for k in ("param", "exp_avg", "exp_avg_sq"))
        sn = [r["sn"] for r in recs]
        self.sn = [None if s is None else (place(s[0]), place(s[1]), place(s[2]), s[3], s[4]) for s in sn]
        self.plan = hip.optim_plan([dict(param=p, exp_avg=m, exp_avg_sq=v, sn=s)
                                    for p, m, v, s in zip(self.p.views, self.m.views, self.v.views, self.sn)])

    def step(self, grads, sc):
        G = Arena(grads, [e["goff"] for e in self.table])
        stats = Out((2,))
        gs = place(torch.tensor([sc["grad_scale"]])) if sc["grad_scale"] else None
        lr_dev = place(torch.tensor([sc["lr_dev"]])) if sc["lr_dev"] is not None else None
        self.hip.optim_step(self.plan, G.views, tf.optim_hp(sc), gs, stats.t, lr_dev=lr_dev)
        st = stats.check()
        G.read()
        return dict(p=self.p.read(), m=self.m.read(), v=self.v.read(), norm=float(st[0]), found_inf=float(st[1]),
                    step=int(self.plan.step_dev.item()))


TABLE = tf.optim_table()


def _state_from(recs, got):
    """records (CPU) holding the state a step left on the device"""
    out, at = [], 0
    for r in recs:
        n = r["param"].numel()
        out.append(dict(r, param=got["p"][at:at + n].clone(), exp_avg=got["m"][at:at + n].clone(),
                        exp_avg_sq=got["v"][at:at + n].clone()))
        at += n
    return out


def _two_steps(hip, table, recs, sc, label):
    dev = Device(hip, table, recs)
    dev.plan.step_dev.fill_(sc["t_prev"])
    step = sc["t_prev"]
    for call in (1, 2):
        grads = tf.optim_grads(table, recs, seed=call, scale=sc["grad_scale"] or 1.0)
        ref, bound = tf.optim_reference(recs, grads, tf.optim_hp(sc), sc["grad_scale"], step, sc["lr_dev"])
        got = dev.step(grads, sc)
        worst, failures = tf.check_optim(got, ref, bound, strict=False)
        show(f"optim {label} call {call}", worst)
        assert not failures, failures
        recs, step = _state_from(recs, got), got["step"]         # the next reference starts from the device state
    assert step == sc["t_prev"] + 2


@pytest.mark.parametrize("sc", tf.OPTIM_SCENARIOS, ids=lambda s: s["name"])
def test_optim_step(hip, sc):
    assert hip.lib.calm_optim_chunk_elems() == tf.OPT_CHUNK
    _two_steps(hip, TABLE, tf.optim_state(TABLE), sc, sc["name"])


@pytest.mark.parametrize("kinds", [("sn", "cancel"), ("cancel",)], ids=["spectral_only", "cancelling_only"])
def test_optim_step_deferred_correction_norm_alone(hip, kinds):
    """Only spectral-norm tensors in the plan, so the reported norm IS the deferred-correction norm; then the cancelling
    tensor alone, whose norm is what is left of (|G|^2 - 2 c u^T G v + c^2 |u|^2 |v|^2) / sigma^2 after the parts
    cancel to 1e-3 of themselves (the bound is relative to the parts: tail_f64.optim_reference)."""
    keep = [i for i, e in enumerate(TABLE) if e["kind"] in kinds]
    recs = tf.optim_state(TABLE)
    sc = next(s for s in tf.OPTIM_SCENARIOS if s["name"] == "clip_t1000")
    _two_steps(hip, [TABLE[i] for i in keep], [recs[i] for i in keep], sc, "+".join(kinds))


@pytest.mark.parametrize("case", tf.optim_nonfinite_cases(TABLE), ids=lambda c: c[0])
def test_optim_step_skipped_on_non_finite_gradient(hip, case):
    _, tensor, element, value = case
    sc = next(s for s in tf.OPTIM_SCENARIOS if s["name"] == "clip_t1000")
    recs = tf.optim_state(TABLE)
    grads = tf.optim_grads(TABLE, recs, seed=1)
    grads[tensor][element] = value
    dev = Device(hip, TABLE, recs)
    dev.plan.step_dev.fill_(sc["t_prev"])
    got = dev.step(grads, sc)
    tf.check_optim_skipped(got, tf.optim_flat(recs), sc["t_prev"])
