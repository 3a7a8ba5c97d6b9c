"""TEST INFRASTRUCTURE: the float64 reference and the bounds of calm_optim_step_lamb (csrc/optim.hip), built on tail_f64 as
sam_f64 is: the table, the state and the gradients are tail_f64's (two records overridden, below), and the corrected
gradient, the norm, the clip coefficient, found_inf, the step count, the new moments m, v AND their bounds e_m, e_v are
tail_f64.optim_reference's — LAMB's passes 1 and 2 are calm_optim_step's kernels and its moments calm_optim_step's formula,
neither of which reads lr or weight_decay.  The module knows nothing about who produced what it checks.

No measured tolerance.  From the operation order the header states, with U = 2^-24, d = tail_f64.optim_sum_depth(numel),
every hyper-parameter the fp32 value the ABI receives, t the step count after the call, bc1 = 1 - b1^t, bc2 = 1 - b2^t,
rr1 / ri2 the relative errors tail_f64.optim_reference charges for the fp32 bc1 and 1 / sqrt(bc2), and a division charged
2 U (one ulp: it is correctly rounded, and U would do) where a product, a sum and a square root are charged U:

    sv = sqrt(v)              e_sv = min(e_v / sv, sqrt(e_v)) + U sv                  (|sqrt a - sqrt b| <= both)
    den = sv isb2 + eps       e_den = e_sv isb2 + sv isb2 (ri2 + U) + U den           (optim_reference's own expression)
    q = m / den               e_q = e_m / den + |m| e_den / (den (den - e_den)) + 2 U |q|
    r = q / bc1               e_r = (e_q / bc1)(1 + rr1) + |r| rr1 + 2 U (|r| + e_q / bc1)
    dw = wd_t w               e_dw = U |dw|                                           (exact inputs, one rounding)
    u = r + dw                e_u = e_r + e_dw + U (|u| + e_r + e_dw)                 (never contracted: three roundings)
    W2 = sum w^2              e_W2 = (d + 1) U W2                                     (one rounding per square, the depth)
    U2 = sum u^2              e_U2 = sum (2 |u| e_u + e_u^2) + (d + 1) U sum (|u| + e_u)^2
    wn = sqrt(W2)             e_wn = min(e_W2 / wn, sqrt(e_W2)), + U (wn + that);     un likewise
    ratio = wn / un           e_ratio = (e_wn + ratio e_un) / (un - e_un), + 2 U (ratio + that)     needs un > e_un
    trust = min(ratio, clip)  e_trust = e_ratio while ratio - e_ratio < clip, else 0  (min is 1-Lipschitz; as the clip of
                                                                                      the gradient norm in optim_reference)
    step = lr_t trust         e_step = lr_t e_trust + U (step + lr_t e_trust)
    upd = step u              e_upd = step e_u + |u| e_step + e_step e_u + U (|upd| + those)
    w' = w - upd              e_w = e_upd + U (|w'| + e_upd)                          (an fma commits less)
    length of a tensor        | ||got - w||_2 - lr_t wn | <= ||e_w||_2 over the tensor  (triangle inequality; for an
                              adapted, unclipped tensor ||upd|| = lr_t (wn / un) un = lr_t wn, LAMB's defining property)

Exact, with no bound: found_inf; the step counter; every bit of w / m / v and of the trust table under a skipped step; w's
bits for a tensor with lr_t == 0; trust == 1 (min(1, clip) with a clip) for a tensor that does not adapt or whose wn or un
is an exact zero — the two overridden records make both zeros exact in fp32 and in float64 alike."""
import functools
import math

import torch

import optim_groups_f64 as gf
import tail_f64 as tf
from tail_f64 import U, _Report

# the two overridden records, both tiny plain tensors of group 0 of optim_groups_f64.table_groups (lr 1e-3, wd 0.05)
ZERO_W = 6        # all-zero parameters, a non-zero update: wn = 0
ZERO_ALL = 9      # zero parameters, moments and gradient: un = 0 whatever the weight decay


def lamb_state(table, seed=0):
    recs = tf.optim_state(table, seed)
    for k in (ZERO_W, ZERO_ALL):
        assert table[k]["sn"] is None and table[k]["numel"] <= 8 and k % 3 == 0
        recs[k]["param"] = torch.zeros_like(recs[k]["param"])
    recs[ZERO_ALL]["exp_avg"] = torch.zeros_like(recs[ZERO_ALL]["exp_avg"])
    recs[ZERO_ALL]["exp_avg_sq"] = torch.zeros_like(recs[ZERO_ALL]["exp_avg_sq"])
    return recs


def lamb_grads(table, recs, seed, scale=1.0):
    grads = tf.optim_grads(table, recs, seed, scale)
    grads[ZERO_ALL] = torch.zeros_like(grads[ZERO_ALL])
    return grads


def tensor_rates(recs, hp, lr_dev=None, groups=None, group_hp=None):
    """(lr_t, wd_t) of every tensor, as fp32 values: the group's with groups, else hp's (lr_dev in front of hp's lr)"""
    if groups is not None:
        return [(tf.f32(group_hp[g][0]), tf.f32(group_hp[g][1])) for g in groups]
    return [(tf.f32(lr_dev if lr_dev is not None else hp[0]), tf.f32(hp[4]))] * len(recs)


def reference(recs, grads, hp, grad_scale, step, lamb_hp, lr_dev=None, groups=None, group_hp=None):
    """calm_optim_step_lamb in float64.  recs / grads / hp / grad_scale / step / lr_dev as for tail_f64.optim_reference (the
    state BEFORE the call); lamb_hp = (trust_clip or None, always_adapt); groups: the group of every tensor, or None.
    -> (ref, bound): ref holds norm, found_inf, step, p / m / v (flat float64), w (the parameters before, flat), spans,
    rates, and per tensor wn, un, trust, ratio (unclipped; None where the rule gives 1), exact (trust is exact);
    bound holds norm, p, m, v, wn, un, trust."""
    o_ref, o_bound = tf.optim_reference(recs, grads, hp, grad_scale, step, lr_dev)
    rates = tensor_rates(recs, hp, lr_dev, groups, group_hp)
    spans, at = [], 0
    for r in recs:
        spans.append((at, at + r["param"].numel()))
        at += r["param"].numel()
    w = torch.cat([r["param"].double().reshape(-1) for r in recs])
    ref = dict(found_inf=o_ref["found_inf"], step=o_ref["step"], norm=o_ref["norm"], w=w, spans=spans, rates=rates)
    if o_ref["found_inf"]:
        ref.update(p=w, m=o_ref["m"], v=o_ref["v"])
        return ref, {}
    clip = tf.f32(lamb_hp[0]) if lamb_hp[0] else 0.0
    always = bool(lamb_hp[1])
    b1, b2, eps = (tf.f32(x) for x in hp[1:4])
    t = o_ref["step"]
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    r_bc1, r_bc2 = tf._pow_err(b1, t) / bc1, tf._pow_err(b2, t) / bc2
    rr1 = r_bc1 / (1 - r_bc1)
    isb2 = 1 / math.sqrt(bc2)
    ri2 = (1 - r_bc2) ** -0.5 - 1 + 2 * U
    m, v, e_m, e_v = o_ref["m"], o_ref["v"], o_bound["m"], o_bound["v"]
    sv = v.sqrt()
    e_sv = torch.minimum(torch.where(sv > 0, e_v / sv.clamp_min(1e-300), torch.zeros_like(sv)), e_v.sqrt()) + U * sv
    den = sv * isb2 + eps
    e_den = e_sv * isb2 + sv * isb2 * (ri2 + U) + U * den
    q = m / den
    e_q = e_m / den + m.abs() * e_den / (den * (den - e_den).clamp_min(1e-300)) + 2 * U * q.abs()
    r = q / bc1
    e_r = (e_q / bc1) * (1 + rr1) + r.abs() * rr1 + 2 * U * (r.abs() + e_q / bc1)
    p = w.clone()
    e_p = torch.zeros_like(w)
    WN, UN, TRUST, RATIO, EXACT, E_WN, E_UN, E_TRUST = [], [], [], [], [], [], [], []
    for (lo, hi), (lr, wd) in zip(spans, rates):
        d = tf.optim_sum_depth(hi - lo)
        wt = w[lo:hi]
        dw = wd * wt
        e_dw = U * dw.abs()
        u = r[lo:hi] + dw
        e_u = e_r[lo:hi] + e_dw + U * (u.abs() + e_r[lo:hi] + e_dw)
        W2, U2 = float((wt * wt).sum()), float((u * u).sum())
        e_W2 = (d + 1) * U * W2
        e_U2 = float((2 * u.abs() * e_u + e_u * e_u).sum()) + (d + 1) * U * float(((u.abs() + e_u) ** 2).sum())
        wn, un = math.sqrt(W2), math.sqrt(U2)
        e_wn = min(e_W2 / wn, math.sqrt(e_W2)) if wn > 0 else 0.0
        e_wn += U * (wn + e_wn)
        e_un = min(e_U2 / un, math.sqrt(e_U2)) if un > 0 else 0.0
        e_un += U * (un + e_un)
        adapt = always or wd != 0.0
        if adapt and wn > 0 and un > 0:
            ratio = wn / un
            # un <= e_un: the elements' errors do not separate the update from zero (a gradient that cancels to its own
            # rounding error under r = m / (sqrt(v) + eps)); the reference then decides nothing about this tensor's trust
            # and parameters, and says so with an infinite bound (case() refuses inputs that lead here)
            e_ratio = (e_wn + ratio * e_un) / (un - e_un) if un > e_un else math.inf
            e_ratio += 2 * U * (ratio + e_ratio)
            trust, e_trust, exact = ratio, e_ratio, False
            if clip > 0:
                trust = min(ratio, clip)
                e_trust = e_ratio if ratio - e_ratio < clip else 0.0
        else:
            # (an exact zero norm: every element and every error term of it is zero, so fp32 takes this branch too)
            assert (wn > 0 or e_W2 == 0.0) and (un > 0 or e_U2 == 0.0)
            ratio, trust, e_trust, exact = None, (min(1.0, clip) if clip > 0 else 1.0), 0.0, True
        if lr != 0.0:
            step_ = lr * trust
            e_step = lr * e_trust + U * (step_ + lr * e_trust)
            upd = step_ * u
            p[lo:hi] = wt - upd
            if math.isfinite(e_step):
                e_upd = step_ * e_u + u.abs() * e_step + e_step * e_u
                e_upd = e_upd + U * (upd.abs() + e_upd)
                e_p[lo:hi] = e_upd + U * (p[lo:hi].abs() + e_upd)
            else:
                e_p[lo:hi] = math.inf
        for lst, x in zip((WN, UN, TRUST, RATIO, EXACT, E_WN, E_UN, E_TRUST), (wn, un, trust, ratio, exact, e_wn, e_un, e_trust)):
            lst.append(x)
    ref.update(p=p, m=m, v=v, wn=WN, un=UN, trust=TRUST, ratio=RATIO, exact=EXACT)
    return ref, dict(norm=o_bound["norm"], p=e_p, m=e_m, v=e_v, wn=E_WN, un=E_UN, trust=E_TRUST)


def median_clip(ref):
    """A trust_clip that clips some tensors and leaves others: the fp32 median of the reference's unclipped ratios."""
    ratios = sorted(x for x in ref["ratio"] if x is not None)
    return tf.f32(ratios[len(ratios) // 2]) if ratios else 1.0       # (no tensor adapts: wd = 0 without always_adapt)


def clipped_kinds(ref, bound, clip):
    """(tensors surely clipped, tensors surely not) of a reference made WITH clip"""
    hit = sum(1 for x, e in zip(ref["ratio"], bound["trust"]) if x is not None and x - e > clip)
    free = sum(1 for x, e in zip(ref["ratio"], bound["trust"]) if x is not None and x + e < clip)
    return hit, free


TABLE = tf.optim_table()
MODES = {"plain": (0, False), "always": (1, False), "clip": (0, True), "always_clip": (1, True)}     # always_adapt, a clip
RUNS = [(sc["name"], grouped, mode) for sc in tf.OPTIM_SCENARIOS for grouped in (False, True) for mode in MODES]


@functools.lru_cache(maxsize=None)
def case(name, grouped, mode, nonfinite=None):
    """The inputs of a run with its reference and bounds, made once and shared by every test that needs them (nobody
    modifies them): scenario `name` of tail_f64.OPTIM_SCENARIOS, ungrouped or with optim_groups_f64's groups (a grouped call
    has no lr_dev: the group table holds the rates), MODES[mode]; nonfinite: the name of one of
    tail_f64.optim_nonfinite_cases.  The clip is median_clip of the same run's reference without one."""
    sc = gf.scenario(name)
    always, clipped = MODES[mode]
    recs = lamb_state(TABLE)
    grads = lamb_grads(TABLE, recs, seed=1, scale=sc["grad_scale"] or 1.0)
    if nonfinite is not None:
        _, tensor, element, value = next(c for c in tf.optim_nonfinite_cases(TABLE) if c[0] == nonfinite)
        grads[tensor][element] = value
    kw = dict(groups=gf.table_groups(TABLE), group_hp=gf.GROUP_HP, lr_dev=None) if grouped else \
        dict(groups=None, group_hp=None, lr_dev=sc["lr_dev"])
    hp = gf.hp_of(sc) if grouped else tf.optim_hp(sc)
    clip = None
    if clipped and nonfinite is None:
        clip = median_clip(reference(recs, grads, hp, sc["grad_scale"], sc["t_prev"], (None, always), **kw)[0])
    elif clipped:
        clip = 1.0
    lamb_hp = (clip, always)
    ref, bound = reference(recs, grads, hp, sc["grad_scale"], sc["t_prev"], lamb_hp, **kw)
    assert not bound or all(math.isfinite(e) for e in bound["trust"]), "an update norm is not separated from zero"
    return dict(recs=recs, grads=grads, hp=hp, scale=sc["grad_scale"], step=sc["t_prev"], lamb_hp=lamb_hp, ref=ref, bound=bound,
                sc=sc, **kw)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check(got, ref, bound, strict=True):
    """got: p, m, v (flat fp32), norm, found_inf, step, trust (float32 [n, 3]: wn, un, trust) of a step that was NOT
    skipped, from the state `ref` was made of.  -> (worst, failures)"""
    rep = _Report()
    if got["found_inf"] != ref["found_inf"]:
        rep.fail("found_inf", f"got {got['found_inf']}, expected {ref['found_inf']}")
    if got["step"] != ref["step"]:
        rep.fail("step", f"step count {got['step']}, expected {ref['step']}")
    if ref["found_inf"]:
        rep.fail("found_inf", "the reference skips this step: check_skipped is its checker")
        return rep.done(strict)
    one = lambda x: torch.tensor([float(x)], dtype=torch.float64)              # noqa: E731
    col = lambda x: torch.tensor(x, dtype=torch.float64)                       # noqa: E731
    rep.bounded("norm", one(got["norm"]), one(ref["norm"]), one(bound["norm"]))
    for k in ("m", "v", "p"):
        rep.bounded(k, got[k], ref[k], bound[k])
    table = got["trust"].double().reshape(-1, 3)
    for j, k in enumerate(("wn", "un", "trust")):
        rep.bounded(k, table[:, j], col(ref[k]), col(bound[k]))
    w32 = ref["w"].float()
    for t, ((lo, hi), (lr, _), exact) in enumerate(zip(ref["spans"], ref["rates"], ref["exact"])):
        if exact and float(table[t, 2]) != ref["trust"][t]:
            rep.fail("trust", f"tensor {t}: trust {float(table[t, 2])!r}, expected exactly {ref['trust'][t]!r}")
        if lr == 0.0 and not _same_bits(got["p"][lo:hi], w32[lo:hi]):
            rep.fail("p", f"tensor {t} has lr 0 and its parameters changed")
    return rep.done(strict)


def check_length(got, ref, bound, strict=True):
    """LAMB's defining property on every tensor that adapts, is not clipped and has positive norms: the step's length is
    lr_t ||w||.  -> (worst, failures, tensors checked)"""
    rep = _Report()
    lens, want, lim = [], [], []
    for t, ((lo, hi), (lr, _)) in enumerate(zip(ref["spans"], ref["rates"])):
        if ref["ratio"][t] is None or ref["trust"][t] != ref["ratio"][t]:
            continue
        lens.append(float((got["p"][lo:hi].double() - ref["w"][lo:hi]).norm()))
        want.append(lr * ref["wn"][t])
        lim.append(float(bound["p"][lo:hi].norm()) + 1e-12 * want[-1])            # (the float64 evaluation itself)
    col = lambda x: torch.tensor(x, dtype=torch.float64)                       # noqa: E731
    rep.bounded("length", col(lens), col(want), col(lim))
    return rep.done(strict) + (len(lens),)


def check_skipped(got, before, step_before, trust_before, strict=True):
    """A step with a non-finite gradient: tail_f64.check_optim_skipped, and the trust table's bits as before."""
    worst, failures = tf.check_optim_skipped(got, before, step_before, strict=False)
    if not _same_bits(got["trust"].reshape(-1), trust_before.reshape(-1)):
        failures.append(("trust", "the trust table changed under a skipped step"))
    if strict:
        assert not failures, failures
    return worst, failures
