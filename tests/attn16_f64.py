"""Staged float64 reference and element-wise bounds for the bf16 latent-mask attention (calm_attention16_fwd / _bwd).

An end-to-end float64 comparison says nothing here: the kernels round R, hp, hg and the mask to bf16 on the way, and one
bf16 ulp of a mask value near 20 is 0.125 in the logits.  So every stage is referenced from the checked implementation's
OWN stored output of the stage before it (R_got -> hp, hg; hg_got -> Mk; Mk_got -> lse, out; out_got / Mk_got / lse_got
-> the backward).  Each stage then carries only its fp32 accumulation error plus at most one bf16 rounding, and both can
be bounded element by element:

    U32 = 2^-24   unit roundoff of fp32
    U16 = 2^-8    unit roundoff of bf16 under round-to-nearest-even (half of the 2^-7 spacing of [1, 2))
    dot(n, T)     (n + 8) U32 T: an fp32 dot product of n terms whose absolute values sum to T.  Any summation order
                  has error <= (n - 1) U32 T to first order (bf16 x bf16 products are exact in fp32); the 8 covers the
                  epilogue's few roundings (1 / sigma, the scale, the bias add), each <= U32 of a quantity <= T

check_forward / check_backward take CPU tensors, return (worst, failures): worst[name] = max error / bound of the
outputs that have a bound of their own, failures = a list of (name, message).  With strict=True (the default) a non-empty
list raises AssertionError.  The module knows nothing about who produced the tensors: the GPU tests hand it the kernels'
outputs, the CPU tests the emulation's (and planted faults on copies of them)."""
import math

import torch


U32 = 2.0 ** -24
U16 = 2.0 ** -8
MIN_EQUAL = 0.99          # share of elements that must BE the rounded reference, among those counted (see bf16_stage)
COUNT_ULP_FRACTION = 32   # counted: elements whose fp32 bound is <= 1/32 of a bf16 ulp of the reference

FILL = {torch.float32: 0x7FC0DEAD, torch.bfloat16: 0x7FDE}   # quiet NaNs with payloads no arithmetic yields
GELU_FWD_ERR = 1.39e-7    # gelu_erf_f of common.h against float64, measured: see the docstring of test_rowwise_f64_gpu.py
GELU_BWD_ERR = 2.85e-7    # gelu_erf_grad_f of common.h against float64, measured there as well

FWD_NAMES = ("out", "R", "hp", "hg", "Mk", "MkT", "lse")
BWD_NAMES = ("delta", "dq", "dk", "dv", "dM")


# ------------------------------------------------------------------------------------------------- the 48 instances
def instance_of(S, hd):
    """(NP, HDP) of with_shape16 in csrc/attention_bf16.hip"""
    return -(-S // 32), 32 * -(-hd // 32)


def sweep_cases():
    """One (S, hd) per compiled instance: key counts short of 32 NP by 0 / 8 / 16 / 24, head dims short of HDP by 0..28
    (hd % 8 == 4 in half of them); the smallest is S = 8 at (1, 64)."""
    cases = []
    for NP in range(1, 13):
        for HDP in (32, 64, 96, 128):
            S = 32 * NP - 8 * ((NP + HDP // 32) % 4)
            hd = HDP - 4 * ((3 * NP + HDP // 32) % 8)
            assert instance_of(S, hd) == (NP, HDP)
            cases.append((S, hd))
    return cases


def pipelined_capable(S, hd):
    """Fwd2Geo / Bwd2Geo OK: the instances that have the pipelined kernels next to the register-staged ones"""
    NP, HDP = instance_of(S, hd)
    return NP <= 7 and HDP <= 64


EXTRA_SHAPES = [(8, 4), (384, 128), (32, 32), (64, 64), (224, 64), (232, 64), (224, 68), (320, 32)]


def make_inputs(B, S, H, hd, seed=0):
    """q, k, v, w1, b1, s1, w2, b2, s2 (the distribution of test_attention16_gpu._inputs) and dout"""
    g = torch.Generator().manual_seed(seed)
    D = H * hd
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc)
    q, k, v = rn(B, S, D, sc=0.5).bfloat16(), rn(B, S, D, sc=0.5).bfloat16(), rn(B, S, D).bfloat16()
    w1, w2 = rn(2 * S, S, sc=S ** -0.5).bfloat16(), rn(S, 2 * S, sc=(2 * S) ** -0.5).bfloat16()
    b1, b2 = rn(2 * S, sc=0.1), rn(S, sc=0.1)
    s1, s2 = torch.tensor([1.3]), torch.tensor([0.8])
    dout = torch.randn(B, S, D, generator=torch.Generator().manual_seed(seed + 101)).bfloat16()
    return (q, k, v, w1, b1, s1, w2, b2, s2), dout


# ------------------------------------------------------------------------------------------------------- primitives
def dot_bound(n, terms):
    return (n + 8) * U32 * terms


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def bf16_ulp(ref64):
    """spacing of bf16 at |ref|: 2^(floor(log2 |ref|) - 7); 0 at 0 (such elements are never counted)"""
    _, e = torch.frexp(ref64.abs())                       # |ref| = m 2^e, m in [0.5, 1)
    return torch.where(ref64 == 0, torch.zeros_like(ref64), torch.ldexp(torch.ones_like(ref64), e - 8))


def bf16_ord(t):
    """bf16 values as integers ordered like the values, adjacent representables one apart (+0 and -0 both 0)."""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def assert_bf16_rounding_of(got, ref64, fp32_bound, min_equal=0.99, count=None):
    """bf16 result of an fp32 computation whose own error is <= fp32_bound: at least `min_equal` of the elements are
    the float64 reference rounded once (RNE), the rest one bf16 ulp away — or, where the fp32 bound exceeds a bf16 ulp
    (values near 0, cancellation), within that bound plus the rounding.  An fp32 error of a few u moves a value across
    a bf16 rounding boundary with probability ~ (few u) / 2^-8 < 1e-4 per element.  `count` (a boolean mask) restricts
    the share to the elements it selects, for outputs whose fp32 bound is not small against a bf16 ulp everywhere."""
    r = ref64.to(torch.bfloat16)
    d = (bf16_ord(got) - bf16_ord(r)).abs()
    near = (got.double() - ref64).abs() <= fp32_bound + 2.0 ** -8 * ref64.abs()
    assert bool(((d <= 1) | near).all()), f"bf16 output {int(d[~near].max())} ulps from the rounded reference"
    eq = d == 0 if count is None else (d == 0)[count]
    assert eq.numel() == 0 or float(eq.double().mean()) >= min_equal, \
        f"only {float(eq.double().mean()):.4f} of {eq.numel()} elements equal the rounded reference"


class _Report:
    def __init__(self):
        self.worst, self.failures = {}, []

    def fail(self, name, msg):
        self.failures.append((name, msg))

    def bounded(self, name, got, ref64, bound):
        """|got - ref| <= bound element-wise (a NaN / inf in got fails); records max error / bound"""
        err = (got.double() - ref64).abs()
        ok = err <= bound
        ratio = err / bound
        self.worst[name] = float(ratio[torch.isfinite(ratio)].max()) if bool(torch.isfinite(ratio).any()) else float("inf")
        if not bool(ok.all()):
            bad = ~ok
            idx = tuple(int(i) for i in bad.nonzero()[0])
            self.fail(name, f"{int(bad.sum())} elements outside the bound, first at {idx}: got {float(got[idx])!r}, "
                            f"ref {float(ref64[idx])!r}, bound {float(bound[idx]):.3e}")

    def bf16_stage(self, name, got, ref64, fp32_bound):
        """got = one bf16 rounding of an fp32 result whose own error is <= fp32_bound.  Every element is the RNE-rounded
        reference, or one bf16 ulp from it, or within fp32_bound + U16 |ref|; and among the elements whose fp32_bound is
        at most 1/32 of a bf16 ulp of the reference at least 99 % ARE the rounded reference (an fp32 error of e moves
        a value across a rounding boundary with probability ~ 2 e / ulp <= 1/16 even if every element sat at its
        worst-case bound; the errors are in fact ~ sqrt(n) U32, not n U32, which puts the expected share of flips
        below 1e-3).  The cap keeps the "one ulp away" clause from hiding a kernel that is systematically off."""
        counted = fp32_bound * COUNT_ULP_FRACTION <= bf16_ulp(ref64)
        finite = torch.isfinite(got.float())
        if not bool(finite.all()):
            self.fail(name, f"{int((~finite).sum())} non-finite elements, first at {tuple(int(i) for i in (~finite).nonzero()[0])}")
        try:
            assert_bf16_rounding_of(got, ref64, fp32_bound, MIN_EQUAL, count=counted)
        except AssertionError as e:
            self.fail(name, str(e))
        d = (bf16_ord(got) - bf16_ord(ref64.to(torch.bfloat16))).abs()
        n = int(counted.sum())
        self.worst[name + ":equal"] = float((d[counted] == 0).double().mean()) if n else 1.0
        self.worst[name + ":counted"] = n / max(1, ref64.numel())
        # error / bound of the third clause, for the record (elements one ulp away may exceed 1: that clause allows them)
        ratio = (got.double() - ref64).abs() / (fp32_bound + U16 * ref64.abs())
        fin = torch.isfinite(ratio)
        self.worst[name] = float(ratio[fin].max()) if bool(fin.any()) else float("inf")

    def done(self, strict):
        if strict and self.failures:
            raise AssertionError("; ".join(f"{n}: {m}" for n, m in self.failures))
        return self.worst, self.failures


def _heads(t, B, S, H, hd):
    return t.double().view(B, S, H, hd).transpose(1, 2)          # [B, H, S, hd]


def _unheads(t, B, S, H, hd):
    return t.transpose(1, 2).reshape(B, S, H * hd)


def _logits(q, k, Mk, B, S, H, hd):
    """float64 logits from the bf16 q, k and the STORED mask, and their fp32 bound: hd products, the scale, one add"""
    sc = 1.0 / math.sqrt(hd)
    qh, kh = _heads(q, B, S, H, hd), _heads(k, B, S, H, hd)
    m = Mk.double().view(B, 1, S, S)
    logits = sc * (qh @ kh.transpose(-1, -2)) + m
    e_l = dot_bound(hd, sc * (qh.abs() @ kh.abs().transpose(-1, -2)) + m.abs())
    return logits, e_l


def _exp_rel(x):
    """relative error of the fp32 exp(x), x = logit - (max or lse): the subtraction and the product with log2 e round
    the argument by <= 2 U32 |x| (absolute in the argument = relative in the result), v_exp_f32 and the store 2 U32"""
    return 4 * U32 * (1 + x.abs())


# ---------------------------------------------------------------------------------------------------------- forward
def forward_reference(ins, got, B, S, H, hd):
    """The float64 stages and their fp32 bounds, each from `got`'s stored output of the stage before it."""
    q, k, v, w1, b1, s1, w2, b2, s2 = ins
    D = H * hd
    q3, k3 = q.double().view(B, S, D), k.double().view(B, S, D)
    ref, bound = {}, {}
    # R = q k^T over all D = H hd columns
    ref["R"] = q3 @ k3.transpose(1, 2)
    bound["R"] = dot_bound(D, q3.abs() @ k3.abs().transpose(1, 2))
    # pre = R_got w1^T / s1 + b1: S products, then the 1 / s1 scale and the bias (inside dot_bound's + 8)
    Rg, w1d = got["R"].double().view(B, S, S), w1.double()
    ref["hp"] = Rg @ w1d.t() / s1.double() + b1.double()
    bound["hp"] = dot_bound(S, Rg.abs() @ w1d.abs().t() / s1.double() + b1.double().abs())
    # hg = gelu(pre) of the fp32 pre-activation (not of the stored hp): |gelu'| <= 1.13 carries pre's error over, the
    # kernel's GELU is within GELU_FWD_ERR max(1, |x|) of the exact one (measured once, asserted at twice that)
    ref["hg"] = gelu64(ref["hp"])
    bound["hg"] = 1.13 * bound["hp"] + 2 * GELU_FWD_ERR * ref["hp"].abs().clamp_min(1.0)
    # Mk = hg_got w2^T / s2 + b2: 2 S products
    hgg, w2d = got["hg"].double().view(B, S, 2 * S), w2.double()
    ref["Mk"] = hgg @ w2d.t() / s2.double() + b2.double()
    bound["Mk"] = dot_bound(2 * S, hgg.abs() @ w2d.abs().t() / s2.double() + b2.double().abs())
    # logits = scale q_h k_h^T + Mk_got; lse = logsumexp: 1-Lipschitz in the max norm of the logits' error, plus
    # (S / 64 + 16) U32 (1 + |lse|) for exp, log and the row sum (a wave sums its S / 64 logits per lane, then a tree)
    logits, e_l = _logits(q, k, got["Mk"], B, S, H, hd)
    lse = torch.logsumexp(logits, dim=-1)
    ref["lse"] = lse
    bound["lse"] = e_l.amax(dim=-1) + (S / 64 + 16) * U32 * (1 + lse.abs())
    # out = bf16(P) v_h: the output's rounding U16 |ref|; P's rounding to bf16 U16 sum P |v|; the fp32 P itself is off
    # by eps_P relative = logit error + lse error + exp; the P.V accumulation over S keys
    P = torch.exp(logits - lse.unsqueeze(-1))
    vh = _heads(v, B, S, H, hd)
    eps_p = e_l + bound["lse"].unsqueeze(-1) + _exp_rel(logits - lse.unsqueeze(-1))
    o = P @ vh
    ob = U16 * o.abs() + (U16 * P + eps_p * P) @ vh.abs() + dot_bound(S, P @ vh.abs())
    ref["out"], bound["out"] = _unheads(o, B, S, H, hd), _unheads(ob, B, S, H, hd)
    return ref, bound


def check_forward(ins, got, B, S, H, hd, strict=True):
    ref, bound = forward_reference(ins, got, B, S, H, hd)
    rep = _Report()
    rep.bf16_stage("R", got["R"].view(B, S, S), ref["R"], bound["R"])
    rep.bf16_stage("hp", got["hp"].view(B, S, 2 * S), ref["hp"], bound["hp"])
    rep.bf16_stage("hg", got["hg"].view(B, S, 2 * S), ref["hg"], bound["hg"])
    rep.bf16_stage("Mk", got["Mk"].view(B, S, S), ref["Mk"], bound["Mk"])
    if not torch.equal(bf16_ord(got["MkT"].view(B, S, S)), bf16_ord(got["Mk"].view(B, S, S).transpose(1, 2).contiguous())):
        rep.fail("MkT", "not the bit-exact transpose of Mk")
    rep.bounded("lse", got["lse"].view(B, H, S), ref["lse"], bound["lse"])
    rep.bounded("out", got["out"].view(B, S, H * hd), ref["out"], bound["out"])
    return rep.done(strict)


# --------------------------------------------------------------------------------------------------------- backward
def backward_reference(ins, saved, dout, B, S, H, hd):
    """saved: out, Mk, lse as stored by a forward of the implementation under test.  P = exp(logits - lse_got)."""
    q, k, v = ins[:3]
    sc = 1.0 / math.sqrt(hd)
    qh, kh, vh, oh, doh = (_heads(t, B, S, H, hd) for t in (q, k, v, saved["out"], dout))
    ref, bound = {}, {}
    # delta = rowsum(dO o out_got): hd products
    delta = (doh * oh).sum(-1)
    e_delta = dot_bound(hd, (doh.abs() * oh.abs()).sum(-1))
    ref["delta"], bound["delta"] = delta, e_delta
    logits, e_l = _logits(q, k, saved["Mk"], B, S, H, hd)
    x = logits - saved["lse"].double().view(B, H, S, 1)
    P = torch.exp(x)
    eps_p = e_l + _exp_rel(x)                                   # relative error of the fp32 P
    dP = doh @ vh.transpose(-1, -2)
    e_dp = dot_bound(hd, doh.abs() @ vh.abs().transpose(-1, -2))
    t = dP - delta.unsqueeze(-1)
    dS = P * t
    # fp32 dS = P (dP - delta): P's relative error on the whole product, the errors of dP and delta and the roundings
    # of the subtraction and the product scaled by P
    e_ds = eps_p * dS.abs() + P * (e_dp + e_delta.unsqueeze(-1) + 2 * U32 * (dP.abs() + delta.abs().unsqueeze(-1)))
    # dM = sum_h dS in fp32, rounded once
    ref["dM"] = dS.sum(1)
    bound["dM"] = e_ds.sum(1) + dot_bound(H, dS.abs().sum(1))
    # dq = scale bf16(dS) k_h, dk = scale bf16(dS)^T q_h, dv = bf16(P)^T dO_h: the output's rounding U16 |ref|, the
    # operand's rounding U16 sum |operand| |other|, the operand's fp32 error, the accumulation over S
    dq = sc * (dS @ kh)
    bq = U16 * dq.abs() + sc * ((U16 * dS.abs() + e_ds) @ kh.abs()) + dot_bound(S, sc * (dS.abs() @ kh.abs()))
    dk = sc * (dS.transpose(-1, -2) @ qh)
    bk = U16 * dk.abs() + sc * ((U16 * dS.abs() + e_ds).transpose(-1, -2) @ qh.abs()) \
        + dot_bound(S, sc * (dS.abs().transpose(-1, -2) @ qh.abs()))
    dv = P.transpose(-1, -2) @ doh
    bv = U16 * dv.abs() + ((U16 + eps_p) * P).transpose(-1, -2) @ doh.abs() + dot_bound(S, P.transpose(-1, -2) @ doh.abs())
    for n, r, b in (("dq", dq, bq), ("dk", dk, bk), ("dv", dv, bv)):
        ref[n], bound[n] = _unheads(r, B, S, H, hd), _unheads(b, B, S, H, hd)
    ref["dS"] = dS
    return ref, bound


def check_backward(ins, saved, dout, got, B, S, H, hd, strict=True):
    ref, bound = backward_reference(ins, saved, dout, B, S, H, hd)
    rep = _Report()
    rep.bounded("delta", got["delta"].view(B, H, S), ref["delta"], bound["delta"])
    rep.bf16_stage("dM", got["dM"].view(B, S, S), ref["dM"], bound["dM"])
    for n in ("dq", "dk", "dv"):
        rep.bounded(n, got[n].view(B, S, H * hd), ref[n], bound[n])
    return rep.done(strict)
