"""The staged float64 checker of the bf16 attention (tests/attn16_f64.py) on a machine without a GPU: the fp32 emulation
of the kernels' rounding points (EmulatedBackend.attn16_fwd / attn16_bwd) stays inside every bound and every 99 % share
at every case the GPU file sweeps, and faults planted on copies of the emulation's outputs are caught — each by the
output it corrupts.  The planted faults are the ones a max-norm tolerance lets through: a pad key at weight 1 %, a
dropped key, a neighbour's lse, a shifted tile, a missing head, an untransposed tile, a stale element."""
import math

import pytest
import torch

import attn16_f64 as A
from attn16_f64 import FILL
from emulated_backend import EmulatedBackend

B, H = 2, 3
CASES = A.sweep_cases() + A.EXTRA_SHAPES
FAULT_SHAPES = [(72, 20), (200, 100)]          # ragged keys and hd % 8 == 4; both have S >= 64 for the 32 x 32 tile


def emulate(B, S, H, hd, seed):
    emu = EmulatedBackend()
    ins, dout = A.make_inputs(B, S, H, hd, seed=seed)
    D = H * hd
    bf = lambda *s: torch.full(s, float("nan"), dtype=torch.bfloat16)
    fwd = dict(out=bf(B, S, D), R=bf(B, S, S), hp=bf(B, S, 2 * S), hg=bf(B, S, 2 * S), Mk=bf(B, S, S), MkT=bf(B, S, S),
               lse=torch.full((B, H, S), float("nan")))
    emu.attn16_fwd(*ins, *[fwd[n] for n in A.FWD_NAMES], B, S, H, hd)
    bwd = dict(delta=torch.full((B, H, S), float("nan")), dq=bf(B, S, D), dk=bf(B, S, D), dv=bf(B, S, D), dM=bf(B, S, S))
    q, k, v = ins[:3]
    emu.attn16_bwd(q, k, v, fwd["out"], dout, fwd["Mk"], fwd["MkT"], fwd["lse"], *[bwd[n] for n in A.BWD_NAMES],
                   B, S, H, hd)
    return ins, dout, fwd, bwd


def test_sweep_reaches_every_compiled_instance():
    every = {(NP, HDP) for NP in range(1, 13) for HDP in (32, 64, 96, 128)}
    sweep = A.sweep_cases()
    assert len(sweep) == 48 and {A.instance_of(*c) for c in sweep} == every
    assert sum(A.pipelined_capable(*c) for c in sweep) == 14
    assert min(sweep) == (8, 44) and all(S % 8 == 0 and hd % 4 == 0 for S, hd in sweep)


@pytest.mark.parametrize("S,hd", CASES, ids=[f"{S}-{hd}" for S, hd in CASES])
def test_emulation_is_inside_every_bound(S, hd):
    ins, dout, fwd, bwd = emulate(B, S, H, hd, seed=S + hd)
    wf, _ = A.check_forward(ins, fwd, B, S, H, hd)
    wb, _ = A.check_backward(ins, fwd, dout, bwd, B, S, H, hd)
    print("attn16_f64 emu", S, hd, " ".join(f"{k}={v:.4g}" for k, v in sorted({**wf, **wb}.items())))


def test_bf16_unit_roundoff_is_two_to_the_minus_eight():
    """1 + 2^-8 is the midpoint of [1, 1 + 2^-7]: rounding moves a value by up to 2^-8 relative, not 2^-9"""
    x = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20], dtype=torch.float64)
    assert float((x.bfloat16().double() - x).abs() / x) > 0.99 * A.U16
    assert float(A.bf16_ulp(torch.tensor([1.5], dtype=torch.float64))) == 2.0 ** -7
    assert float(A.bf16_ulp(torch.tensor([-0.75], dtype=torch.float64))) == 2.0 ** -8


@pytest.fixture(scope="module", params=FAULT_SHAPES, ids=lambda p: f"{p[0]}-{p[1]}")
def clean(request):
    S, hd = request.param
    return (S, hd) + emulate(B, S, H, hd, seed=7)


def _copy(d):
    return {n: t.clone() for n, t in d.items()}


def _flagged_fwd(clean, fwd):
    S, hd, ins, dout, _, _ = clean
    return {n for n, _ in A.check_forward(ins, fwd, B, S, H, hd, strict=False)[1]}


def _flagged_bwd(clean, bwd):
    S, hd, ins, dout, fwd, _ = clean
    return {n for n, _ in A.check_backward(ins, fwd, dout, bwd, B, S, H, hd, strict=False)[1]}


def test_unplanted_copies_pass(clean):
    S, hd, ins, dout, fwd, bwd = clean
    assert _flagged_fwd(clean, _copy(fwd)) == set() and _flagged_bwd(clean, _copy(bwd)) == set()
    A.check_forward(ins, _copy(fwd), B, S, H, hd)
    A.check_backward(ins, fwd, dout, _copy(bwd), B, S, H, hd)


def _row_softmax(clean, b, h, i):
    """float64 logits of one query row from the emulation's stored mask, and v of that head"""
    S, hd, ins, _, fwd, _ = clean
    q, k, v = ins[:3]
    sl = slice(h * hd, (h + 1) * hd)
    x = q[b, i, sl].double() @ k[b, :, sl].double().t() / math.sqrt(hd) + fwd["Mk"][b, i].double()
    return x, v[b, :, sl].double(), sl


def test_a_pad_key_at_one_percent_is_caught(clean):
    """One query row whose softmax includes one extra key (a pad key: zero V row) at weight ~ 1 %: every real weight
    shrinks by 1 / 1.01 and lse grows by log 1.01 = 1e-2, a thousand times its bound.  (out moves by 1 % of itself,
    which is of the size of its own bf16 bound, 2 U16 = 0.8 %: it is the lse bound that catches this; the next test
    shows from which weight on out is a witness of its own.)"""
    S, hd, ins, dout, fwd, _ = clean
    b, h, i = 1, 1, 7
    x, vh, sl = _row_softmax(clean, b, h, i)
    f = _copy(fwd)
    lse = torch.logsumexp(torch.cat([x, (torch.logsumexp(x, 0) + math.log(0.01)).view(1)]), 0)
    f["lse"][b, h, i] = lse.float()
    f["out"][b, i, sl] = (torch.exp(x - lse) @ vh).bfloat16()
    assert "lse" in _flagged_fwd(clean, f)


@pytest.mark.parametrize("lse_too", [True, False])
def test_a_pad_key_at_ten_percent_is_caught_by_out(clean, lse_too):
    """The limit of the `out` bound, made explicit: out alone cannot see a normalisation error below its own bf16
    bound, U16 |ref| + U16 sum_j P_j |v_j| >= 2 U16 |ref| = 0.8 % of the element (more where the sum cancels), which is
    why the 1 % plant above is caught by lse only.  At weight w the row shrinks by w / (1 + w); an element is outside
    its bound as soon as |sum P v| > U16 sum P |v| / (w / (1 + w) - U16), i.e. 4.5 % of sum P |v| at w = 10 %, and a
    row of hd elements has such an element.  So at 10 % `out` is flagged — also when lse is stored correctly and only
    the normalisation of out is wrong (lse_too = False), where out is the only witness."""
    S, hd, ins, dout, fwd, _ = clean
    b, h, i = 1, 1, 7
    x, vh, sl = _row_softmax(clean, b, h, i)
    f = _copy(fwd)
    lse = torch.logsumexp(torch.cat([x, (torch.logsumexp(x, 0) + math.log(0.10)).view(1)]), 0)
    if lse_too:
        f["lse"][b, h, i] = lse.float()
    f["out"][b, i, sl] = (torch.exp(x - lse) @ vh).bfloat16()
    assert _flagged_fwd(clean, f) == ({"lse", "out"} if lse_too else {"out"})


def test_a_dropped_key_is_caught(clean):
    """One row's softmax without its second-heaviest real key"""
    S, hd, ins, dout, fwd, _ = clean
    b, h, i = 0, 2, S - 1
    x, vh, sl = _row_softmax(clean, b, h, i)
    keep = torch.ones(S, dtype=torch.bool)
    keep[x.argsort(descending=True)[1]] = False
    f = _copy(fwd)
    lse = torch.logsumexp(x[keep], 0)
    f["lse"][b, h, i] = lse.float()
    f["out"][b, i, sl] = (torch.exp(x[keep] - lse) @ vh[keep]).bfloat16()
    flagged = _flagged_fwd(clean, f)
    assert "lse" in flagged


def test_swapped_lse_of_two_heads_is_caught(clean):
    S, hd, ins, dout, fwd, _ = clean
    f = _copy(fwd)
    f["lse"][1, 0], f["lse"][1, 1] = fwd["lse"][1, 1].clone(), fwd["lse"][1, 0].clone()
    assert _flagged_fwd(clean, f) == {"lse"}


def test_a_dk_tile_shifted_by_one_row_is_caught(clean):
    S, hd, ins, dout, fwd, bwd = clean
    g = _copy(bwd)
    g["dk"][1, 16:32, hd:2 * hd] = bwd["dk"][1, 15:31, hd:2 * hd]
    assert _flagged_bwd(clean, g) == {"dk"}


def test_dM_missing_one_head_is_caught(clean):
    S, hd, ins, dout, fwd, bwd = clean
    ref, _ = A.backward_reference(ins, fwd, dout, B, S, H, hd)
    g = _copy(bwd)
    g["dM"][0] = (ref["dM"][0] - ref["dS"][0, H - 1]).bfloat16()
    assert _flagged_bwd(clean, g) == {"dM"}


def test_an_untransposed_MkT_tile_is_caught(clean):
    S, hd, ins, dout, fwd, _ = clean
    f = _copy(fwd)
    f["MkT"][1, 0:32, 32:64] = fwd["Mk"][1, 0:32, 32:64]
    assert _flagged_fwd(clean, f) == {"MkT"}


@pytest.mark.parametrize("name", [n for n in A.FWD_NAMES + A.BWD_NAMES if n != "MkT"])
def test_an_element_left_at_its_prefill_is_caught(clean, name):
    """The payload NaN of the guard buffers in one element of one output (MkT has its own bit-equality test above)"""
    S, hd, ins, dout, fwd, bwd = clean
    src = _copy(fwd if name in A.FWD_NAMES else bwd)
    t = src[name]
    flat = t.view(-1).view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    flat[flat.numel() // 3] = FILL[t.dtype]
    assert torch.isnan(t.view(-1)[flat.numel() // 3])
    flagged = _flagged_fwd(clean, src) if name in A.FWD_NAMES else _flagged_bwd(clean, src)
    assert name in flagged


def test_a_stale_MkT_element_is_caught(clean):
    S, hd, ins, dout, fwd, _ = clean
    f = _copy(fwd)
    f["MkT"][0, 3, 5] = float("nan")
    assert "MkT" in _flagged_fwd(clean, f)
