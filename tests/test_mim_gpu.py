"""The masked-image-modelling kernels on the MI355X: calm_mim_draw against the emulation byte for byte (the cases of
tests/mim_f64.py, k = 0 / P, the high words of sample0, the two tie samples, the split batch), calm_mim_apply bit for bit (in
place, a base misaligned by one float), calm_mim_huber_fwd / _bwd against float64 (two deltas, two dloss, drawn / uneven /
one-patch / full masks, misaligned bases, exact zeros and NaN behaviour outside and inside the mask, repeatability), and two
RegTrainStep(mim=) steps of the nano-48 generative model with the loss kernels on against the same steps with them off."""
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import emulated_mim as E
import weights as W
import mim_f64 as F
from emulated_dropout import KeyStream
from helpers import rel_err
from test_host_logic_cpu import build_model

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
TOL_STEP = 1e-3                     # the project's fp32 bound (TOL of test_model_gpu.py)


@pytest.fixture(autouse=True)
def _restore():
    yield
    calm.backend.set_loss_kernels(False)
    calm.ops.set_dropout_key_override(None)


def _shifted(t, lead, fill=7.0, tail=8):
    """`t` copied to the device at a base `lead` floats behind a 16-byte aligned one, `tail` guard elements behind it."""
    buf = torch.full((lead + t.numel() + tail,), fill, dtype=t.dtype, device="cuda")
    view = buf[lead:lead + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * lead
    return buf, view


class HipImpl:
    """The kernels behind the checker's interface; every call also checks that nothing was written outside its output."""

    def __init__(self):
        self.be = calm.backend.get_backend()

    def draw(self, B, G, k, key, sample0):
        buf = torch.full((B * G * G + 16,), 9, dtype=torch.uint8, device="cuda")
        mask = buf[:B * G * G].view(B, G * G)
        self.be.mim_draw(mask, B, G, k, torch.tensor(key, dtype=torch.int64, device="cuda"), sample0)
        assert (buf[B * G * G:] == 9).all()
        return mask.cpu()

    def apply(self, x, mask, fill, p, in_place, lead):
        B, S, _ = x.shape
        xbuf, xs = _shifted(x, lead)
        ybuf, ys = (xbuf, xs) if in_place else _shifted(torch.empty_like(x), lead)
        self.be.mim_apply(xs, ys, mask.cuda(), fill, B, S, p)
        assert (ybuf[:lead] == 7.0).all() and (ybuf[lead + x.numel():] == 7.0).all()
        return ys.cpu()

    def huber(self, tokens, target, mask, delta, dloss, p, masked, lead):
        B, S, _ = tokens.shape
        (_, t), (_, g) = _shifted(tokens, lead), _shifted(target, lead)
        dbuf, d = _shifted(torch.empty_like(tokens), lead)
        m = mask.cuda()
        loss = torch.full((), 5.0, device="cuda")
        self.be.mim_huber_fwd(t, g, m, delta, loss, B, S, p, masked)
        self.be.mim_huber_bwd(t, g, m, delta, torch.tensor([dloss], device="cuda"), d, B, S, p, masked)
        assert (dbuf[:lead] == 7.0).all() and (dbuf[lead + tokens.numel():] == 7.0).all()
        return loss.cpu(), d.cpu()


# ---- calm_mim_draw -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", F.DRAW_CASES, ids=lambda c: "B{}_S{}_p{}_k{}".format(*c))
def test_draw_matches_the_definition_and_the_emulation_byte_for_byte(case):
    impl = HipImpl()
    assert F.check_draw(impl, [case], ties=False) == []
    B, S, p, k = case
    got = impl.draw(B, S // p, k, F.KEY, F.SAMPLE0)
    assert np.array_equal(got.numpy(), E.draw(F.KEY, F.SAMPLE0, B, S // p, k))


def test_draw_sends_equal_words_to_the_lower_index():
    assert F.check_draw(HipImpl(), [], ties=True) == []


def test_draw_on_more_samples_than_the_grid_and_under_the_default_key_source():
    """70 000 samples (the grid is capped at 65 536 workgroups: some own two) at G = 2; then the frequencies of the CPU test."""
    impl = HipImpl()
    B = 70000
    got = impl.draw(B, 2, 2, F.KEY, 5)
    assert np.array_equal(got.numpy(), E.draw(F.KEY, 5, B, 2, 2))
    freq = impl.draw(4096, 4, 8, F.KEY, F.SAMPLE0).float().mean(dim=0)
    assert bool(((freq - 0.5).abs() < 4 * np.sqrt(0.25 / 4096)).all())
    torch.manual_seed(5)
    a = trainer.MaskedImageModelling(8).draw(4, 48, torch.device("cuda"))
    torch.manual_seed(5)
    b = trainer.MaskedImageModelling(8).draw(4, 48, torch.device("cuda"))
    c = trainer.MaskedImageModelling(8).draw(4, 48, torch.device("cuda"))
    assert torch.equal(a, b) and not torch.equal(a, c) and bool((a.sum(dim=1) == 22).all())


# ---- calm_mim_apply ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", F.HUBER_CASES, ids=lambda c: "B{}_S{}_p{}".format(*c))
def test_apply_is_the_select_bit_for_bit(case):
    assert F.check_apply(HipImpl(), [case]) == []


# ---- calm_mim_huber_fwd / _bwd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", F.HUBER_CASES, ids=lambda c: "B{}_S{}_p{}".format(*c))
def test_huber_pair_against_float64(case):
    found = F.check_huber(HipImpl(), [case], verbose=True)
    assert found == [], found


def test_two_calls_agree_bit_for_bit_and_the_scratch_plan_holds():
    impl = HipImpl()
    B, S, p = 2, 224, 16
    tokens, target = F.inputs(B, S)
    mask = F.masks(B, S, p)["drawn"]
    a = impl.huber(tokens, target, mask, 1.0, 3.0, p, int(mask.sum()), 0)
    b = impl.huber(tokens, target, mask, 1.0, 3.0, p, int(mask.sum()), 0)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    # the forward writes no more partials than calm_reduce_scratch_floats promises
    from calm_vit_dte_amd import _lib as binding
    be = impl.be
    need = int(be.lib.calm_reduce_scratch_floats(binding.RED_MIM, B, S))
    part = torch.full((need + 64,), 3.0, device="cuda")
    loss = torch.empty((), device="cuda")
    t, g, m = tokens.cuda(), target.cuda(), mask.cuda()
    rc = be.lib.calm_mim_huber_fwd(t.data_ptr(), g.data_ptr(), m.data_ptr(), 1.0, loss.data_ptr(), B, S, p, int(mask.sum()),
                                   part.data_ptr(), calm.backend._stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool((part[need:] == 3.0).all())


def test_mim_huber_fn_on_the_device():
    B, S, p = 2, 24, 6
    tokens, target = F.inputs(B, S)
    mask = F.masks(B, S, p)["uneven"]
    t = tokens.cuda().requires_grad_(True)
    loss = calm.ops.MimHuberFn.apply(t, target.cuda(), mask.cuda(), 1.0, int(mask.sum()))
    (loss * 3.0).backward()
    ref = F.ref_huber(tokens, target, mask.numpy(), 1.0, 3.0, p, int(mask.sum()))
    assert abs(float(loss.detach()) - float(ref[0])) <= F.TOL * float(ref[0]) and rel_err(t.grad, ref[1]) <= F.TOL


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_two_steps_with_the_loss_kernels_on_match_the_steps_with_them_off():
    x = (torch.randn(4, 3, 48, 48, generator=torch.Generator().manual_seed(4)) * 0.5).cuda()
    mim = {"patch": 8, "ratio": 0.6}
    runs, masks, keys = {}, [], []
    real = trainer.MaskedImageModelling.draw

    def recording(stream):
        def draw_key(device):
            keys.append(stream(device))
            return keys[-1]
        return draw_key

    def spying(self, B, S, device):
        first = len(keys)                                            # the key this draw takes is the next one
        masks.append((real(self, B, S, device).cpu(), first))
        return masks[-1][0].to(device)
    trainer.MaskedImageModelling.draw = spying
    try:
        for kernels in (False, True):
            calm.backend.set_loss_kernels(kernels)
            calm.ops.set_dropout_key_override(recording(KeyStream(F.SEED)))
            calm.ops.set_noise_override(W.NoiseStream(9))
            m = build_model("nano48_gen", None, "cuda").train()
            opt = trainer.FusedClipAdamW(m)
            try:
                step = trainer.RegTrainStep(m, opt, mim=mim)
                losses = [float(step(x)[0]) for _ in range(2)]
            finally:
                opt.close()
            runs[kernels] = (losses, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    finally:
        trainer.MaskedImageModelling.draw = real
        calm.ops.set_noise_override(None)
    assert len(masks) == 4                                           # one mask per forward, and it is the emulation's
    for i, (got, first) in enumerate(masks):
        assert np.array_equal(got.numpy(), E.draw([int(v) for v in keys[first]], 0, 4, 6, 22)), i
    assert not torch.equal(masks[0][0], masks[1][0]) and torch.equal(masks[0][0], masks[2][0])
    print(runs[False][0], runs[True][0])
    for a, b in zip(runs[True][0], runs[False][0]):
        assert abs(a - b) <= TOL_STEP * abs(b)
    figs = {k: rel_err(runs[True][1][k], v) for k, v in runs[False][1].items() if v.is_floating_point()}
    worst = sorted(figs.items(), key=lambda kv: -kv[1])[:3]
    print(worst)
    assert all(v <= TOL_STEP for v in figs.values()), worst
