"""Masked image modelling without a GPU: the emulation of csrc/mim.hip (tests/emulated_mim.py) — exactly k per sample, the
split batch, k = 0 / P, patch frequencies, the tie rule —, the checker (tests/mim_f64.py) on the emulation and on eleven
planted faults, the C-ABI surface (exported, declared, bound, every refusal on fake addresses), ops.MimHuberFn against torch
autograd on trainer.mim_huber_torch, MaskedImageModelling's k table and refusals, RegTrainStep(mim=) against a hand-written
loop under injected keys, train(task="reg", mim=) on one and two gloo ranks against steps that mask themselves (plain,
accumulate=2, sam=), the snapshot header with exact resume, and load_backbone."""
import ctypes
import os
import re
import socket
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import calm_vit_dte_amd as calm
import emulated_mim as E
import mim_f64 as F
from emulated_backend import EmulatedBackend
from emulated_dropout import KeyStream
from helpers import rel_err
from test_host_logic_cpu import build_model
from test_recon_cpu import _GenSet

trainer = import_module("calm_vit_dte_amd.trainer")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "calm_vit.h")
NEW = ("calm_mim_draw", "calm_mim_apply", "calm_mim_huber_fwd", "calm_mim_huber_bwd")
PATCH, MIM = 8, {"patch": 8, "ratio": 0.6}          # the nano-48 model: G = 6, P = 36, k = 22


@pytest.fixture(autouse=True)
def _restore():
    yield
    calm.backend.set_loss_kernels(False)
    calm.ops.set_dropout_key_override(None)


class EmuImpl:
    """The emulated backend behind the checker's interface."""

    def __init__(self, fault=None):
        self.be = E.EmulatedMimBackend()
        self.be.mim_fault = fault

    def draw(self, B, G, k, key, sample0):
        mask = torch.empty(B, G * G, dtype=torch.uint8)
        self.be.mim_draw(mask, B, G, k, torch.tensor(key, dtype=torch.int64), sample0)
        return mask

    def apply(self, x, mask, fill, p, in_place, lead):
        y = x if in_place else torch.empty_like(x)
        self.be.mim_apply(x, y, mask, fill, x.shape[0], x.shape[1], p)
        return y

    def huber(self, tokens, target, mask, delta, dloss, p, masked, lead):
        B, S, _ = tokens.shape
        loss, g = torch.empty(()), torch.empty_like(tokens)
        self.be.mim_huber_fwd(tokens, target, mask, delta, loss, B, S, p, masked)
        self.be.mim_huber_bwd(tokens, target, mask, delta, torch.tensor(dloss), g, B, S, p, masked)
        return loss, g


class TorchImpl:
    """trainer.mim_huber_torch with torch autograd behind the checker's interface."""

    def huber(self, tokens, target, mask, delta, dloss, p, masked, lead):
        t = tokens.clone().requires_grad_(True)
        loss = trainer.mim_huber_torch(t, target, mask, p, delta, masked)
        (loss * dloss).backward()
        return loss.detach(), t.grad


SMALL = [c for c in F.HUBER_CASES if c[1] < 100]


# ---- the emulation ---------------------------------------------------------------------------------------------------------
def test_exactly_k_per_sample_and_k_zero_and_k_all():
    for B, S, p, k in F.DRAW_CASES:
        G = S // p
        assert (E.draw(F.KEY, F.SAMPLE0, B, G, k).sum(axis=1) == k).all()
        assert not E.draw(F.KEY, F.SAMPLE0, B, G, 0).any() and E.draw(F.KEY, F.SAMPLE0, B, G, G * G).all()


def test_a_split_batch_with_sample0_advanced_equals_one_call():
    B, G, k, cut = 11, 5, 9, 3
    one = E.draw(F.KEY, F.SAMPLE0, B, G, k)
    two = np.concatenate([E.draw(F.KEY, F.SAMPLE0, cut, G, k), E.draw(F.KEY, F.SAMPLE0 + cut, B - cut, G, k)])
    assert np.array_equal(one, two)
    assert len({m.tobytes() for m in one}) > 1                       # the samples differ
    assert np.array_equal(E.draw(F.KEY, F.SAMPLE0, 2, 3, 4)[1], E.draw(F.KEY, F.SAMPLE0 + 1, 1, 3, 4)[0])


def test_every_patch_is_masked_half_the_time_within_four_sigma():
    B, G, k = 4096, 4, 8
    freq = E.draw(F.KEY, F.SAMPLE0, B, G, k).mean(axis=0)
    sigma = np.sqrt(0.25 / B)
    print(f"worst patch {np.abs(freq - 0.5).max() / sigma:.2f} sigma")
    assert (np.abs(freq - 0.5) < 4 * sigma).all()


@pytest.mark.parametrize("sample,lo,hi,pos", F.TIES)
def test_equal_words_go_to_the_lower_index(sample, lo, hi, pos):
    w = F.ref_words(F.KEY, sample, 1024)
    assert w[lo] == w[hi] and lo < hi
    order = np.argsort(w, kind="stable")
    assert order[pos - 1] == lo and order[pos] == hi               # sorted positions pos - 1 / pos
    for k, want in ((pos - 1, (0, 0)), (pos, (1, 0)), (pos + 1, (1, 1))):
        m = E.draw(F.KEY, sample, 1, 32, k)[0]
        assert (m[lo], m[hi]) == want and m.sum() == k


# ---- the checker on the emulation and on planted faults ----------------------------------------------------------------------
def test_emulation_agrees_with_the_checker():
    impl = EmuImpl()
    assert F.check_draw(impl) == []
    assert F.check_apply(impl) == []
    assert F.check_huber(impl) == []


def test_the_torch_twin_agrees_with_the_checker():
    assert F.check_huber(TorchImpl()) == []


_DRAW_SMALL = [(3, 8, 4, 2), (5, 12, 3, 8)]


@pytest.mark.parametrize("fault", E.FAULTS)
def test_the_checker_catches_planted_faults(fault):
    impl = EmuImpl(fault)
    if fault in ("tie_high", "rank_le", "stride_P", "sample0"):
        found = F.check_draw(impl, _DRAW_SMALL)
        assert F.check_apply(impl, SMALL[:2]) == [] and F.check_huber(impl, SMALL[:2]) == []
    elif fault == "fill_swapped":
        found = F.check_apply(impl, SMALL)
        assert F.check_draw(impl, _DRAW_SMALL, ties=False) == [] and F.check_huber(impl, SMALL[:2]) == []
    elif fault == "transposed":
        found = F.check_apply(impl, SMALL)
        assert found and F.check_huber(impl, SMALL)
    else:
        found = F.check_huber(impl, SMALL)
        assert F.check_draw(impl, _DRAW_SMALL, ties=False) == [] and F.check_apply(impl, SMALL[:2]) == []
    print(fault, len(found), found[:2])
    assert found
    if fault == "tie_high":
        assert all("tie" in line for line in found)                  # nothing but the two tie samples tells
    if fault == "multiply":
        assert any("outside the mask changed" in line for line in found)     # (and g * 0 is -0.0 where g < 0)


# ---- the C-ABI surface -----------------------------------------------------------------------------------------------------------
_P = 0x7f0000010000                                                  # a fake, 16-byte aligned device address
_DRAW = [_P, 8, 7, 29, 0, _P, None]                                 # mask, B, G, k, sample0, key, stream
_APPLY = [_P, _P, _P, (ctypes.c_float * 3)(0, 0, 0), 8, 224, 32, None]          # x, y, mask, fill, B, S, p, stream
_FWD = [_P, _P, _P, 1.0, _P, 8, 224, 32, 8 * 29, _P, None]          # tokens, target, mask, delta, loss, B, S, p, masked, partials
_BWD = [_P, _P, _P, 1.0, _P, _P, 8, 224, 32, 8 * 29, None]          # tokens, target, mask, delta, dloss, dtokens, B, S, p, masked
INVAL, UNSUPP, LAYOUT = "E_INVAL", "E_UNSUPP", "E_LAYOUT"
_DRAW_REFUSED = [({0: None}, INVAL, "null mask"), ({5: None}, INVAL, "null key"), ({1: -1}, INVAL, "B < 0"),
                 ({2: 0}, INVAL, "G < 1"), ({3: -1}, INVAL, "k < 0"), ({3: 50}, INVAL, "k > P"), ({4: -1}, INVAL, "sample0 < 0"),
                 ({4: (1 << 53) - 7}, INVAL, "sample0 + B > 2^53"), ({1: 0, 0: None}, INVAL, "null mask at B = 0"),
                 ({2: 33, 3: 5}, UNSUPP, "G > 32")]
_SHAPE_REFUSED = [({"B": -1}, INVAL, "B < 0"), ({"S": 0}, INVAL, "S <= 0"), ({"p": 0}, INVAL, "p <= 0"),
                  ({"p": 48}, INVAL, "S % p != 0"), ({"S": 264, "p": 8}, UNSUPP, "G > 32"),
                  ({"B": 14267}, UNSUPP, "3 B S^2 >= 2^31")]
_LOSS_REFUSED = [({"B": 0}, INVAL, "B = 0"), ({"delta": 0.0}, INVAL, "delta = 0"), ({"delta": -1.0}, INVAL, "delta < 0"),
                 ({"delta": float("inf")}, INVAL, "delta inf"), ({"delta": float("nan")}, INVAL, "delta NaN"),
                 ({"masked": 0}, INVAL, "masked = 0"), ({"masked": 8 * 49 + 1}, INVAL, "masked > B P")]


def _call(lib, name, base, where, change):
    a = list(base)
    for key, v in change.items():
        a[where[key] if isinstance(key, str) else key] = v
    return getattr(lib, name)(*a)


def test_entry_points_are_exported_declared_bound_and_refuse_bad_arguments():
    """Every call below is turned down by the argument checks (or has B == 0, which returns before any launch): no kernel
    runs and the fake addresses are never dereferenced."""
    import test_abi_cpu as abi
    from calm_vit_dte_amd import _lib as binding
    raw = open(HEADER).read()
    assert int(re.search(r"#define\s+CALM_ABI_VERSION\s+(\d+)", raw).group(1)) == binding.ABI_VERSION == 7   # additions only
    assert re.search(r"CALM_RED_MIM\s*=\s*11\b", raw) and binding.RED_MIM == 11
    for name in NEW:
        assert name in abi._declared() and hasattr(ctypes.CDLL(abi.LIB), name) and name in binding.SIGNATURES
    assert "mim.hip" in import_module("calm_vit_dte_amd.build").SOURCES
    lib = binding.load()
    code = {INVAL: binding.E_INVAL, UNSUPP: binding.E_UNSUPP, LAYOUT: binding.E_LAYOUT}
    assert int(lib.calm_reduce_scratch_floats(binding.RED_MIM, 256, 224)) == 2048
    assert int(lib.calm_reduce_scratch_floats(binding.RED_MIM, 1, 8)) == 2048
    for change, kind, what in _DRAW_REFUSED:
        assert _call(lib, "calm_mim_draw", _DRAW, {}, change) == code[kind], what
    assert _call(lib, "calm_mim_draw", _DRAW, {}, {1: 0}) == 0       # nothing to do
    for name, base, where, nulls, aligned in (
            ("calm_mim_apply", _APPLY, dict(B=4, S=5, p=6), (0, 1, 2, 3), (0, 1)),
            ("calm_mim_huber_fwd", _FWD, dict(delta=3, B=5, S=6, p=7, masked=8), (0, 1, 2, 4, 9), (0, 1)),
            ("calm_mim_huber_bwd", _BWD, dict(delta=3, B=6, S=7, p=8, masked=9), (0, 1, 2, 4, 5), (0, 1, 5))):
        for i in nulls:
            assert _call(lib, name, base, where, {i: None}) == code[INVAL], (name, "null argument", i)
        for i in aligned:
            assert _call(lib, name, base, where, {i: _P + 2}) == code[LAYOUT], (name, "not 4-byte aligned", i)
        refused = _SHAPE_REFUSED + (_LOSS_REFUSED if name != "calm_mim_apply" else [])
        for change, kind, what in refused:
            assert _call(lib, name, base, where, change) == code[kind], (name, what)
    assert _call(lib, "calm_mim_huber_fwd", _FWD, {}, {9: _P + 4}) == code[LAYOUT]          # partials off 16 bytes
    assert _call(lib, "calm_mim_apply", _APPLY, dict(B=4), {"B": 0}) == 0


def test_hip_backend_checks_key_and_mask_before_the_call():
    be = calm.backend.HipBackend.__new__(calm.backend.HipBackend)    # no library, no device: the checks come first
    mask = torch.zeros(2, 4, dtype=torch.uint8)
    for key in (None, torch.zeros(2, dtype=torch.int64), torch.zeros(2)):
        with pytest.raises(TypeError, match="mim_draw expects its key"):
            be.mim_draw(mask, 2, 2, 1, key)
    for bad in (mask, None):                                         # (a CPU mask; the shape is checked as well)
        with pytest.raises(TypeError, match=r"mim_apply expects its mask as a contiguous uint8 CUDA tensor \[B, P\] = \[2, 4\]"):
            be._mim_mask("mim_apply", bad, 2, 4)


def test_plain_emulated_backends_have_no_mask_kernel():
    """The kernels are not optional: a backend without the entry points fails, it does not train unmasked."""
    with calm.backend.use_backend(EmulatedBackend()), pytest.raises(AttributeError, match="mim_draw"):
        trainer.MaskedImageModelling(4).draw(2, 8, torch.device("cpu"))


# ---- ops.MimHuberFn ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,p", [(3, 8, 4), (2, 12, 3)])
def test_mim_huber_fn_matches_torch_autograd_on_the_twin(B, S, p):
    tokens, target = F.inputs(B, S)
    mask = F.masks(B, S, p)["uneven"]
    masked = int(mask.sum())
    be = E.EmulatedMimBackend()
    with calm.backend.use_backend(be):
        t = tokens.clone().requires_grad_(True)
        loss = calm.ops.MimHuberFn.apply(t, target, mask, 0.5, masked)
        (loss * 3.0).backward()
    assert be.mim_huber_calls == 1
    tr = tokens.clone().requires_grad_(True)
    ref = trainer.mim_huber_torch(tr, target, mask, p, 0.5)           # (counts the mask itself)
    (ref * 3.0).backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-6 * float(ref.detach()) and rel_err(t.grad, tr.grad) <= 1e-6
    m = torch.from_numpy(F.ref_element_mask(mask.numpy(), S, p))
    assert (t.grad[~m].view(torch.int32) == 0).all() and (tr.grad[~m].view(torch.int32) == 0).all()
    with calm.backend.use_backend(be), pytest.raises(ValueError, match="mask"):
        calm.ops.MimHuberFn.apply(tokens, target, mask[:, :-1], 1.0, masked)


# ---- MaskedImageModelling --------------------------------------------------------------------------------------------------------
def test_k_table_settings_and_refusals():
    M = trainer.MaskedImageModelling
    table = {(224, 32, 0.6): 29, (224, 16, 0.6): 118, (224, 7, 0.6): 614, (48, 8, 0.6): 22, (8, 4, 0.01): 1, (8, 4, 0.99): 3,
             (8, 4, 0.5): 2, (12, 3, 0.75): 12, (9, 3, 0.5): 5}
    for (S, p, ratio), k in table.items():
        G = S // p
        assert M(p, ratio).grid(S) == (G, G * G, k), (S, p, ratio)
    assert M().settings() == {"patch": 32, "ratio": 0.6, "fill": [0.0, 0.0, 0.0]}
    assert M(16, 0.5, (1, 2, 3)).settings() == {"patch": 16, "ratio": 0.5, "fill": [1.0, 2.0, 3.0]}
    assert M(**M(16, 0.5, 0.25).settings()).settings() == M(16, 0.5, 0.25).settings()
    with pytest.raises(ValueError, match="image side 50 is not a multiple of the patch side 32"):
        M().grid(50)
    with pytest.raises(ValueError, match="image side 264 holds 33 patches of side 8"):
        M(8).grid(264)
    for bad in (0.0, 1.0, -0.1, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="ratio is a share"):
            M(ratio=bad)
    for bad in (0, -4, 2.0, True):
        with pytest.raises(ValueError, match="patch is a side"):
            M(patch=bad)
    for bad in ((1, 2), float("inf"), "0", (0, 0, float("nan"))):
        with pytest.raises(ValueError, match="fill is a finite float"):
            M(fill=bad)


def test_draw_apply_and_loss_go_through_the_backend():
    mim = trainer.MaskedImageModelling(4, 0.5, (0.25, -0.5, 1.5))
    x, target = F.inputs(3, 8)
    be = E.EmulatedMimBackend()
    calm.ops.set_dropout_key_override(KeyStream(F.SEED))
    with calm.backend.use_backend(be):
        mask = mim.draw(3, 8, x.device)
        assert np.array_equal(mask.numpy(), F.ref_mask((F.SEED, 0), 0, 3, 2, 2))
        y = mim.apply(x, mask)
        assert torch.equal(y, F.ref_apply(x, mask.numpy(), mim.fill, 4))
        plain = mim.loss(x, target, mask)
        assert getattr(be, "mim_huber_calls", 0) == 0                # the loss kernels are off: the torch twin
        calm.backend.set_loss_kernels(True)
        fused = mim.loss(x, target, mask)
        assert be.mim_huber_calls == 1
    ref = F.ref_huber(x, target, mask.numpy(), 1.0, 1.0, 4, 6)[0]
    assert abs(float(plain) - float(ref)) <= F.TOL * float(ref) and abs(float(fused) - float(ref)) <= F.TOL * float(ref)


# ---- RegTrainStep(mim=) ----------------------------------------------------------------------------------------------------
def _rows(x):
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], x.shape[2], 3 * x.shape[3]).contiguous()


def _hand_forward(model, x, kl_weight, fill=(0.0, 0.0, 0.0)):
    """What a step with mim= computes, written out: the mask from the definition, the select, the twin's loss."""
    rows = _rows(x) if x.dim() == 4 else x
    B, S, _ = rows.shape
    G = S // PATCH
    k = F.ratio_k(G * G, MIM["ratio"])
    key = [int(v) for v in calm.ops.draw_dropout_key(x.device)]
    mask = F.ref_mask(key, 0, B, G, k)
    y_hat, kl = model(F.ref_apply(rows, mask, fill, PATCH))
    loss = trainer.mim_huber_torch(y_hat.reshape(rows.shape), rows, torch.from_numpy(mask), PATCH, 1.0, B * k) + kl * kl_weight
    return loss, y_hat.reshape(-1, S, S, 3).permute(0, 3, 1, 2)


@pytest.mark.parametrize("layout", ["image", "rows"])
def test_reg_train_step_with_mim_equals_the_hand_written_loop(layout):
    x = torch.randn(2, 3, 48, 48, generator=torch.Generator().manual_seed(4)) * 0.5
    x = _rows(x) if layout == "rows" else x
    runs = {}
    for kind in ("step", "hand", "kernels", "plain"):
        be = E.EmulatedMimBackend()
        with calm.backend.use_backend(be):
            calm.backend.set_loss_kernels(kind == "kernels")
            calm.ops.set_dropout_key_override(KeyStream(F.SEED))
            torch.manual_seed(8)
            m = build_model("nano48_gen", None).train()
            opt = trainer.make_optimizer(m)
            step = trainer.RegTrainStep(m, opt, mim=None if kind in ("hand", "plain") else
                                        (trainer.MaskedImageModelling(**MIM) if kind == "step" else MIM))
            losses = []
            for _ in range(2):
                torch.manual_seed(9)
                if kind == "hand":
                    loss, img = _hand_forward(m, x, step.kl_weight)
                    loss, img = step._finish(loss, img)
                else:
                    loss, img = step(x)
                assert tuple(img.shape) == (2, 3, 48, 48)
                losses.append(float(loss))
            assert getattr(be, "mim_draw_calls", 0) == (0 if kind in ("hand", "plain") else 2)
            assert getattr(be, "mim_huber_calls", 0) == (2 if kind == "kernels" else 0)
            runs[kind] = (losses, [p.detach().clone() for p in m.parameters()])
        calm.backend.set_loss_kernels(False)
    assert runs["step"][0] == runs["hand"][0]
    assert all(torch.equal(a, b) for a, b in zip(runs["step"][1], runs["hand"][1]))
    assert all(abs(a - b) <= 1e-5 * abs(b) for a, b in zip(runs["kernels"][0], runs["step"][0]))
    assert runs["plain"][0] != runs["step"][0]                        # the unmasked job is another job
    with pytest.raises(ValueError, match='mim takes the keys "patch", "ratio", "fill"'):
        trainer.RegTrainStep(m, opt, mim={"size": 8})


# ---- train(task="reg", mim=) -----------------------------------------------------------------------------------------------------
class _HandMim(trainer.RegTrainStep):
    """RegTrainStep that is told nothing about mim and masks itself."""

    def __init__(self, *args, mim=None, **kw):
        super().__init__(*args, **kw)

    def __call__(self, x, _y=None):
        return self._finish(*_hand_forward(self.model, x, self.kl_weight))


class _HandAccumMim(trainer.AccumTrainStep, _HandMim):
    def __init__(self, model, optimizer, reducer=None, accumulate=2, kl_weight=0.1, **kw):
        super().__init__(model, optimizer, reducer, accumulate=accumulate, kl_weight=kl_weight, **kw)


class _HandSamMim(trainer.SamTrainStep, _HandMim):
    def __init__(self, model, optimizer, reducer=None, sam=None, sync=False, kl_weight=0.1, **kw):
        super().__init__(model, optimizer, reducer, sam=sam, sync=sync, kl_weight=kl_weight, **kw)


_HAND = {("reg", False): _HandMim, ("reg", True): _HandAccumMim, ("reg", "sam"): _HandSamMim}


def _train(seed=50, n=8, epochs=1, hand=False, keys=True, mim=MIM, **kw):
    """train(task="reg") on nano48_gen with the emulated backend: 4 batches of 2 per epoch (and rank); hand: the step classes
    are the ones above and train() is not told about mim; keys: injected (KeyStream), else torch's generator."""
    torch.manual_seed(seed)
    m = build_model("nano48_gen", None).train()
    real = dict(trainer._STEP_CLASSES)
    if hand:
        trainer._STEP_CLASSES.update(_HAND)
    calm.ops.set_dropout_key_override(KeyStream(F.SEED) if keys else None)
    try:
        with calm.backend.use_backend(E.EmulatedMimBackend()):
            return trainer.train(m, "fused", None, use_gpu=False, dataset=_GenSet(n), epochs=epochs, batch_size=2,
                                 num_workers=0, log_every=1000, task="reg", mim=None if hand else mim, **kw)
    finally:
        trainer._STEP_CLASSES.update(real)
        calm.ops.set_dropout_key_override(None)


def _same_bits(a, b, what):
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{what}: differs at {k}"


def _differ(a, b):
    return any(not torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kw", [{}, dict(accumulate=2), dict(sam=0.05)], ids=["plain", "accumulate", "sam"])
def test_train_with_mim_equals_the_steps_that_mask_themselves(kw, capsys):
    out = _train(**kw)
    assert "mim: patch 8, ratio 0.6000, fill [0.0, 0.0, 0.0]" in capsys.readouterr().out
    _same_bits(out, _train(hand=True, **kw), f"train(mim=, {kw}) against the steps that mask themselves")
    assert all(bool(torch.isfinite(p).all()) for p in out.parameters())
    if not kw:
        assert _differ(out, _train(mim=None))
        _same_bits(out, _train(mim=trainer.MaskedImageModelling(**MIM)), "the object form")
        assert _differ(out, _train(mim={"patch": 8, "ratio": 0.6, "fill": 0.5}))


@pytest.mark.timeout(600)
def test_snapshot_header_refusals_and_exact_resume(tmp_path):
    fa, fb, fc, fd = (str(tmp_path / f"{n}.snap") for n in "abcd")
    kw = dict(epochs=2, keys=False, ema=0.9)                          # the keys come from the RNG state a snapshot holds
    a = _train(snapshot_path=fa, **kw)
    _train(snapshot_path=fb, max_steps=2, **kw)
    head = trainer.TrainState.read_header(fb)[0]["host"]
    assert head["progress"]["step"] == 2 and head["mim"] == {"patch": 8, "ratio": 0.6, "fill": [0.0, 0.0, 0.0]}
    c = _train(seed=51, snapshot_path=fc, resume=fb, **kw)
    _same_bits(a, c, "the resumed run")
    with pytest.raises(ValueError, match=r"written with mim patch 8, ratio 0.6, fill \[0.0, 0.0, 0.0\], this step trains without mim"):
        _train(snapshot_path=fc, resume=fb, **{**kw, "mim": None})
    with pytest.raises(ValueError, match="written with mim patch 8, ratio 0.6, .* this step trains with mim patch 8, ratio 0.5"):
        _train(snapshot_path=fc, resume=fb, **{**kw, "mim": {"patch": 8, "ratio": 0.5}})
    _train(snapshot_path=fd, max_steps=2, **{**kw, "mim": None})
    assert "mim" not in trainer.TrainState.read_header(fd)[0]["host"]  # older snapshots load as before
    with pytest.raises(ValueError, match="written without mim, this step trains with mim patch 8"):
        _train(snapshot_path=fc, resume=fd, **kw)


def test_train_refusals_come_before_any_process_group():
    data = torch.utils.data.TensorDataset(torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,)))
    lin = torch.nn.Linear(4, 4)
    kw = dict(use_gpu=False, dataset=data, epochs=1, batch_size=2, num_classes=10)
    with pytest.raises(ValueError, match='mim= needs task="reg"'):
        trainer.train(lin, "fused", mim=True, **kw)
    for bad in (1.0, 0.0, -0.1, float("nan"), {"ratio": 1.5}):
        with pytest.raises(ValueError, match="ratio is a share of the patches"):
            trainer.train(lin, "fused", task="reg", mim=bad, **kw)
    for bad in ({"ratio": 0.5, "size": 8}, {"patches": 4}):
        with pytest.raises(ValueError, match='mim takes the keys "patch", "ratio", "fill"'):
            trainer.train(lin, "fused", task="reg", mim=bad, **kw)
    with pytest.raises(ValueError, match="patch is a side in pixels"):
        trainer.train(lin, "fused", task="reg", mim={"patch": 0}, **kw)
    for bad in ("0.5", [0.5]):
        with pytest.raises(ValueError, match="mim is None, True, a ratio or a dict"):
            trainer.train(lin, "fused", task="reg", mim=bad, **kw)
    assert not torch.distributed.is_initialized()


# ---- two gloo ranks ------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _two_rank_worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    run = _train(n=16, destroy_process_group=False)
    hand = _train(n=16, hand=True, destroy_process_group=False)
    torch.save(dict(run=run.state_dict(), hand=hand.state_dict()), os.path.join(outdir, f"rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_train_with_mim_on_two_gloo_ranks(tmp_path):
    mp.spawn(_two_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(2))
    for k in r0["run"]:
        assert torch.equal(r0["run"][k], r0["hand"][k]), f"train(mim=) differs from the steps that mask themselves at {k}"
        assert torch.equal(r0["run"][k], r1["run"][k]), f"the ranks diverged at {k}"


# ---- load_backbone -----------------------------------------------------------------------------------------------------------
def test_load_backbone_hands_the_pretrained_autoencoder_to_a_classifier(tmp_path):
    torch.manual_seed(1)
    gen = build_model("nano48_gen", None)
    torch.manual_seed(2)
    cls = build_model("nano48_cls", None)
    before = {k: v.clone() for k, v in cls.state_dict().items()}
    src = {k: v * 0.5 - 0.25 if v.is_floating_point() else v for k, v in gen.state_dict().items()}   # "pre-trained"
    under = [k for k in before if k.startswith("autoencoder.")]
    assert under and any(not torch.equal(before[k], src[k]) for k in under) and any(k.endswith("weight_u") for k in under)
    rep = trainer.load_backbone(cls, src)
    after = cls.state_dict()
    assert rep["loaded"] == under and set(rep["ignored"]) == {k for k in src if not k.startswith("autoencoder.")}
    assert all(torch.equal(after[k], src[k]) for k in under)                     # bit-equal under the prefix
    assert all(torch.equal(after[k], before[k]) for k in before if k not in under)   # the head is untouched
    path = str(tmp_path / "model_reg_ema.pth")                                   # the path form
    torch.save({k: v + 1.0 if v.is_floating_point() else v for k, v in src.items()}, path)
    trainer.load_backbone(cls, path)
    assert all(torch.equal(cls.state_dict()[k], src[k] + 1.0) for k in under if src[k].is_floating_point())
    held = {k: v.clone() for k, v in cls.state_dict().items()}
    bad = dict(src)
    first = under[0]
    bad[first] = torch.zeros(3, 5, 7)
    del bad[under[1]]
    bad["autoencoder.extra"] = torch.zeros(1)
    with pytest.raises(ValueError, match=r"3 mismatch\(es\) under 'autoencoder.'.*missing in the source.*not in the model.*in the source,"):
        trainer.load_backbone(cls, bad)
    assert all(torch.equal(cls.state_dict()[k], held[k]) for k in held)          # nothing was copied
    with pytest.raises(ValueError, match="no key of the model starts with"):
        trainer.load_backbone(cls, src, prefix="backbone.")
    with pytest.raises(ValueError, match="state dict or the path of one"):
        trainer.load_backbone(cls, [1, 2])
