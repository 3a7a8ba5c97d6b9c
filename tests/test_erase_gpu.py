"""calm_augment_collate_erase (csrc/augment.hip, the ERASE instantiations) against the float64 emulation of
tests/emulated_erase.py, and train(random_erasing=).

Tolerance: absolute 2e-5 on the output, the bound of tests/test_augment_gpu.py, whose derivation covers the un-erased
pixels; pixels near the solarize threshold are left out as there (tests/test_erase_cpu.py caps their share).  For noise
pixels the fp32 error is dominated by the rounding of the argument 2 pi u of the sine and cosine, <= 2 pi 2^-24 2, times
r <= 5.77: about 4e-6 (an fp32 numpy evaluation of the formula against float64 over 2 M draws gave 1.7e-6); 2e-5 leaves
about 5x over that.  A constant fill is exact.  Shapes, boxes and the CutMix boxes are emulated_erase's: a 19 x 70 window
(ragged 16 x 64 tiles both ways, scalar stores) and a 32 x 64 one (16-byte stores), B = 3, both layouts; every output is
pre-filled with NaN."""
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import emulated_erase as EE
from test_host_logic_cpu import build_model

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")

MEAN, STD = trainer.DeviceCollate.MEAN, trainer.DeviceCollate.STD
TOL, GM_RTOL = 2e-5, 1e-6


def run_kernel(src, t, boxes, value, key, H, W, mode=0, lam=1.0, box=None, tokens=False, misalign=False):
    """The erase entry point (boxes None: calm_augment_collate) into a NaN-filled output; misalign: `out` starts one float
    behind a 16-byte boundary."""
    B = src.shape[0]
    shape = (B, H, 3 * W) if tokens else (B, 3, H, W)
    if misalign:
        out = torch.full((B * 3 * H * W + 1,), float("nan"), device="cuda")[1:].view(shape)
        assert out.data_ptr() % 16 == 4
    else:
        out = torch.full(shape, float("nan"), device="cuda")
    gm = torch.full((B,), float("nan"), device="cuda")
    samples = trainer.DeviceAugment.pack(t, device="cuda")
    be, img = calm.backend.get_backend(), torch.from_numpy(src.copy()).cuda()       # (the shared source is read-only)
    if boxes is None:
        be.augment_collate(img, samples, gm, out, mode, lam, box, MEAN, STD, tokens=tokens)
    else:
        be.augment_collate_erase(img, samples, gm, out, mode, lam, box, MEAN, STD, trainer.DeviceErase.pack(boxes, device="cuda"),
                                 value, key, tokens=tokens)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(gm).all()       # every element written
    return out, gm


def run_case(shape, boxset, noise_fill, mode, tokens, lam=None, box="case", misalign=False):
    src, t, H, W = EE.case_inputs(shape)
    boxes = EE.case_samples(shape, boxset, noise_fill)[4]
    m, case_lam = EE.MODES[mode]
    return run_kernel(src, t, boxes, None if noise_fill else EE.VALUE, EE.KEY, H, W, m, case_lam if lam is None else lam,
                      (EE.CUTMIX[shape] if box == "case" else box) if m == 2 else None, tokens, misalign)


def bits(t):
    return t.contiguous().view(torch.int32)


def to_tokens(image):
    B, _, H, W = image.shape
    return image.permute(0, 2, 3, 1).reshape(B, H, 3 * W)


# ---- 1. against the emulation --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("case", EE.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{'noise' if c[2] else 'const'}")
def test_against_the_emulation(case, mode, tokens):
    shape, boxset, noise_fill = case
    ref, ref_gm, near = EE.case_reference(shape, boxset, noise_fill, mode, tokens)
    out, gm = run_case(shape, boxset, noise_fill, mode, tokens)
    out, gm = out.cpu().numpy().astype(np.float64), gm.cpu().numpy().astype(np.float64)
    d = np.abs(out - ref)[~near].max()
    dg = (np.abs(gm - ref_gm) / np.where(ref_gm == 0, 1.0, np.abs(ref_gm))).max()
    print(f"{case} mode {mode} tokens {tokens}: max |kernel - float64| = {d:.3e} (bound {TOL:.0e}), gray_mean rel {dg:.3e}, "
          f"excluded {near.mean():.4%}")
    assert d <= TOL, (case, mode, tokens, d)
    assert dg <= GM_RTOL
    if mode == 0 and not noise_fill:                      # a constant-erased pixel is the float32 of the value, exactly
        erased = np.repeat(EE.case_samples(shape, boxset, noise_fill)[3][:, None], 3, axis=1)
        want = np.broadcast_to(np.asarray(EE.VALUE, dtype=np.float32).astype(np.float64)[None, :, None, None], erased.shape)
        if tokens:
            B, _, H, W = erased.shape
            erased, want = (a.transpose(0, 2, 3, 1).reshape(B, H, 3 * W) for a in (erased, want))
        assert erased.any() and np.array_equal(out[erased], want[erased])


# ---- 2. the partner's erasure is the partner's own -------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("case", EE.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{'noise' if c[2] else 'const'}")
def test_the_partner_is_erased_with_its_own_box_and_its_own_noise(case, tokens):
    """MixUp with lam = 0 and CutMix over the whole window hand sample b the partner's erased image: bit for bit the
    mode-0 output of sample (b - 1) mod B — its box, and noise keyed by ITS sample index, not by the reader's."""
    H, W = EE.case_inputs(case[0])[2:]
    plain, _ = run_case(*case, 0, tokens)
    want = bits(plain.roll(1, 0))
    mixup, _ = run_case(*case, 1, tokens, lam=0.0)
    assert torch.equal(bits(mixup), want)
    cutmix, _ = run_case(*case, 2, tokens, box=(0, H, 0, W))
    assert torch.equal(bits(cutmix), want)


# ---- 3. layout and store path do not change a value -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("case", [c for c in EE.CASES if c[2]], ids=lambda c: f"{c[0]}-{c[1]}")
def test_layout_and_store_path_do_not_change_a_value(case, mode):
    image, gm = run_case(*case, mode, False)
    tokens, gm_t = run_case(*case, mode, True)
    assert torch.equal(bits(tokens), bits(to_tokens(image))) and torch.equal(bits(gm), bits(gm_t))
    for tok, aligned in ((False, image), (True, tokens)):  # one float off a 16-byte boundary: the scalar stores
        off, _ = run_case(*case, mode, tok, misalign=True)
        assert torch.equal(bits(off), bits(aligned))


# ---- 4. a table without boxes is calm_augment_collate ---------------------------------------------------------------------
@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", list(EE.SHAPES))
def test_a_table_without_boxes_equals_augment_collate(shape, mode, tokens):
    src, t, H, W = EE.case_inputs(shape)
    m, lam = EE.MODES[mode]
    box = EE.CUTMIX[shape] if m == 2 else None
    plain, gm_plain = run_kernel(src, t, None, None, None, H, W, m, lam, box, tokens)
    for value in (None, EE.VALUE):
        out, gm = run_kernel(src, t, trainer.DeviceErase.identity(EE.B), value, EE.KEY, H, W, m, lam, box, tokens)
        assert torch.equal(out, plain) and torch.equal(gm, gm_plain)


# ---- 5. the noise ----------------------------------------------------------------------------------------------------------
def test_noise_is_standard_normal_keyed_and_uncorrelated_across_channels():
    """A 64 x 64 box in a 65 x 65 window on sample 1 of 2: 3 x 4096 normals."""
    src = EE.source(80, 2, 65, 65)
    t = trainer.DeviceAugment.identity(2)
    boxes = EE.boxes_of([(0, 0, 0, 0), (1, 0, 64, 64)])

    def erased(key):
        out, _ = run_kernel(src, t, boxes, None, key, 65, 65)
        return out[1, :, 1:65, 0:64]

    a = erased(EE.KEY)
    x = a.double().reshape(3, -1).cpu().numpy()
    n = x.size
    assert n == 12288 and np.abs(x).max() <= 5.78
    mean, var = x.mean(), x.var()
    corr = np.corrcoef(x)
    print(f"noise: mean {mean:.4f}, variance {var:.4f}, channel correlations {corr[0, 1]:.4f} {corr[0, 2]:.4f} {corr[1, 2]:.4f}")
    assert abs(mean) <= 5.0 / np.sqrt(n) and abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert max(abs(corr[0, 1]), abs(corr[0, 2]), abs(corr[1, 2])) <= 5.0 / np.sqrt(n)
    ref = EE.noise(EE.KEY, 1, 65, 65)[:, 1:65, 0:64]
    assert np.abs(a.cpu().numpy().astype(np.float64) - ref).max() <= TOL
    assert torch.equal(bits(erased(EE.KEY)), bits(a))                    # the same key: the same noise
    other = erased((EE.KEY[0], EE.KEY[1] + 1))
    assert (other != a).float().mean().item() > 0.99                    # another offset: another fill


# ---- 6. train(random_erasing=) ------------------------------------------------------------------------------------------------
class _U8Set(torch.utils.data.Dataset):
    def __init__(self, n=12):
        g = torch.Generator().manual_seed(11)
        self.x = torch.randint(0, 256, (n, 3, 38, 38), generator=g, dtype=torch.uint8)
        self.y = torch.randint(0, 10, (n,), generator=g)

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return self.x[i], int(self.y[i])


def _train(**kw):
    torch.manual_seed(50)
    m = build_model("tiny32_cls", None).train()
    return trainer.train(m, "fused", scheduler=False, use_gpu=True, dataset=_U8Set(), epochs=2, batch_size=4, num_classes=10,
                         device_collate=True, device_augment=True, crop=(32, 32), log_every=1000, **kw)


def _same(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.mark.timeout(600)
def test_train_with_random_erasing_and_exact_resume(tmp_path):
    """2 epochs of 3 batches.  p = 0 draws no box: the run without the argument, bit for bit; p = 1 is another run; a
    run snapshotted behind step 2 and resumed equals the uninterrupted one, the erase generator being in the snapshot."""
    plain = _train()
    assert _same(_train(random_erasing=0.0), plain)
    fa, fb = str(tmp_path / "a.snap"), str(tmp_path / "b.snap")
    full = _train(random_erasing=1.0, snapshot_path=fa)
    assert not _same(full, plain)
    assert all(torch.isfinite(v.float()).all() for v in full.state_dict().values())
    _train(random_erasing=1.0, snapshot_path=fb, max_steps=2)
    assert trainer.TrainState.read_header(fb)[0]["host"]["progress"] == {"epoch": 0, "batch": 2, "step": 2}
    resumed = _train(random_erasing=1.0, snapshot_path=fb, resume=fb)
    assert _same(resumed, full)
    assert os.path.exists(fa) and not torch.distributed.is_initialized()
