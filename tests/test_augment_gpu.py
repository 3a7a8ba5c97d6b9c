"""calm_augment_collate (csrc/augment.hip) against the float64 emulation of tests/emulated_augment.py.

Tolerance: absolute 2e-5 on the normalised output.  The pointwise chain is a few dozen fp32 operations on values in
[0, 1] (an fp32 and an fp64 run of a four-operation chain differ by about 2e-7), the blur is a convex combination and
Normalize multiplies by at most 1 / 0.224 = 4.5: the bound leaves about 20x over that.  A solarize comparison can fall on
either side when a pre-solarize value is within 1e-5 of the threshold; the emulation marks the output pixels such a value
contributes to (through the blur's 3x3 neighbourhood, own and partner sample), they are left out of the comparison, and a
case in which they are more than 0.5 % of the output fails.  gray_mean (the contrast means): 1e-6 relative.
Sources are seeded random uint8 images; every case writes into an output pre-filled with NaN."""
import itertools
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import emulated_augment as EA
from helpers import CONFIGS, load_golden
from test_host_logic_cpu import build_model

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")

MEAN, STD = trainer.DeviceCollate.MEAN, trainer.DeviceCollate.STD
TOL, GM_RTOL, MAX_NEAR = 2e-5, 1e-6, 0.005
THR = np.float32(223.5 / 255.0)


def source(seed, B, Hs, Ws):
    return np.random.default_rng(seed).integers(0, 256, (B, 3, Hs, Ws), dtype=np.uint8)


def table(B, corners):
    t = trainer.DeviceAugment.identity(B)
    t["y0"], t["x0"] = np.asarray(corners)[:, 0], np.asarray(corners)[:, 1]
    t["solarize_thr"] = THR
    return t


def varied_table(seed, B, Hs, Ws, H, W, orders=None):
    """Every sample with its own factors, corner and flags; orders: one per sample, or random permutations."""
    rng = np.random.default_rng(seed)
    t = table(B, np.stack([rng.integers(0, Hs - H + 1, B), rng.integers(0, Ws - W + 1, B)], axis=1))
    t["order"] = orders if orders is not None else rng.permuted(np.tile(np.arange(4, dtype=np.uint8), (B, 1)), axis=1)
    for name in ("brightness", "contrast", "saturation"):
        t[name] = rng.uniform(0.5, 1.0, B)
    t["hue"] = rng.uniform(-0.125, 0.125, B)
    t["blur_sigma"] = rng.uniform(0.1, 2.0, B)
    b = np.arange(B)
    t["flags"] = (binding.AUG_BLUR | np.where(b % 2 == 1, binding.AUG_SOLARIZE, 0) | np.where(b % 3 == 0, binding.AUG_FLIP, 0)
                  | np.where(b % 5 == 2, binding.AUG_GRAYSCALE, 0)).astype(np.uint32)
    return t


def run_kernel(src, t, H, W, mode=0, lam=1.0, box=None, tokens=False):
    B = src.shape[0]
    out = torch.full((B, H, 3 * W) if tokens else (B, 3, H, W), float("nan"), device="cuda")
    gm = torch.full((B,), float("nan"), device="cuda")
    samples = trainer.DeviceAugment.pack(t, device="cuda")
    calm.backend.get_backend().augment_collate(torch.from_numpy(src).cuda(), samples, gm, out, mode, lam, box, MEAN, STD,
                                               tokens=tokens)
    torch.cuda.synchronize()
    return out, gm


def reference(src, t, H, W, mode=0, lam=1.0, box=None, tokens=False):
    ref, gm, near = EA.augment_collate(src, t, H, W, mode, lam, box, MEAN, STD, tokens=tokens)
    assert near.mean() <= MAX_NEAR, f"{near.mean():.4%} of the output is near the solarize threshold"
    return ref, gm, near


def compare(what, src, t, H, W, mode=0, lam=1.0, box=None, tokens=False):
    ref, ref_gm, near = reference(src, t, H, W, mode, lam, box, tokens)
    out, gm = run_kernel(src, t, H, W, mode, lam, box, tokens)
    out, gm = out.cpu().numpy().astype(np.float64), gm.cpu().numpy().astype(np.float64)
    assert np.isfinite(out).all() and np.isfinite(gm).all()              # every element written
    d = np.abs(out - ref)[~near].max()
    dg = (np.abs(gm - ref_gm) / np.where(ref_gm == 0, 1.0, np.abs(ref_gm))).max()
    print(f"{what}: max |kernel - float64| = {d:.3e} (bound {TOL:.0e}), gray_mean rel {dg:.3e}, excluded {near.mean():.4%}")
    assert d <= TOL, (what, d)
    assert dg <= GM_RTOL and (gm[ref_gm == 0] == 0).all(), (what, dg)


# ---- 1. each operation alone ------------------------------------------------------------------------------------------
def _jitter_only(op, name, factors):
    def fill(t):
        t["order"][:, 0] = op
        t[name] = factors
    return fill


def _flag_only(flag, **fields):
    def fill(t):
        t["flags"] = flag
        for k, v in fields.items():
            t[k] = v
    return fill


SINGLE = {
    "brightness": _jitter_only(binding.AUG_OP_BRIGHTNESS, "brightness", [0.5, 0.73, 1.0]),
    "contrast": _jitter_only(binding.AUG_OP_CONTRAST, "contrast", [0.5, 0.61, 0.97]),
    "saturation": _jitter_only(binding.AUG_OP_SATURATION, "saturation", [0.5, 0.82, 1.0]),
    "hue_plus": _jitter_only(binding.AUG_OP_HUE, "hue", [0.125, 0.04, 0.09]),
    "hue_minus": _jitter_only(binding.AUG_OP_HUE, "hue", [-0.125, -0.01, -0.07]),
    "solarize": _flag_only(binding.AUG_SOLARIZE),
    "grayscale": _flag_only(binding.AUG_GRAYSCALE),
    "blur_0.1": _flag_only(binding.AUG_BLUR, blur_sigma=0.1),
    "blur_0.8": _flag_only(binding.AUG_BLUR, blur_sigma=0.8),
    "blur_2.0": _flag_only(binding.AUG_BLUR, blur_sigma=2.0),
}


def single_case(name):
    src = source(10, 3, 37, 45)
    t = table(3, [(0, 0), (8, 12), (3, 5)])
    SINGLE[name](t)
    return src, t, 29, 33


@pytest.mark.parametrize("name", list(SINGLE))
def test_each_operation_alone(name):
    compare(name, *single_case(name))


# ---- 2. all 24 jitter orders ------------------------------------------------------------------------------------------
ORDERS = np.array(list(itertools.permutations(range(4))), dtype=np.uint8)
ORDER_SHAPES = {"image_29x33": (37, 45, 29, 33, False), "tokens_32x32": (40, 36, 32, 32, True), "image_32x32": (40, 36, 32, 32, False)}


def orders_case(name):
    Hs, Ws, H, W, tokens = ORDER_SHAPES[name]
    return source(20, 24, Hs, Ws), varied_table(21, 24, Hs, Ws, H, W, orders=ORDERS), H, W, 0, 1.0, None, tokens


@pytest.mark.parametrize("name", list(ORDER_SHAPES))
def test_all_24_jitter_orders(name):
    """One permutation per sample, random factors, flags varied across the samples, blur on; the 32-wide crops take the
    16-byte stores, the 33-wide one the scalar stores."""
    compare(name, *orders_case(name))


# ---- 3. the partner ---------------------------------------------------------------------------------------------------
BOX = (10, 50, 60, 69)               # rows 10..49, columns 60..68 of a 70 x 70 crop: crosses the 16-row and 64-column tile edges


def partner_case(mode, B, tokens):
    return (source(30 + B, B, 80, 80), varied_table(31 + B, B, 80, 80, 70, 70), 70, 70, mode, 0.3 if mode == 1 else 1.0,
            BOX if mode == 2 else None, tokens)


@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_partner_goes_through_its_own_augmentation(mode, B, tokens):
    """MixUp / CutMix with the partner (b - 1) mod B — itself at B = 1 — augmented with its own parameters, corner, flip
    and contrast mean; the CutMix box crosses tile boundaries both ways."""
    compare(f"mode {mode} B {B} tokens {tokens}", *partner_case(mode, B, tokens))


# ---- 4. the window is reflected, not the source -------------------------------------------------------------------------
def window_case():
    src = source(40, 4, 37, 45)
    t = table(4, [(8, 12), (0, 0), (8, 0), (0, 12)])
    t["flags"] = [binding.AUG_BLUR, binding.AUG_BLUR, binding.AUG_BLUR | binding.AUG_FLIP, binding.AUG_BLUR | binding.AUG_FLIP]
    t["blur_sigma"] = [2.0, 1.5, 1.0, 2.0]
    return src, t, 29, 33


def test_blur_reflects_at_the_window_edge_not_the_source():
    """Corners at the maximum and at (0, 0): the random source pixels just outside the window differ from the reflected
    ones, so a kernel that reads past the window's edge (or clamps at it) is off by far more than the bound."""
    src, t, H, W = window_case()
    compare("window", src, t, H, W)
    wrong = src.copy()                                        # the emulation on a source whose outside differs: same result
    inside = np.zeros(src.shape, dtype=bool)
    for b in range(4):
        inside[b, :, t["y0"][b]:t["y0"][b] + H, t["x0"][b]:t["x0"][b] + W] = True
    wrong[~inside] ^= 0xFF
    assert np.array_equal(EA.augment_collate(wrong, t, H, W, 0, 1.0, None, MEAN, STD)[0],
                          EA.augment_collate(src, t, H, W, 0, 1.0, None, MEAN, STD)[0])


# ---- 5. identity table = the plain collate ----------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", [(37, 45, 29, 33), (40, 36, 32, 32)])
def test_identity_table_equals_collate_crop_mix(shape, mode, tokens):
    """No operation, no flag except the flips: both kernels are within one rounding of (u / 255 - mean) / std, of
    magnitude at most 2.7 — 1e-6 absolute."""
    Hs, Ws, H, W = shape
    B = 5
    src = torch.from_numpy(source(50, B, Hs, Ws)).cuda()
    rng = np.random.default_rng(51)
    corners = np.stack([rng.integers(0, Hs - H + 1, B), rng.integers(0, Ws - W + 1, B)], axis=1).astype(np.int32)
    flips = torch.tensor([1, 0, 0, 1, 1], dtype=torch.uint8)
    box = (3, 20, 5, 31) if mode == 2 else None
    be = calm.backend.get_backend()
    plain = torch.full((B, H, 3 * W) if tokens else (B, 3, H, W), float("nan"), device="cuda")
    be.collate_crop_mix(src, torch.from_numpy(corners).cuda(), flips.cuda(), plain, mode, 0.35, box, MEAN, STD, tokens=tokens)
    out, gm = torch.full_like(plain, float("nan")), torch.full((B,), float("nan"), device="cuda")
    samples = trainer.DeviceAugment.pack(trainer.DeviceAugment.identity(B), corners, flips, device="cuda")
    be.augment_collate(src, samples, gm, out, mode, 0.35, box, MEAN, STD, tokens=tokens)
    d = (out - plain).abs().max().item()
    print(f"identity {shape} mode {mode} tokens {tokens}: max |augment - plain| = {d:.3e}")
    assert d <= 1e-6 and plain.abs().max().item() <= 2.7
    assert (gm == 0).all()


# ---- 6. repeatability -------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical():
    src, t, H, W, *_ = orders_case("image_29x33")
    a, ga = run_kernel(src, t, H, W, 1, 0.3)
    b, gb = run_kernel(src, t, H, W, 1, 0.3)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ga.view(torch.int32), gb.view(torch.int32))
    assert (ga != 0).all()


# ---- 7. through DeviceCollate and the launcher --------------------------------------------------------------------------
def test_device_collate_routes_an_augment_object_to_the_kernel():
    src = source(60, 6, 40, 36)
    u8 = torch.from_numpy(src).cuda()
    labels = torch.arange(6, device="cuda")
    col, aug = trainer.DeviceCollate(num_classes=10, seed=5), trainer.DeviceAugment(seed=6)
    tab = aug.draw(6)
    dec = col.draw(6, 32, 32)
    out, y = col(u8, labels, decisions=dec, crop=(32, 32), tokens=True, aug_table=tab)
    t = tab.copy()
    corners = col.last_corners.cpu().numpy()
    t["y0"], t["x0"] = corners[:, 0], corners[:, 1]
    t["flags"] |= np.where(dec[3].numpy() != 0, binding.AUG_FLIP, 0).astype(np.uint32)
    ref, ref_gm, near = reference(src, t, 32, 32, dec[0], dec[1], dec[2], True)
    d = np.abs(out.cpu().numpy().astype(np.float64) - ref)[~near].max()
    print(f"DeviceCollate(aug_table): max |kernel - float64| = {d:.3e}")
    assert d <= TOL and tuple(y.shape) == (6, 10)
    assert np.abs(col.last_gray_mean.cpu().numpy() - ref_gm).max() <= GM_RTOL
    out2, _ = col(u8, labels, crop=(32, 32), tokens=True, augment=aug)       # drawn parameters: runs, finite
    assert torch.isfinite(out2).all()


def test_train_launcher_with_device_augment(capsys):
    """trainer.train(device_collate=True, device_augment=True): uint8 images -> H2D -> the augmenting collate -> the
    model's first Block; two steps on the nano configuration end with a finite loss."""
    name = "nano48_cls"
    g = load_golden(name)
    cfg = CONFIGS[name]
    S = cfg.seq_length
    gen = torch.Generator().manual_seed(0)
    data = torch.utils.data.TensorDataset(torch.randint(0, 256, (8, 3, S + 6, S + 6), generator=gen, dtype=torch.uint8),
                                          torch.randint(0, cfg.out_features, (8,), generator=gen))
    m = build_model(name, g, "cpu")
    out = trainer.train(m, "fused", scheduler=False, use_gpu=True, dataset=data, epochs=1, batch_size=4,
                        num_classes=cfg.out_features, device_collate=True, device_augment=True, crop=(S, S), max_steps=2,
                        log_every=1)
    losses = [float(v) for v in re.findall(r"Loss: ([^,]+),", capsys.readouterr().out)]
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    assert all(torch.isfinite(v.float()).all() for v in out.state_dict().values())
