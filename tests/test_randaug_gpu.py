"""calm_randaugment_u8 (csrc/randaugment.hip) against the numpy emulation of tests/emulated_randaug.py, which
tests/test_randaug_cpu.py holds against PIL: every comparison is exact equality of bytes.

Shapes: windows 1 x 1, 3 x 3 and 17 x 33 from a 20 x 40 source (byte stores, ragged groups of four pixels, the copy-only
branches of the 3 x 3 smooth) and 64 x 48 from 70 x 60 (dword stores, more than one workgroup per sample: 768 groups of
four against 1024 per workgroup is one, so the 224 x 224 case covers several — 13 — and several statistics chunks), B = 5
with mixed corners and flips."""
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import emulated_randaug as R

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
DRA = trainer.DeviceRandAugment

CASES = {"1x1": (20, 40, 1, 1), "3x3": (20, 40, 3, 3), "17x33": (20, 40, 17, 33), "64x48": (70, 60, 64, 48)}     # Hs, Ws, H, W
B = 5


def corners_flips(seed, n, Hs, Ws, H, W):
    rng = np.random.default_rng(seed)
    c = np.stack([rng.integers(0, Hs - H + 1, n), rng.integers(0, Ws - W + 1, n)], axis=1)
    c[0] = (Hs - H, Ws - W)                                # the last window of the source
    return c, (np.arange(n) % 2 == 1)


def run_kernel(src, table, H, W, fill=R.FILL, plan=None, misalign=False):
    """The entry point into an output pre-filled with 0x5A; plan: (n_slots, stats_mask) given instead of derived."""
    n = src.shape[0]
    if misalign:
        out = torch.full((n * 3 * H * W + 1,), 0x5A, dtype=torch.uint8, device="cuda")[1:].view(n, 3, H, W)
        assert out.data_ptr() % 4 == 1
    else:
        out = torch.full((n, 3, H, W), 0x5A, dtype=torch.uint8, device="cuda")
    n_slots, mask = plan if plan is not None else DRA.launch_plan(table)
    img = torch.from_numpy(np.array(src)).cuda()
    calm.backend.get_backend().randaugment_u8(img, DRA.pack(table, device="cuda"), out, n_slots, mask, fill=fill)
    torch.cuda.synchronize()
    return out


def assert_bytes(out, ref, what):
    got = out.cpu().numpy()
    diff = int((got != ref).sum())
    print(f"{what}: {diff} differing bytes of {ref.size}")
    assert got.tobytes() == ref.tobytes() and torch.equal(out.cpu(), torch.from_numpy(ref)), (what, diff)


# ---- 1. every operation alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_every_operation_alone(case):
    Hs, Ws, H, W = CASES[case]
    src = R.batch(100, B, Hs, Ws, "ramp" if case == "64x48" else "noise")
    corners, flips = corners_flips(5, B, Hs, Ws, H, W)
    for name, slot in R.every_op(H, W).items():
        t = R.table_of([[slot]] * B, corners, flips)
        assert_bytes(run_kernel(src, t, H, W), R.randaugment(src, t, H, W, R.FILL), f"{case} {name}")


# ---- 2. different chains per sample ---------------------------------------------------------------------------------------
def mixed_chains(H, W):
    ops = R.every_op(H, W)
    return [[],
            [ops["rotate+"], ops["equalize"], ops["sharpness+"], ops["contrast-"]],
            [ops["autocontrast"]],
            [ops["color+"], ops["shear_x-"], ops["posterize4"], ops["autocontrast"]],
            [ops["contrast+"], ops["solarize"], ops["translate_y+"]]]


@pytest.mark.parametrize("case", ["17x33", "64x48"])
def test_per_sample_chains_with_none_next_to_four(case):
    Hs, Ws, H, W = CASES[case]
    src = R.batch(200, B, Hs, Ws, "ramp")
    corners, flips = corners_flips(6, B, Hs, Ws, H, W)
    t = R.table_of(mixed_chains(H, W), corners, flips)
    assert DRA.launch_plan(t) == (4, 0b1011)
    ref = R.randaugment(src, t, H, W, R.FILL)
    assert_bytes(run_kernel(src, t, H, W), ref, f"{case} mixed")
    assert_bytes(run_kernel(src, t, H, W, misalign=True), ref, f"{case} mixed, misaligned out")
    assert (ref[0] == R.window(src[0], *corners[0], flips[0], H, W)).all()          # n_ops = 0: crop and flip alone
    # no sample with an operation at all: one copy launch
    t0 = R.table_of([[]] * B, corners, flips)
    assert DRA.launch_plan(t0) == (0, 0)
    assert_bytes(run_kernel(src, t0, H, W), R.randaugment(src, t0, H, W), f"{case} crop and flip")


# ---- 3. the histogram edge cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["3x3", "17x33", "64x48"])
def test_histogram_edge_cases(case):
    """A constant channel, a two-level image, a low-contrast ramp and noise under AutoContrast, Equalize and Contrast:
    3 x 3 has step = 0 (9 pixels), 17 x 33 = 561 and 64 x 48 have at least 510."""
    Hs, Ws, H, W = CASES[case]
    src = np.stack([R.image(300 + i, Hs, Ws, kind) for i, kind in enumerate(("constant", "two_level", "ramp", "noise"))])
    corners, flips = corners_flips(7, 4, Hs, Ws, H, W)
    ops = R.every_op(H, W)
    for name in ("autocontrast", "equalize", "contrast+", "contrast-"):
        t = R.table_of([[ops[name]]] * 4, corners, flips)
        assert_bytes(run_kernel(src, t, H, W), R.randaugment(src, t, H, W), f"{case} {name}")
    t = R.table_of([[ops["equalize"], ops["autocontrast"], ops["equalize"], ops["contrast+"]]] * 4, corners, flips)
    assert_bytes(run_kernel(src, t, H, W), R.randaugment(src, t, H, W), f"{case} four statistics slots")


# ---- 4. the training shape ------------------------------------------------------------------------------------------------
def test_224_from_256_three_operations():
    H = W = 224
    src = R.batch(400, 4, 256, 256, "ramp")
    corners, flips = corners_flips(8, 4, 256, 256, H, W)
    ops = R.every_op(H, W)
    chains = [[ops["rotate-"], ops["equalize"], ops["sharpness+"]], [ops["shear_y+"], ops["contrast+"], ops["color-"]],
              [ops["autocontrast"], ops["translate_x-"], ops["brightness+"]], [ops["solarize"], ops["posterize4"], ops["sharpness-"]]]
    t = R.table_of(chains, corners, flips)
    assert_bytes(run_kernel(src, t, H, W), R.randaugment(src, t, H, W, R.FILL), "224 from 256")


# ---- 5. records the host would refuse ---------------------------------------------------------------------------------------
def test_invalid_op_ids_bits_and_counts_are_harmless():
    Hs, Ws, H, W = CASES["17x33"]
    src = R.batch(500, B, Hs, Ws)
    ops = R.every_op(H, W)
    t = R.table_of([[ops["brightness+"], ops["posterize4"]]] * B, *corners_flips(9, B, Hs, Ws, H, W))
    t["op"][0, 0], t["op"][1, 0], t["op"][2, 1] = 10, -1, 2 ** 31 - 1          # skipped
    t["param"][3, 1], t["param"][4, 1] = 9, -3                                  # bits outside 0 .. 8: 8
    t["y0"][1], t["x0"][2] = 10 ** 6, -5                                        # clamped
    t["n_ops"][4] = 77                                                          # runs n_slots slots
    with pytest.raises(ValueError):
        DRA.check(t, H, W)
    ref = R.randaugment(src, t, H, W, R.FILL, n_slots=2, stats_mask=0)
    assert_bytes(run_kernel(src, t, H, W, plan=(2, 0)), ref, "invalid records")
    # a statistics operation in a slot whose bit the host did not set is skipped; wild coefficients address nothing outside
    t2 = R.table_of([[ops["equalize"], ops["rotate+"]]] * B)
    t2["coef"][:, 1] = (2 ** 31 - 1, -2 ** 31, 12345678, -2 ** 31, 2 ** 31 - 1, -87654321)
    assert_bytes(run_kernel(src, t2, H, W, plan=(2, 0)), R.randaugment(src, t2, H, W, R.FILL, n_slots=2, stats_mask=0),
                 "unset statistics bit, wrapping coefficients")


# ---- 6. repeatable, and a sample does not see its neighbours -----------------------------------------------------------------
def test_two_runs_agree_and_a_permuted_batch_permutes_the_output():
    Hs, Ws, H, W = CASES["64x48"]
    src = R.batch(200, B, Hs, Ws, "ramp")
    corners, flips = corners_flips(6, B, Hs, Ws, H, W)
    t = R.table_of(mixed_chains(H, W), corners, flips)
    a, b = run_kernel(src, t, H, W), run_kernel(src, t, H, W)
    assert torch.equal(a, b)
    perm = np.array([3, 0, 4, 2, 1])
    c = run_kernel(src[perm], t[perm], H, W)
    assert torch.equal(c, a[torch.from_numpy(perm).cuda()])


# ---- 7. the collate behind the stage ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", [False, True])
def test_collate_behind_the_stage_equals_collate_on_the_emulation(tokens):
    Hs, Ws, H, W = 40, 40, 32, 32
    src = R.batch(600, 4, Hs, Ws, "ramp")
    labels = torch.arange(4, device="cuda")
    outs = []
    for emulated in (False, True):
        col, ra = trainer.DeviceCollate(num_classes=10, seed=3), DRA(num_ops=3, seed=4, fill=(1, 2, 3))
        decisions = col.draw(4, H, W)
        corners = col.draw_corners(4, Hs, Ws, H, W)
        table = ra.draw(4, H, W)
        if emulated:
            t = np.array(table)
            t["y0"], t["x0"], t["flip"] = corners[:, 0], corners[:, 1], decisions[3].numpy()
            x = torch.from_numpy(R.randaugment(src, t, H, W, ra.fill)).cuda()
        else:
            x = ra(torch.from_numpy(np.array(src)).cuda(), corners, decisions[3], (H, W), table=table)
        outs.append(col(x, labels, decisions=(*decisions[:3], torch.zeros_like(decisions[3])), tokens=tokens))
    (xa, ya), (xb, yb) = outs
    assert tuple(xa.shape) == ((4, H, 3 * W) if tokens else (4, 3, H, W))
    assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)) and torch.equal(ya, yb)


# ---- 8. train(rand_augment=) --------------------------------------------------------------------------------------------------
class _U8Set(torch.utils.data.Dataset):
    def __init__(self, n=12):
        self.x = torch.from_numpy(np.stack([R.image(900 + i, 38, 38, "ramp") for i in range(n)]))
        self.y = torch.randint(0, 10, (n,), generator=torch.Generator().manual_seed(11))

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return self.x[i], int(self.y[i])


def _train(**kw):
    from test_host_logic_cpu import build_model
    torch.manual_seed(50)
    m = build_model("tiny32_cls", None).train()
    return trainer.train(m, "fused", scheduler=False, use_gpu=True, dataset=_U8Set(), epochs=2, batch_size=4, num_classes=10,
                         device_collate=True, device_augment=True, crop=(32, 32), log_every=1000, selfcheck=None, **kw)


def _same(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.mark.timeout(600)
def test_train_with_rand_augment_and_exact_resume(tmp_path):
    """2 epochs of 3 batches with the augmenting collate and erasing behind the stage.  num_ops = 0 is the run without the
    argument, bit for bit; three operations are another run; a run snapshotted behind step 2 and resumed equals the
    uninterrupted one, the stage's generator being in the snapshot."""
    plain = _train(random_erasing=0.5)
    assert _same(_train(random_erasing=0.5, rand_augment={"num_ops": 0}), plain)
    fa, fb = str(tmp_path / "a.snap"), str(tmp_path / "b.snap")
    kw = dict(random_erasing=0.5, rand_augment={"num_ops": 3, "fill": 128})
    full = _train(snapshot_path=fa, **kw)
    assert not _same(full, plain)
    assert all(torch.isfinite(v.float()).all() for v in full.state_dict().values())
    _train(snapshot_path=fb, max_steps=2, **kw)
    assert "rand_augment" in trainer.TrainState.read_header(fb)[0]["host"]["generators"]
    assert _same(_train(snapshot_path=fb, resume=fb, **kw), full)
    assert not torch.distributed.is_initialized()


# ---- 9. the stage behind the other input modes, both tasks, accumulation and a captured step ---------------------------------
class _Ragged(torch.utils.data.Dataset):
    """Decoded images (uint8 [h, w, 3]) of different sizes."""

    def __init__(self, n=8):
        rng = np.random.default_rng(21)
        self.items = [(np.ascontiguousarray(R.image(700 + i, int(rng.integers(40, 70)), int(rng.integers(40, 70)), "ramp")
                                            .transpose(1, 2, 0)), int(rng.integers(0, 10))) for i in range(n)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _two_steps(capsys, model="tiny32_cls", dataset=None, **kw):
    import re
    from test_host_logic_cpu import build_model
    torch.manual_seed(50)
    m = build_model(model, None).train()
    capsys.readouterr()
    torch.manual_seed(11)
    out = trainer.train(m, "fused", scheduler=False, use_gpu=True, dataset=dataset if dataset is not None else _U8Set(8), epochs=1,
                        batch_size=4, num_classes=10, device_collate=True, log_every=1, selfcheck=None, **kw)
    losses = re.findall(r"Loss: ([^,\n]+)", capsys.readouterr().out)
    assert len(losses) == 2 and all(np.isfinite(float(v)) for v in losses), losses
    return losses, out


class _U8Side(_U8Set):
    def __init__(self, side, n=8):
        self.x = torch.from_numpy(np.stack([R.image(900 + i, side, side, "ramp") for i in range(n)]))
        self.y = torch.randint(0, 10, (n,), generator=torch.Generator().manual_seed(11))


# mode -> (dataset, train()'s keywords); the ragged set feeds the resize stages, the others are stacked uint8 batches
MODES = {
    "resize": (_Ragged, dict(device_resize=(40, 40), crop=(32, 32))),
    "resize_window": (_Ragged, dict(device_resize=(40, 40), crop=(32, 32), resize_window=True)),
    "random_resized_crop": (_Ragged, dict(random_resized_crop=(32, 32))),
    "no_crop": (lambda: _U8Side(32), dict()),
    "reg": (lambda: _U8Side(52), dict(model="nano48_gen", task="reg", crop=(48, 48))),
    "accumulate": (lambda: _U8Side(38), dict(crop=(32, 32), accumulate=2)),
    "graph": (lambda: _U8Side(38), dict(crop=(32, 32), graph=True)),
}


def _mode_kw(mode):
    data, kw = MODES[mode]
    kw = dict(kw, dataset=data())
    if "random_resized_crop" in kw:                        # a fresh object per run: it owns a generator
        kw["random_resized_crop"] = trainer.DeviceResizedCrop.random_resized(kw["random_resized_crop"], seed=3)
    return kw


@pytest.fixture
def deterministic_gemm():
    """Trainings are compared bit for bit: the k-split weight gradients go through the workspace reduction instead of
    atomics, as in tests/test_determinism_gpu.py."""
    be = calm.backend.get_backend()
    prev = be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, 1)
    yield be
    be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, prev)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("mode", MODES)
def test_the_stage_composes_with_the_other_input_modes(capsys, deterministic_gemm, mode):
    """Two steps (accumulate: one optimizer step of two micro-batches, two log lines) with three operations per sample: the
    losses are finite and differ from the run without the stage; with num_ops = 0 the printed losses equal those of the run
    without the argument to the last digit."""
    ra = {"num_ops": 3, "magnitude": 15}
    plain, _ = _two_steps(capsys, **_mode_kw(mode))
    zero, _ = _two_steps(capsys, rand_augment={"num_ops": 0}, **_mode_kw(mode))
    full, _ = _two_steps(capsys, rand_augment=ra, **_mode_kw(mode))
    print(mode, plain, zero, full)
    if mode != "graph":                                    # (the capture's warm-up makes a captured run its own comparison)
        assert zero == plain
    assert full != plain


def test_resize_window_behind_the_stage_equals_the_whole_resize(capsys, deterministic_gemm):
    """The window holds the bytes of the crop of the whole resize, and the draws are made in the same order: the stage
    sees the same pixels either way."""
    ra = {"num_ops": 3, "magnitude": 15}
    a, _ = _two_steps(capsys, rand_augment=ra, **_mode_kw("resize"))
    b, _ = _two_steps(capsys, rand_augment=ra, **_mode_kw("resize_window"))
    assert a == b
