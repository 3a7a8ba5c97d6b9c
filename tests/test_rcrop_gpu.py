"""calm_resized_crop (csrc/resized_crop.hip) against the numpy emulation of tests/emulated_rcrop.py — crop the box, resize
it as PIL does, keep the window.  The uint8 output is integer arithmetic on coefficients the kernel computes in fp64 with
the functions the host entry point is tested with: every uint8 comparison is equality.  The fp32 outputs are held to the
float64 n(v) at 2e-5 absolute, the bound tests/test_augment_gpu.py holds the normalised output to.

The packed buffer holds the 13 small sources of emulated_resize.SMALL_SOURCES (1x1 .. 64x2049, the last one 3x700) and
the records point into it: whole images, 1x1 boxes, the last rows and columns of the last image of the buffer, odd bx0,
and a 3x700 box squeezed to 8 columns (up to 2 * 88 + 1 = 177 taps, taken in rounds of 32).  Every output buffer has 64 sentinel bytes on
either side."""
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import emulated_rcrop as EC
import emulated_resize as ER
from helpers import CONFIGS, load_golden
from test_host_logic_cpu import build_model

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
DRC = trainer.DeviceResizedCrop

GUARD, SENTINEL = 64, 0x5A
TOL = 2e-5
# H x W of the window and its corner (wy0, wx0): one tile and less, two tiles each way with scalar stores, one whole tile
WINDOWS = [((8, 8), (0, 0)), ((8, 8), (1, 3)), ((17, 65), (0, 0)), ((17, 65), (3, 1)), ((16, 64), (0, 0)), ((16, 64), (1, 5))]
_cache = {}


def sources():
    if "src" not in _cache:
        _cache["src"] = [ER.image(700 + i, h, w) for i, (h, w) in enumerate(ER.SMALL_SOURCES)]
    return _cache["src"]


def records_for(size, corner):
    """(image index, box (by0, bx0, bh, bw), (vh, vw), (wy0, wx0)) for one window: the resized size differs per sample
    (up- and downscaling on either axis), the window is the launch's."""
    (H, W), (wy0, wx0) = size, corner
    shapes = ER.SMALL_SOURCES
    last = len(shapes) - 1
    assert shapes[last] == (3, 700) and shapes[7] == (37, 64) and shapes[8] == (100, 75) and shapes[9] == (255, 257)
    rec = []
    for i, (h, w) in enumerate(shapes):                                       # the whole image
        rec.append((i, (0, 0, h, w), (H + wy0 + i % 3, W + wx0 + i % 5), corner))
    for i in (0, 5, 9):                                                       # 1x1 boxes: a corner, the interior, the end
        h, w = shapes[i]
        rec.append((i, (h // 2, w // 2, 1, 1), (H + wy0, W + wx0 + 2), corner))
    rec.append((9, (254, 256, 1, 1), (H + wy0 + 1, W + wx0), corner))
    rec.append((last, (1, 695, 2, 5), (H + wy0, W + wx0 + 1), corner))        # the last rows and columns of the last image
    rec.append((last, (2, 699, 1, 1), (H + wy0, W + wx0), corner))            # the last pixel of the buffer
    rec.append((last, (0, 693, 3, 7), (H + wy0 + 2, W + wx0), corner))
    rec.append((7, (1, 3, 30, 51), (H + wy0 + 1, W + wx0 + 4), corner))       # odd bx0
    rec.append((8, (5, 7, 90, 61), (H + wy0, W + wx0 + 3), corner))
    rec.append((11, (3, 1001, 60, 1040), (H + wy0 + 2, W + wx0), corner))     # 64x2049: several rounds of taps at 8 columns
    if (W, wx0) == (8, 0):
        rec.append((last, (0, 0, 3, 700), (H + wy0, 8), corner))              # 3x700 -> 8 columns: 2 * 88 + 1 taps, rounds of 32
        assert 700 / 8 > 32
    return rec


def reference(size, corner):
    """The emulation's uint8 [B,3,H,W] for records_for(size, corner), computed once and shared."""
    key = ("ref", size, corner)
    if key not in _cache:
        ref = EC.rcrop_batch(sources(), records_for(size, corner), *size)
        ref.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def to_table(rec, meta):
    t = np.zeros(len(rec), dtype=DRC.dtype())
    for k, (i, box, vsize, corner) in enumerate(rec):
        t[k] = (meta[i][0], meta[i][1], meta[i][2]) + tuple(box) + tuple(vsize) + tuple(corner)
    return t


def run_kernel(rec, H, W, kind="u8", pad=None, base_shift=0, front=GUARD, table=None, imgs=None):
    """-> the output on the host ([B,3,H,W] uint8 / fp32 or [B,H,3W] fp32); the sentinels around it are checked here.
    rec: records_for's tuples (checked on the host as DeviceResizedCrop would) or, table=..., a ready record array."""
    packed, meta = ER.pack(sources() if imgs is None else imgs, pad)
    dev = torch.cat([torch.zeros(base_shift, dtype=torch.uint8), torch.from_numpy(packed)]).cuda()[base_shift:]
    if table is None:
        table = to_table(rec, meta)
        assert DRC.valid(table, dev.numel(), H, W).all()
    B = len(table)
    item = 1 if kind == "u8" else 4
    n = B * 3 * H * W * item
    assert front % item == 0
    buf = torch.full((front + n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[front:front + n]
    if kind == "u8":
        out = out.view(B, 3, H, W)
    else:
        out = out.view(torch.float32).view((B, H, 3 * W) if kind == "tokens" else (B, 3, H, W))
    samples = torch.from_numpy(table.view(np.uint8).reshape(B, 48)).cuda()
    if kind == "u8":
        calm.backend.get_backend().resized_crop(dev, samples, out)
    else:
        calm.backend.get_backend().resized_crop(dev, samples, out, EC.MEAN, EC.STD, tokens=kind == "tokens")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:front] == SENTINEL).all() and (host[front + n:] == SENTINEL).all(), "a sentinel byte was overwritten"
    body = host[front:front + n]
    return body.reshape(B, 3, H, W) if kind == "u8" else body.view(np.float32).reshape(out.shape)


def assert_equal(what, got, want):
    differing = int((got != want).sum())
    print(f"{what}: {differing} differing bytes of {want.size}")
    if differing:
        b, c, y, x = (int(v[0]) for v in np.nonzero(got != want))
        raise AssertionError(f"{what}: {differing} differing bytes; first at record {b} channel {c} ({y}, {x}): "
                             f"{got[b, c, y, x]} != {want[b, c, y, x]}")


def assert_close(what, got, want):
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{what}: max |error| {err:.3g} (bound {TOL:g})")
    assert np.isfinite(got).all() and err <= TOL, (what, err)


_ids = [f"{h}x{w}_at_{y}_{x}" for (h, w), (y, x) in WINDOWS]


# ---- 1. a ragged batch, kind 0 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,corner", WINDOWS, ids=_ids)
def test_ragged_batch_equals_the_emulation(size, corner):
    rec = records_for(size, corner)
    assert_equal(f"{len(rec)} records -> {size} at {corner}", run_kernel(rec, *size), reference(size, corner))


@pytest.mark.parametrize("size,corner", WINDOWS, ids=_ids)
def test_images_at_odd_byte_offsets(size, corner):
    """1, 2, 3 bytes of filler between the images, and the buffer itself starting at an odd address: the aligned-dword
    loads select the same bytes, and the last image still ends with the buffer.  The output starts 67 bytes into its
    buffer as well (byte stores)."""
    rec, want = records_for(size, corner), reference(size, corner)
    assert_equal(f"odd offsets -> {size}", run_kernel(rec, *size, pad=(1, 2, 3)), want)
    assert_equal(f"odd base -> {size}", run_kernel(rec, *size, pad=(3, 1, 2), base_shift=1, front=67), want)


def test_batch_of_one_and_of_sixty_five():
    size, corner = (17, 65), (3, 1)
    rec, want = records_for(size, corner), reference(size, corner)
    k = 17                                                           # the last rows and columns of the last image
    assert rec[k][0] == len(ER.SMALL_SOURCES) - 1 and rec[k][1] == (1, 695, 2, 5)
    assert_equal("B = 1", run_kernel([rec[k]], *size), want[k:k + 1])
    order = [(7 * i) % len(rec) for i in range(65)]
    assert_equal("B = 65", run_kernel([rec[i] for i in order], *size), want[order])


# ---- 2. the kernel it generalises -----------------------------------------------------------------------------------------
def ragged_images(n=12, seed=7):
    """Decoded images of 40 .. 90 pixels per side, as np.asarray(pil_image) gives them."""
    rng = np.random.default_rng(seed)
    return [ER.image(seed + i, int(rng.integers(40, 91)), int(rng.integers(40, 91))) for i in range(n)]


def test_window_equals_resize_u8_sliced():
    """.window((56, 56), (48, 48)) with given corners: the bytes calm_resize_u8 writes for 56 x 56, sliced."""
    imgs = ragged_images()
    packed, meta, _ = trainer.RaggedU8Collate()([(a, 0) for a in imgs])
    dev = packed.cuda()
    whole = trainer.DeviceResize((56, 56))(dev, meta).cpu().numpy()
    corners = np.stack([np.arange(12) % 9, (3 * np.arange(12) + 1) % 9], axis=1).astype(np.int32)
    corners[0], corners[1] = (0, 0), (8, 8)
    win = DRC.window((56, 56), (48, 48))
    got = win(dev, meta, corners=corners).cpu().numpy()
    assert got.shape == (12, 3, 48, 48) and win.last_records["wy0"].tolist() == corners[:, 0].tolist()
    want = np.stack([whole[b, :, y:y + 48, x:x + 48] for b, (y, x) in enumerate(corners)])
    assert_equal(".window against calm_resize_u8", got, want)


# ---- 3. kinds 1 and 2 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,corner", [WINDOWS[1], WINDOWS[3], WINDOWS[5]], ids=[_ids[1], _ids[3], _ids[5]])
def test_fp32_image_and_tokens(size, corner):
    """Both fp32 kinds within 2e-5 of the float64 n(v) of the emulated bytes; the two are permutations of each other, bit
    for bit; from a base that is 4- but not 16-byte aligned (scalar stores) the same bits."""
    rec = records_for(size, corner)
    want = EC.normalise(reference(size, corner))
    image = run_kernel(rec, *size, kind="image")
    tokens = run_kernel(rec, *size, kind="tokens")
    assert_close(f"image {size}", image, want)
    assert_close(f"tokens {size}", tokens, EC.tokens(want))
    assert np.array_equal(EC.tokens(image).view(np.int32), tokens.view(np.int32))
    assert np.array_equal(image.view(np.int32), EC.normalise_f32(reference(size, corner)).view(np.int32))    # the header's fp32 form
    assert np.array_equal(run_kernel(rec, *size, kind="image", front=68).view(np.int32), image.view(np.int32))
    assert np.array_equal(run_kernel(rec, *size, kind="tokens", front=68).view(np.int32), tokens.view(np.int32))


def test_fp32_output_against_the_collate_over_the_uint8_output():
    """calm_collate_crop_mix(mode 0) over the kind-0 output is the two-launch form of kinds 1 and 2.  Both are within 2e-5
    of the float64 value (the collate is held to that by tests/test_augment_gpu.py), so they differ by at most 4e-5; the
    worst difference is printed (a measurement; DESIGN.md records it)."""
    size, corner = (16, 64), (1, 5)
    rec = records_for(size, corner)
    u8 = torch.from_numpy(run_kernel(rec, *size)).cuda()
    B = len(rec)
    be = calm.backend.get_backend()
    for kind in ("image", "tokens"):
        two = torch.empty((B, size[0], 3 * size[1]) if kind == "tokens" else (B, 3) + size, dtype=torch.float32, device="cuda")
        be.collate_crop_mix(u8, None, None, two, 0, 1.0, None, EC.MEAN, EC.STD, tokens=kind == "tokens")
        one = run_kernel(rec, *size, kind=kind)
        diff = np.abs(one.astype(np.float64) - two.cpu().numpy().astype(np.float64))
        print(f"{kind}: worst |one launch - resize then collate| = {diff.max():.3g}, {int((diff != 0).sum())} of {diff.size} differ")
        assert diff.max() <= 2 * TOL


# ---- 4. safety and repeatability ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "image", "tokens"])
def test_two_calls_are_bit_identical(kind):
    size, corner = (17, 65), (3, 1)
    rec = records_for(size, corner)
    a, b = run_kernel(rec, *size, kind=kind), run_kernel(rec, *size, kind=kind)           # (sentinels checked in each)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def invalid_table(size, corner):
    """Nine good records with 26 that fail calm_resized_crop_check among them -> (records, which are good, nbytes)."""
    import ctypes
    H, W = size
    packed, meta = ER.pack(sources())
    n = packed.size
    table = to_table(records_for(size, corner)[:9], meta)
    g = table[8].copy()                                              # 100 x 75, whole, to 11 x 14, window 8 x 8 at (1, 3)
    assert (int(g["h"]), int(g["w"]), int(g["vh"]), int(g["vw"])) == (100, 75, 11, 14) and (size, corner) == ((8, 8), (1, 3))
    bad = []
    for change in (dict(h=0), dict(w=16385), dict(offset=-16), dict(offset=n - 11), dict(offset=n + 4096),
                   dict(offset=1 << 62), dict(h=16384, w=16384), dict(by0=-1), dict(bx0=-3), dict(bh=0), dict(bw=-7),
                   dict(by0=1), dict(bx0=1), dict(bh=101), dict(bw=1 << 30), dict(by0=(1 << 31) - 1, bh=(1 << 31) - 1),
                   dict(vh=0), dict(vw=16385), dict(vh=8), dict(vw=10), dict(wy0=-1), dict(wx0=-2), dict(wy0=4), dict(wx0=7),
                   dict(wy0=(1 << 31) - 1), dict(vh=-4, wy0=-20)):
        r = g.copy()
        for f, v in change.items():
            r[f] = v
        bad.append(r)
    lib = binding.load()
    for r in bad:                                                    # every one fails the host check, the kernel's guard
        assert lib.calm_resized_crop_check(ctypes.byref(binding.RCropSample.from_buffer_copy(r.tobytes())), n, H, W) == 0
    for r in table:
        assert lib.calm_resized_crop_check(ctypes.byref(binding.RCropSample.from_buffer_copy(r.tobytes())), n, H, W) == 1
    rows = np.concatenate([table[:4], np.array(bad[:13], dtype=table.dtype), table[4:], np.array(bad[13:], dtype=table.dtype)])
    is_good = np.asarray([True] * 4 + [False] * 13 + [True] * 5 + [False] * (len(bad) - 13))
    assert DRC.valid(rows, n, H, W).tolist() == is_good.tolist()
    return rows, is_good, n


@pytest.mark.parametrize("kind", ["u8", "image", "tokens"])
def test_invalid_records_are_not_read_and_give_the_output_of_zeros(kind):
    """The records live on the device, so the launch cannot refuse one.  Each bad record below fails
    calm_resized_crop_check — the function the kernel evaluates before it forms any address (resized_crop.hip: `ok`, which
    gates the taps, so that an invalid record has no rows to walk and no load is issued) — and leaves zeros, or n(0),
    beside good records that come out as ever."""
    size, corner = (8, 8), (1, 3)
    H, W = size
    rows, is_good, n = invalid_table(size, corner)
    out = run_kernel(None, H, W, kind=kind, table=rows)
    want = reference(size, corner)[:9]
    if kind == "u8":
        assert_equal("good records", out[is_good], want)
        assert (out[~is_good] == 0).all()
        return
    want, zero = EC.normalise(want), EC.normalise(np.zeros((1, 3, H, W), dtype=np.uint8))
    if kind == "tokens":
        want, zero = EC.tokens(want), EC.tokens(zero)
    assert_close("good records", out[is_good], want)
    assert_close("bad records", out[~is_good], np.broadcast_to(zero, out[~is_good].shape))


# ---- 5. through the public interface --------------------------------------------------------------------------------------
class Ragged(torch.utils.data.Dataset):
    def __init__(self, classes, n=12, seed=7):
        rng = np.random.default_rng(seed + 100)
        self.items = [(a, int(rng.integers(0, classes))) for a in ragged_images(n, seed)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_evaluate_with_a_center_transform_equals_evaluate_over_the_emulated_batch():
    """evaluate(transform=.center(56, (48, 48))) over packed originals against evaluate over the batch the emulation makes
    — Resize(56) + CenterCrop(48) in numpy, then the header's fp32 n(v), as tokens: the inputs are equal bit for bit, so the
    logits are, and the accuracy is the same.  Also as the image, and through the lean, graph-replayed forward."""
    name = "nano48_cls"
    cfg = CONFIGS[name]
    m = build_model(name, load_golden(name), "cuda").train()
    imgs = ragged_images()
    tr = DRC.center(56, (48, 48))
    collate = trainer.RaggedU8Collate()
    batches, refs, logits = [], [], {"dev": [], "ref": []}
    for lo in (0, 8):                                                # a batch of 8 and a ragged last one of 4
        part = imgs[lo:lo + 8]
        packed, meta, _ = collate([(a, 0) for a in part])
        t = tr.records(meta, packed.numel())
        u8 = EC.rcrop_batch(part, [(i, tuple(int(t[i][f]) for f in ("by0", "bx0", "bh", "bw")), (int(t[i]["vh"]), int(t[i]["vw"])),
                                    (int(t[i]["wy0"]), int(t[i]["wx0"]))) for i in range(len(part))], 48, 48)
        batches.append((packed, meta))
        refs.append(torch.from_numpy(EC.tokens(EC.normalise_f32(u8))).cuda())
    with torch.no_grad():
        m.eval()
        labels = [m(x)[0].reshape(x.shape[0], -1).argmax(dim=1) for x in refs]
        m.train()
    labels[0] = (labels[0] + torch.arange(8, device="cuda") % 2) % cfg.out_features        # some misses
    side = "ref"
    hook = m.register_forward_hook(lambda mod, args, out: logits[side].append(out[0].detach().float().cpu()))
    try:
        acc = trainer.evaluate(m, list(zip(refs, labels)))
        side = "dev"
        got = trainer.evaluate(m, [(p, mt, lb.cpu()) for (p, mt), lb in zip(batches, labels)], transform=tr)
        image = trainer.evaluate(m, [(p, mt, lb) for (p, mt), lb in zip(batches, labels)], transform=tr, transform_out="image")
    finally:
        hook.remove()
    lean = trainer.evaluate(m, [(p, mt, lb) for (p, mt), lb in zip(batches, labels)], transform=tr, lean=True, graph=True)
    assert 0.0 < acc < 1.0 and got == acc and image == acc and lean == acc
    assert len(logits["ref"]) == 2 and len(logits["dev"]) == 4
    for k in range(2):
        worst = float((logits["dev"][k] - logits["ref"][k]).abs().max())
        print(f"batch {k}: worst logit difference {worst:.3g} (tokens), "
              f"{float((logits['dev'][2 + k] - logits['ref'][k]).abs().max()):.3g} (image)")
        assert torch.equal(logits["dev"][k], logits["ref"][k])
    assert m.training


@pytest.fixture
def deterministic_gemm():
    """Two trainings are compared bit for bit: the k-split weight gradients go through the workspace reduction instead of
    atomics (CALM_GEMM_OPT_DETERMINISTIC), as in tests/test_determinism_gpu.py — with atomics a step does not repeat itself."""
    be = calm.backend.get_backend()
    prev = be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, 1)
    yield be
    be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, prev)


def _train(capsys, **kw):
    name = "nano48_cls"
    cfg = CONFIGS[name]
    m = build_model(name, load_golden(name), "cpu")
    capsys.readouterr()
    torch.manual_seed(11)                                           # the model's latent noise comes from torch's generator
    out = trainer.train(m, "fused", scheduler=False, use_gpu=True, dataset=Ragged(cfg.out_features), epochs=1, batch_size=4,
                        num_classes=cfg.out_features, device_collate=True, max_steps=2, log_every=1, **kw)
    losses = re.findall(r"Loss: ([^,]+),", capsys.readouterr().out)
    assert len(losses) == 2 and all(np.isfinite(float(v)) for v in losses), losses
    return losses, out.state_dict()


@pytest.mark.parametrize("augment", [False, True], ids=["collate", "augmenting_collate"])
def test_train_with_resize_window_equals_train_without(capsys, deterministic_gemm, augment):
    """Two steps of train(device_resize=(56, 56), crop=(48, 48), resize_window=True) against the same steps without the
    flag: the draws are made in the same order and the window holds the same bytes, so loss and parameters are equal bit
    for bit."""
    kw = dict(device_resize=(56, 56), crop=(48, 48), device_augment=augment)
    losses_a, sd_a = _train(capsys, **kw)
    losses_b, sd_b = _train(capsys, resize_window=True, **kw)
    assert losses_a == losses_b, (losses_a, losses_b)
    keys = [k for k, v in sd_a.items() if v.is_floating_point() and v.numel() > 8]
    for k in keys[:: max(len(keys) // 6, 1)]:
        assert torch.equal(sd_a[k].view(torch.int32), sd_b[k].view(torch.int32)), k
    assert losses_a[0] != losses_a[1]


def test_train_with_random_resized_crop_runs_and_repeats(capsys, deterministic_gemm):
    runs = [_train(capsys, random_resized_crop=DRC.random_resized((48, 48), seed=3)) for _ in range(2)]
    assert runs[0][0] == runs[1][0]
    keys = [k for k, v in runs[0][1].items() if v.is_floating_point() and v.numel() > 8]
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in keys[:: max(len(keys) // 6, 1)])
    other, _ = _train(capsys, random_resized_crop=DRC.random_resized((48, 48), seed=4))
    assert other != runs[0][0]
