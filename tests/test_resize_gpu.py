"""calm_resize_u8 (csrc/resize.hip) against the numpy emulation of tests/emulated_resize.py and against recorded PIL
outputs.  PIL's 8-bit resample is integer arithmetic on coefficients computed in double, the kernel evaluates the same
coefficient function in fp64 on the device, and the integer sums are associative: every comparison is bit equality.

The ragged batch holds the 13 small sources of emulated_resize.CASES: a single tap (1x1), upscaling, the identity (8x8 to
8x8), tap counts clamped at both edges, a 1200-row and a 2049-column source that take several row chunks and several
rounds of horizontal taps, and outputs (17x23) that are no multiple of the 16x64 tile.  Every output buffer is allocated
with 64 sentinel bytes on either side."""
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import emulated_resize as ER
import make_golden_resize as MG
from helpers import CONFIGS, load_golden
from test_host_logic_cpu import build_model

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")

GUARD, SENTINEL = 64, 0x5A
OUTPUTS = [(8, 8), (17, 23), (256, 256)]
_cache = {}


def small_batch():
    if "src" not in _cache:
        _cache["src"] = [ER.image(500 + i, h, w) for i, (h, w) in enumerate(ER.SMALL_SOURCES)]
    return _cache["src"]


def small_reference(oh, ow):
    """The emulation's output for the ragged batch, computed once per output size and shared."""
    if (oh, ow) not in _cache:
        ref = ER.resize_batch(small_batch(), oh, ow)
        ref.setflags(write=False)
        _cache[(oh, ow)] = ref
    return _cache[(oh, ow)]


def run_kernel(imgs, oh, ow, pad=None, base_shift=0, front=GUARD):
    """-> uint8 [B,3,oh,ow] on the host; the sentinels around the output are checked here."""
    packed, meta = ER.pack(imgs, pad)
    dev = torch.cat([torch.zeros(base_shift, dtype=torch.uint8), torch.from_numpy(packed)]).cuda()[base_shift:]
    B, n = len(imgs), len(imgs) * 3 * oh * ow
    buf = torch.full((front + n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[front:front + n].view(B, 3, oh, ow)
    samples = trainer.DeviceResize.pack(meta, dev.numel(), device="cuda")
    calm.backend.get_backend().resize_u8(dev, samples, out)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:front] == SENTINEL).all() and (host[front + n:] == SENTINEL).all(), "a sentinel byte was overwritten"
    return host[front:front + n].reshape(B, 3, oh, ow)


def assert_equal(what, got, want):
    differing = int((got != want).sum())
    print(f"{what}: {differing} differing bytes of {want.size}")
    if differing:
        b, c, y, x = (int(v[0]) for v in np.nonzero(got != want))
        raise AssertionError(f"{what}: {differing} differing bytes; first at sample {b} channel {c} ({y}, {x}): "
                             f"{got[b, c, y, x]} != {want[b, c, y, x]}")


@pytest.mark.parametrize("size", OUTPUTS, ids=lambda s: f"to_{s[0]}x{s[1]}")
def test_ragged_batch_equals_the_emulation(size):
    assert_equal(f"13 sources -> {size}", run_kernel(small_batch(), *size), small_reference(*size))


@pytest.mark.parametrize("size", OUTPUTS, ids=lambda s: f"to_{s[0]}x{s[1]}")
def test_images_at_odd_byte_offsets(size):
    """1, 2, 3 bytes of filler between the images, and the buffer itself starting at an odd address: the aligned-dword
    loads select the same bytes.  The output starts 67 bytes into its buffer as well (byte stores)."""
    want = small_reference(*size)
    assert_equal(f"odd offsets -> {size}", run_kernel(small_batch(), *size, pad=(1, 2, 3)), want)
    assert_equal(f"odd base -> {size}", run_kernel(small_batch(), *size, pad=(3, 1, 2), base_shift=1, front=67), want)


def test_batch_of_one_and_of_sixty_five():
    src = small_batch()
    one = [src[9]]                                                   # 255 x 257
    assert_equal("B = 1", run_kernel(one, 17, 23), small_reference(17, 23)[9:10])
    order = [i % 9 for i in range(65)]                               # the nine sources up to 100 x 75, cycled
    assert_equal("B = 65", run_kernel([src[i] for i in order], 17, 23), small_reference(17, 23)[order])


@pytest.mark.parametrize("value", [0, 255])
def test_constant_images_come_back_unchanged(value):
    imgs = [np.full((h, w, 3), value, dtype=np.uint8) for h, w in ER.SMALL_SOURCES]
    for oh, ow in ((17, 23), (256, 256)):
        out = run_kernel(imgs, oh, ow)
        assert (out == value).all(), (value, oh, ow, np.unique(out))


def test_output_equals_the_recorded_pil_output():
    g = np.load(MG.PATH)
    for i, (_, (oh, ow)) in enumerate(ER.CASES[:MG.N_SMALL]):
        assert_equal(f"PIL case {i}", run_kernel([g[f"src_{i}"]], oh, ow)[0], g[f"out_{i}"].transpose(2, 0, 1))
    big = run_kernel([ER.image(seed, *MG.BIG_SRC) for seed in MG.BIG_SEEDS], *MG.BIG_OUT)
    for i in range(len(MG.BIG_SEEDS)):
        assert_equal(f"PIL 500x375 corner {i}", MG.big_corner(i, big[i].transpose(1, 2, 0)), g[f"big_{i}"])


def test_a_record_outside_the_buffer_is_not_read_and_gives_zeros():
    """The records live on the device, so the launch cannot refuse one: a side of 0 or above 16384, a negative offset and an
    image that ends past nbytes leave zeros (trainer.DeviceResize refuses them on the host; here they go to the backend
    directly), and the good images beside them are resized as ever."""
    src = small_batch()
    good = [src[5], src[8]]                                          # 13 x 29, 100 x 75
    packed, meta = ER.pack(good)
    n = packed.size
    bad = [(0, 0, 8), (0, 8, 16385), (-16, 4, 4), (n - 11, 2, 2), (n + 4096, 2, 2), (0, 16384, 16384)]
    rec = np.zeros(2 + len(bad), dtype=trainer.DeviceResize.dtype())
    rows = [tuple(meta[0])] + bad[:3] + [tuple(meta[1])] + bad[3:]
    rec["offset"], rec["h"], rec["w"] = (np.asarray(v, dtype=np.int64) for v in zip(*rows))
    samples = torch.from_numpy(rec.view(np.uint8).reshape(len(rec), 16)).cuda()
    out = torch.full((len(rec), 3, 17, 23), SENTINEL, dtype=torch.uint8, device="cuda")
    calm.backend.get_backend().resize_u8(torch.from_numpy(packed).cuda(), samples, out)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    ref = small_reference(17, 23)
    assert_equal("good records", out[[0, 4]], ref[[5, 8]])
    assert (out[[1, 2, 3, 5, 6, 7]] == 0).all()


def test_two_calls_are_bit_identical():
    a, b = run_kernel(small_batch(), 17, 23), run_kernel(small_batch(), 17, 23)
    assert np.array_equal(a, b)


# ---- through DeviceResize, DeviceCollate and the launcher ---------------------------------------------------------------
class Ragged(torch.utils.data.Dataset):
    """12 decoded images of 40 .. 90 pixels per side, as np.asarray(pil_image) gives them."""

    def __init__(self, classes, n=12, seed=7):
        rng = np.random.default_rng(seed)
        self.items = [(ER.image(seed + i, int(rng.integers(40, 91)), int(rng.integers(40, 91))), int(rng.integers(0, classes)))
                      for i in range(n)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_resize_then_collate_equals_collate_over_the_emulated_resize():
    """device_resize=(56, 56) in front of DeviceCollate(crop=(48, 48), tokens=True): tokens and soft labels equal, exactly,
    those of the same seeded DeviceCollate over the stack the emulation resized — the draws do not move."""
    data = Ragged(10)
    packed, meta, labels = trainer.RaggedU8Collate()([data[i] for i in range(len(data))])
    assert len({tuple(m[1:]) for m in meta.tolist()}) > 6            # ragged indeed
    resized = trainer.DeviceResize((56, 56))(packed.cuda(), meta)
    want_u8 = ER.resize_batch([img for img, _ in data.items], 56, 56)
    assert_equal("DeviceResize", resized.cpu().numpy(), want_u8)
    x, y = trainer.DeviceCollate(num_classes=10, seed=31)(resized, labels.cuda(), crop=(48, 48), tokens=True)
    xr, yr = trainer.DeviceCollate(num_classes=10, seed=31)(torch.from_numpy(want_u8).cuda(), labels.cuda(), crop=(48, 48),
                                                            tokens=True)
    assert tuple(x.shape) == (12, 48, 144) and torch.equal(x.view(torch.int32), xr.view(torch.int32))
    assert torch.equal(y.view(torch.int32), yr.view(torch.int32))


def test_train_launcher_with_device_resize(capsys):
    """trainer.train(device_collate=True, device_augment=True, device_resize=(56, 56)): decoded images of any size -> one
    packed H2D copy -> resize -> the augmenting collate -> the model; two steps on the nano configuration, finite loss."""
    name = "nano48_cls"
    g = load_golden(name)
    cfg = CONFIGS[name]
    S = cfg.seq_length
    assert S == 48
    m = build_model(name, g, "cpu")
    out = trainer.train(m, "fused", scheduler=False, use_gpu=True, dataset=Ragged(cfg.out_features), epochs=1, batch_size=4,
                        num_classes=cfg.out_features, device_collate=True, device_augment=True, device_resize=(56, 56),
                        crop=(S, S), max_steps=2, log_every=1)
    losses = [float(v) for v in re.findall(r"Loss: ([^,]+),", capsys.readouterr().out)]
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    assert all(torch.isfinite(v.float()).all() for v in out.state_dict().values())
