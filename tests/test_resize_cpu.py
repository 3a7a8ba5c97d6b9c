"""Device resize without a GPU: the numpy emulation the kernel is tested against (tests/emulated_resize.py) against PIL
itself and against the committed PIL outputs, byte for byte; the host definition of the coefficients
(calm_resize_coeffs, the function the kernel evaluates on the device) against the emulation, exactly; the host logic of
trainer.RaggedU8Collate / DeviceResize; the argument checks of train(device_resize=) and of the two entry points; the
layout of struct calm_resize_sample.

PIL's 8-bit resample is integer arithmetic on coefficients computed in double, so every comparison here is equality."""
import ctypes
import os
import pickle
import subprocess
import sys
import tempfile
from importlib import import_module

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import calm_vit_dte_amd as calm  # noqa: E402,F401
import emulated_resize as ER  # noqa: E402
import make_golden_resize as MG  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")


@pytest.fixture(scope="module")
def golden():
    return np.load(MG.PATH)


# ---- the emulation is PIL -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ER.CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}_to_{c[1][0]}x{c[1][1]}")
def test_emulation_equals_pil_byte_for_byte(case):
    (h, w), (oh, ow) = case
    src = ER.image(100 + h * 7 + w, h, w)
    assert h * w < 64 or (src.min() == 0 and src.max() == 255)
    want = MG.pil_resize(src, oh, ow)
    got = ER.resize(src, oh, ow)
    differing = int((got != want).sum())
    print(f"{h}x{w} -> {oh}x{ow}: {differing} differing bytes of {want.size}")
    assert got.shape == want.shape == (oh, ow, 3) and differing == 0


def test_emulation_equals_the_committed_pil_outputs(golden):
    for i, ((h, w), (oh, ow)) in enumerate(ER.CASES[:MG.N_SMALL]):
        src = golden[f"src_{i}"]
        assert src.shape == (h, w, 3) and np.array_equal(src, ER.image(MG.SEED + i, h, w))      # the seeded inputs reproduce
        assert np.array_equal(ER.resize(src, oh, ow), golden[f"out_{i}"]), (h, w, oh, ow)
    for i, seed in enumerate(MG.BIG_SEEDS):
        out = ER.resize(ER.image(seed, *MG.BIG_SRC), *MG.BIG_OUT)
        assert np.array_equal(MG.big_corner(i, out), golden[f"big_{i}"]), seed
    assert os.path.getsize(MG.PATH) < 256 * 1024


# ---- the host definition of the coefficients ------------------------------------------------------------------------------
def _host_coeffs(lib, n_in, n_out, ksize):
    bounds = np.full(2 * n_out, -1, dtype=np.int32)
    kk = np.full(n_out * ksize, -1, dtype=np.int32)
    rc = lib.calm_resize_coeffs(n_in, n_out, bounds.ctypes.data, kk.ctypes.data, ksize)
    assert rc == 0, (n_in, n_out, rc)
    return bounds[0::2], bounds[1::2], kk.reshape(n_out, ksize)


def _axis_cases():
    return [(i, o) for o in (8, 16, 256) for i in range(1, 601)] + [(i, 256) for i in (2049, 8191, 16384)]


def test_host_coefficients_equal_the_emulation_exactly():
    lib = binding.load()
    for n_in, n_out in _axis_cases():
        lo, n, k = ER.coeffs(n_in, n_out)
        hlo, hn, hk = _host_coeffs(lib, n_in, n_out, k.shape[1])
        assert np.array_equal(hlo, lo) and np.array_equal(hn, n) and np.array_equal(hk, k), (n_in, n_out)


def test_every_coefficient_row_sums_to_one_within_its_rounding():
    """k[j] = (int)(0.5 + w[j] 2^22) with sum w = 1: each of the n terms is rounded by at most one half, so the row is
    within n / 2 of 2^22 — asserted with the bound n."""
    lib = binding.load()
    for n_in, n_out in _axis_cases():
        ksize = 2 * (-(-n_in // n_out) if n_in > n_out else 1) + 1
        lo, n, k = _host_coeffs(lib, n_in, n_out, ksize)
        assert (n >= 1).all() and (lo >= 0).all() and (lo + n <= n_in).all() and (k >= 0).all()
        assert (np.abs(k.astype(np.int64).sum(axis=1) - (1 << 22)) <= n).all(), (n_in, n_out)
        assert (np.diff(lo) >= 0).all() and (np.diff(lo + n) >= 0).all()      # what the kernel's row range relies on


def test_same_size_is_the_identity():
    for n in (1, 2, 7, 256):
        lo, cnt, k = ER.coeffs(n, n)
        assert np.array_equal(lo, np.arange(n)) and (k[:, 0] == 1 << 22).all() and (k[:, 1:] == 0).all()
    src = ER.image(3, 19, 23)
    assert np.array_equal(ER.resize(src, 19, 23), src)


# ---- RaggedU8Collate / DeviceResize -------------------------------------------------------------------------------------
def _ragged(seed=0):
    sizes = [(1, 1), (5, 7), (40, 33), (16, 16), (3, 90)]
    return [(ER.image(seed + i, h, w), i % 3) for i, (h, w) in enumerate(sizes)]


def test_ragged_collate_round_trips_sizes_offsets_and_bytes():
    batch = _ragged()
    batch[1] = (torch.from_numpy(batch[1][0]), torch.tensor(batch[1][1]))      # a tensor sample beside arrays
    packed, meta, labels = trainer.RaggedU8Collate()(batch)
    assert packed.dtype == torch.uint8 and packed.dim() == 1 and meta.dtype == torch.int64 and tuple(meta.shape) == (5, 3)
    assert labels.dtype == torch.int64 and labels.tolist() == [0, 1, 2, 0, 1]
    end = 0
    for (img, _), (off, h, w) in zip(batch, meta.tolist()):
        img = np.asarray(img)
        assert (h, w) == img.shape[:2] and off % 16 == 0 and end <= off < end + 16
        assert np.array_equal(packed[off:off + 3 * h * w].numpy().reshape(h, w, 3), img)
        end = off + 3 * h * w
    assert packed.numel() == end
    clone = pickle.loads(pickle.dumps(trainer.RaggedU8Collate()))                # what a worker process receives
    assert all(torch.equal(a, b) for a, b in zip(clone(batch), (packed, meta, labels)))
    with pytest.raises(TypeError):
        trainer.RaggedU8Collate()([(np.zeros((3, 8, 8), dtype=np.float32), 0)])
    with pytest.raises(TypeError):
        trainer.RaggedU8Collate()([(np.zeros((8, 8), dtype=np.uint8), 0)])


def test_ragged_collate_in_loader_workers():
    class Data(torch.utils.data.Dataset):
        def __len__(self):
            return 6

        def __getitem__(self, i):
            return ER.image(i, 4 + i, 9 - i), i

    direct = [trainer.RaggedU8Collate()([Data()[i] for i in idx]) for idx in ((0, 1, 2, 3), (4, 5))]
    loader = torch.utils.data.DataLoader(Data(), batch_size=4, collate_fn=trainer.RaggedU8Collate(), num_workers=1)
    got = list(loader)
    assert len(got) == 2
    for g, d in zip(got, direct):
        assert all(torch.equal(a, b) for a, b in zip(g, d))


def test_device_resize_records_and_their_checks():
    packed, meta, _ = trainer.RaggedU8Collate()(_ragged())
    rec = trainer.DeviceResize.records(meta, packed.numel())
    assert rec.dtype.itemsize == 16 == ctypes.sizeof(binding.ResizeSample)
    assert rec["offset"].tolist() == meta[:, 0].tolist() and rec["h"].tolist() == meta[:, 1].tolist()
    one = binding.ResizeSample.from_buffer_copy(rec[2].tobytes())                  # the ctypes mirror reads the same record
    assert (one.offset, one.h, one.w) == tuple(meta[2].tolist())
    for bad in ([[0, 0, 4]], [[0, 4, 0]], [[0, 16385, 1]], [[0, 1, 16385]], [[-16, 2, 2]], [[packed.numel() - 11, 2, 2]]):
        with pytest.raises(ValueError):
            trainer.DeviceResize.records(torch.tensor(bad), packed.numel())
    with pytest.raises(ValueError):
        trainer.DeviceResize.records(torch.zeros(3, 2, dtype=torch.int64), 100)
    assert trainer.DeviceResize().size == (256, 256) and trainer.DeviceResize((56, 48)).size == (56, 48)
    for size in (256, (0, 8), (8, 16385), (8,)):
        with pytest.raises(ValueError):
            trainer.DeviceResize(size)


def test_train_refuses_device_resize_without_device_collate_or_with_a_bad_size():
    data = torch.utils.data.TensorDataset(torch.zeros(4, 32, 32, 3, dtype=torch.uint8), torch.randint(0, 10, (4,)))
    sgd = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    for kw in (dict(device_resize=(24, 24)), dict(device_resize=(24, 24), device_collate=True)):       # a CPU run
        with pytest.raises(ValueError):
            trainer.train(torch.nn.Linear(4, 4), sgd, use_gpu=False, dataset=data, epochs=1, batch_size=2, num_classes=10, **kw)
    for kw in (dict(device_resize=(24, 24)), dict(device_resize=(24, 24), device_augment=True),
               dict(device_resize=(0, 24), device_collate=True), dict(device_resize=24, device_collate=True)):
        with pytest.raises(ValueError):
            trainer.train(torch.nn.Linear(4, 4), "fused", use_gpu=True, dataset=data, epochs=1, batch_size=2, num_classes=10, **kw)
    assert not torch.distributed.is_initialized()


# ---- the C boundary -------------------------------------------------------------------------------------------------------
def test_resize_sample_layout_matches_the_header():
    fields = ("offset", "h", "w")
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "calm_vit.h"\nint main(void){printf("%zu", sizeof(calm_resize_sample));\n' + \
          "".join(f'printf(" %zu", offsetof(calm_resize_sample, {f}));\n' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == 16 == ctypes.sizeof(binding.ResizeSample) == trainer.DeviceResize.dtype().itemsize
    assert got[1:] == [getattr(binding.ResizeSample, f).offset for f in fields]
    assert got[1:] == [trainer.DeviceResize.dtype().fields[f][1] for f in fields]


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """On a host without a GPU: every call below is turned down by the argument checks, so the fake device addresses are
    never read and nothing is launched."""
    lib = binding.load()
    P = 0x7f0000010000
    valid = [P, 1 << 20, P, P, 4, 256, 256, None]
    assert len(valid) == len(binding.SIGNATURES["calm_resize_u8"][1])
    for change, code in (({0: None}, binding.E_INVAL), ({2: None}, binding.E_INVAL), ({3: None}, binding.E_INVAL),
                         ({1: 0}, binding.E_INVAL), ({1: -5}, binding.E_INVAL), ({4: 0}, binding.E_INVAL),
                         ({4: -1}, binding.E_INVAL), ({5: 0}, binding.E_INVAL), ({6: 0}, binding.E_INVAL),
                         ({6: -3}, binding.E_INVAL), ({4: 65536}, binding.E_UNSUPP), ({5: 16385}, binding.E_UNSUPP),
                         ({6: 16385}, binding.E_UNSUPP)):
        args = list(valid)
        for i, v in change.items():
            args[i] = v
        assert lib.calm_resize_u8(*args) == code, change
    bounds, kk = (ctypes.c_int32 * 16)(), (ctypes.c_int32 * 64)()
    assert lib.calm_resize_coeffs(20, 8, bounds, kk, 7) == 0                     # 2 ceil(2.5) + 1
    for args, code in (((20, 8, None, kk, 7), binding.E_INVAL), ((20, 8, bounds, None, 7), binding.E_INVAL),
                       ((0, 8, bounds, kk, 7), binding.E_INVAL), ((20, 0, bounds, kk, 7), binding.E_INVAL),
                       ((20, 8, bounds, kk, 0), binding.E_INVAL), ((20, 8, bounds, kk, 3), binding.E_INVAL),
                       ((16385, 8, bounds, kk, 7), binding.E_UNSUPP), ((20, 16385, bounds, kk, 7), binding.E_UNSUPP)):
        assert lib.calm_resize_coeffs(*args) == code, args
