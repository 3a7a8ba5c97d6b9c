"""Weight EMA without a GPU:
  * the float64 checker (tests/ema_f64.py) passes on the clean numpy emulation of the two launches (tests/emulated_ema.py)
    and flags every planted fault;
  * the C-ABI additions: header, binding and library agree on the three names, the ABI stays 7, sizeof(calm_ema_entry) is
    32 and equals the ctypes mirror, and every refusal is answered before any launch on a host with no GPU;
  * trainer.ModelEMA on CPU parameters (Tensor.lerp_ with the host-computed fp32 weight): the float64 recurrence, the
    warm-up weights, the swapped-in state, the state_dict round trip, model_state_dict's keys;
  * train(use_gpu=False, ema=0.9) on two gloo ranks: bit-identical averages on both ranks and the `_ema` checkpoint."""
import ctypes
import os
import re
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import calm_vit_dte_amd as calm  # noqa: E402
import ema_f64 as F  # noqa: E402
import emulated_ema as E  # noqa: E402
from test_host_logic_cpu import build_model  # noqa: E402
from importlib import import_module  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
HEADER = os.path.join(ROOT, "include", "calm_vit.h")
NAMES = ("calm_ema_chunk_elems", "calm_ema_update", "calm_ema_swap")


# ---- the checker on the emulation ------------------------------------------------------------------------------------------
def _emulated_update(decay, schedule, n, skip=None, fault=None):
    """One emulated calm_ema_update on a fresh table; returns what the checker needs."""
    be = E.EmulatedEmaBackend()
    be.ema_fault = fault
    pairs = F.make_table(E.CHUNK, "cpu")
    plan = be.ema_plan(pairs)
    assert plan.n == len(pairs) - 1                                  # the pair without elements has no entry
    plan.count_dev.fill_(n)
    before = [a.clone() for _, a in plan.pairs]
    be.ema_update(plan, decay, schedule, None if skip is None else torch.tensor([float(skip)]))
    return plan, before


def _check_applied(plan, before, decay, schedule, n):
    w = float(plan.weight_out[0])
    assert float(plan.weight_out[1]) == 0.0 and int(plan.count_dev) == n + 1
    F.check_weight(w, decay, schedule, n)
    for (src, ema), e0 in zip(plan.pairs, before):
        F.check_update(e0.numpy(), src.numpy(), ema.numpy(), w)


def _check_skipped(plan, before, n):
    assert plan.weight_out.tolist() == [0.0, 1.0] and int(plan.count_dev) == n
    for (_, ema), e0 in zip(plan.pairs, before):
        F.check_bits_equal(ema.numpy(), e0.numpy(), "average after a skipped update")


@pytest.mark.parametrize("decay,schedule,n", [(0.999, F.EMA_CONSTANT, 0), (0.9999, F.EMA_WARMUP, 0), (0.9999, F.EMA_WARMUP, 57)])
def test_checker_passes_on_the_clean_emulation(decay, schedule, n):
    plan, before = _emulated_update(decay, schedule, n)
    _check_applied(plan, before, decay, schedule, n)
    plan, before = _emulated_update(decay, schedule, n, skip=1)
    _check_skipped(plan, before, n)
    plan, before = _emulated_update(decay, schedule, n, skip=0)      # a skip scalar of 0 is an ordinary update
    _check_applied(plan, before, decay, schedule, n)


@pytest.mark.parametrize("fault", ["count+1", "tail", "boundary"])
def test_checker_flags_a_planted_update_fault(fault):
    plan, before = _emulated_update(0.9999, F.EMA_WARMUP, 0, fault=fault)
    with pytest.raises(AssertionError):
        _check_applied(plan, before, 0.9999, F.EMA_WARMUP, 0)


def test_checker_flags_an_update_applied_despite_skip():
    plan, before = _emulated_update(0.999, F.EMA_CONSTANT, 3, skip=1, fault="skip")
    with pytest.raises(AssertionError):
        _check_skipped(plan, before, 3)


def test_checker_on_the_emulated_swap_and_its_planted_fault():
    for fault in (None, "one-way"):
        be = E.EmulatedEmaBackend()
        be.ema_fault = fault
        plan = be.ema_plan(F.make_table(E.CHUNK, "cpu"))
        nan = torch.tensor([0x7fc00001, -0x3edcba, 0x7f800001], dtype=torch.int32).view(torch.float32)    # NaN payloads
        plan.pairs[4][0][:3] = nan
        plan.pairs[-1][1][5:8] = nan
        before = [(s.clone(), a.clone()) for s, a in plan.pairs]
        be.ema_swap(plan)

        def check():
            for (s, a), (s0, a0) in zip(plan.pairs, before):
                F.check_swap(s0.numpy(), a0.numpy(), s.numpy(), a.numpy())
        if fault is None:
            check()
            be.ema_swap(plan)                                        # two swaps are the identity
            for (s, a), (s0, a0) in zip(plan.pairs, before):
                F.check_bits_equal(s.numpy(), s0.numpy(), "parameter after two swaps")
                F.check_bits_equal(a.numpy(), a0.numpy(), "average after two swaps")
        else:
            with pytest.raises(AssertionError):
                check()


def test_emulation_walks_vector_and_scalar_segments_like_the_kernel():
    C = E.CHUNK
    assert E._segments(0, 0, 5) == [(0, 4, "vector"), (4, 5, "scalar")]
    assert E._segments(0, 0, 3) == [(0, 3, "scalar")]
    assert E._segments(0, 4, 9) == [(0, 9, "scalar")]                 # mixed alignment
    assert E._segments(4, 4, 9) == [(0, 9, "scalar")]                 # both one float in: no 16-byte aligned pair
    assert E._segments(64, 128, 2 * C + 7) == [(0, C, "vector"), (C, 2 * C, "vector"), (2 * C, 2 * C + 4, "vector"),
                                               (2 * C + 4, 2 * C + 7, "scalar")]


# ---- C-ABI -----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_ema_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^\s*(?:int|int32_t)\s+(calm_ema_\w+)\s*\(", text, flags=re.M))
    assert declared == set(NAMES)
    assert {n for n in binding.SIGNATURES if n.startswith("calm_ema_")} == set(NAMES)
    lib = binding.load()
    for n in NAMES:
        assert hasattr(lib, n), n
    assert int(re.search(r"#define\s+CALM_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 7
    assert lib.calm_abi_version() == 7 == binding.ABI_VERSION        # additions only
    assert (binding.EMA_CONSTANT, binding.EMA_WARMUP) == (0, 1)
    for name, value in (("CALM_EMA_CONSTANT", 0), ("CALM_EMA_WARMUP", 1)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", text).group(1)) == value
    chunk = int(lib.calm_ema_chunk_elems())
    assert chunk > 0 and chunk % 4 == 0 and chunk == E.CHUNK
    # outside the streaming-entry pattern list of tests/test_abi_cpu.py
    assert not any(re.match(r"calm_(layernorm|rope|softmax|sum_heads|latent|add$|gelu|colsum|row_scale|mean_seq|cnn_residual|"
                            r"soft_ce|huber|top1)", n) for n in NAMES)


def test_ema_entry_layout_matches_the_header():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "calm_vit.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", ' \
          'sizeof(calm_ema_entry), offsetof(calm_ema_entry, ema), offsetof(calm_ema_entry, numel), ' \
          'offsetof(calm_ema_entry, chunk0), offsetof(calm_ema_entry, reserved));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    M = binding.EmaEntry
    assert got == [32, 8, 16, 24, 28]
    assert got == [ctypes.sizeof(M), M.ema.offset, M.numel.offset, M.chunk0.offset, M.reserved.offset]
    assert np.dtype(M).itemsize == 32


_P = 0x7f0000010000          # a fake, 16-byte aligned device address: every call below is refused before any launch
_UPDATE = [_P, 3, _P, 5, 0.999, 0, _P, None, _P, None]
_SWAP = [_P, 3, _P, 5, None]
_REFUSED = [
    ("calm_ema_update", {0: None}, "null entries_dev"), ("calm_ema_update", {2: None}, "null chunk_entry_dev"),
    ("calm_ema_update", {6: None}, "null count_dev"), ("calm_ema_update", {8: None}, "null weight_out"),
    ("calm_ema_update", {1: 0}, "n_entries 0"), ("calm_ema_update", {1: -2}, "n_entries negative"),
    ("calm_ema_update", {3: 0}, "n_chunks 0"), ("calm_ema_update", {3: -1}, "n_chunks negative"),
    ("calm_ema_update", {4: 1.0}, "decay 1"), ("calm_ema_update", {4: 1.5}, "decay above 1"),
    ("calm_ema_update", {4: -1e-3}, "decay negative"), ("calm_ema_update", {4: float("nan")}, "decay NaN"),
    ("calm_ema_update", {4: float("inf")}, "decay inf"),
    ("calm_ema_update", {5: 2}, "schedule 2"), ("calm_ema_update", {5: -1}, "schedule negative"),
    ("calm_ema_swap", {0: None}, "null entries_dev"), ("calm_ema_swap", {2: None}, "null chunk_entry_dev"),
    ("calm_ema_swap", {1: 0}, "n_entries 0"), ("calm_ema_swap", {3: 0}, "n_chunks 0"), ("calm_ema_swap", {3: -7}, "n_chunks negative"),
]


@pytest.mark.parametrize("name,change,what", _REFUSED, ids=[f"{n[9:]}-{w}" for n, _, w in _REFUSED])
def test_ema_entry_points_refuse_bad_arguments_before_any_launch(name, change, what):
    lib = binding.load()
    args = list(_UPDATE if name == "calm_ema_update" else _SWAP)
    assert len(args) == len(binding.SIGNATURES[name][1])
    for i, v in change.items():
        args[i] = v
    assert getattr(lib, name)(*args) == binding.E_INVAL, what


# ---- ModelEMA on CPU parameters ------------------------------------------------------------------------------------------------
def _cpu_model(seed=0):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.LayerNorm(19), torch.nn.Linear(19, 5))
    m.register_buffer("steps_seen", torch.zeros(3))
    return m


def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.05)


@pytest.mark.parametrize("warmup", [True, False])
def test_model_ema_on_cpu_follows_the_float64_recurrence(warmup):
    m = _cpu_model()
    decay = 0.99
    ema = trainer.ModelEMA(m, decay=decay, warmup=warmup)
    schedule = F.EMA_WARMUP if warmup else F.EMA_CONSTANT
    for (n, p), s in zip(m.named_parameters(), ema.shadows):
        assert torch.equal(s, p) and s.data_ptr() != p.data_ptr() and s.dtype == torch.float32, n
    for step in range(5):
        _perturb(m, step)
        before = [s.clone() for s in ema.shadows]
        w = trainer.ema_weight(decay, schedule, step)
        F.check_weight(w, decay, schedule, step)
        ema.update()
        assert ema.num_updates == step + 1
        for p, s, e0 in zip(m.parameters(), ema.shadows, before):      # per step, from its own previous state
            F.check_update(e0.numpy(), p.detach().numpy(), s.numpy(), w)
    skipped = [s.clone() for s in ema.shadows]
    ema.update(skip=torch.ones(1))
    assert ema.num_updates == 5 and all(torch.equal(a, b) for a, b in zip(skipped, ema.shadows))
    ema.update(skip=torch.zeros(1))
    assert ema.num_updates == 6


def test_warmup_weight_sequence_is_the_fp32_formula():
    f = np.float32
    for decay in (0.9999, 0.5, 0.0):
        for n in range(31):
            d = min(f(decay), (f(1) + f(n)) / (f(10) + f(n)))
            want = f(1) - d
            got = trainer.ema_weight(decay, binding.EMA_WARMUP, n)
            assert f(got) == want and got == float(want), (decay, n)
            F.check_weight(got, decay, F.EMA_WARMUP, n)
            assert trainer.ema_weight(decay, binding.EMA_CONSTANT, n) == float(f(1) - f(decay))
    assert trainer.ema_weight(0.9999, binding.EMA_WARMUP, 0) == float(f(1) - f(1) / f(10))       # d = 0.1 at the start
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            trainer.ModelEMA(_cpu_model(), decay=bad)


def test_model_ema_swap_applied_and_refusals():
    m = _cpu_model()
    ema = trainer.ModelEMA(m, decay=0.9, warmup=False)
    _perturb(m, 1)
    ema.update()
    live = [p.detach().clone() for p in m.parameters()]
    avg = [s.clone() for s in ema.shadows]
    ptrs = [p.data_ptr() for p in m.parameters()]
    assert not ema.is_swapped
    with ema.applied() as inner:
        assert inner is m and ema.is_swapped
        assert [p.data_ptr() for p in m.parameters()] == ptrs           # contents exchanged, addresses kept
        for p, a, s, l in zip(m.parameters(), avg, ema.shadows, live):
            F.check_bits_equal(p.detach().numpy(), a.numpy(), "parameter inside applied()")
            F.check_bits_equal(s.numpy(), l.numpy(), "shadow inside applied()")
        for refused in (ema.update, ema.state_dict, ema.model_state_dict, ema.rebind):
            with pytest.raises(RuntimeError, match="swapped"):
                refused()
    assert not ema.is_swapped
    with pytest.raises(ZeroDivisionError):
        with ema.applied():
            1 / 0
    assert not ema.is_swapped                                           # swapped back although the block raised
    for p, l, s, a in zip(m.parameters(), live, ema.shadows, avg):
        assert torch.equal(p, l) and torch.equal(s, a)
    m[0].weight.data = m[0].weight.data.clone()                         # a re-materialised parameter
    with pytest.raises(RuntimeError, match="moved or replaced"):
        ema.update()
    ema.rebind()
    ema.update()
    assert ema.num_updates == 2
    with pytest.raises(TypeError):
        trainer.ModelEMA(_cpu_model().half())


def test_model_ema_state_dict_round_trip_and_model_state_dict():
    m = _cpu_model()
    ema = trainer.ModelEMA(m, decay=0.97, warmup=True)
    for step in range(3):
        _perturb(m, step)
        ema.update()
    sd = ema.state_dict()
    assert sd["decay"] == 0.97 and sd["warmup"] is True and sd["num_updates"] == 3
    assert list(sd["shadow"]) == [n for n, _ in m.named_parameters()]
    other = trainer.ModelEMA(_cpu_model(seed=9), decay=0.5, warmup=False)
    other.load_state_dict(sd)
    assert other.decay == 0.97 and other.schedule == binding.EMA_WARMUP and other.num_updates == 3
    for a, b in zip(ema.shadows, other.shadows):
        assert torch.equal(a, b)
    again = other.state_dict()
    assert all(torch.equal(sd["shadow"][k], again["shadow"][k]) for k in sd["shadow"]) and again["num_updates"] == 3
    with pytest.raises(KeyError):
        other.load_state_dict({**sd, "shadow": {k: v for k, v in sd["shadow"].items() if k != "0.bias"}})
    with pytest.raises(ValueError):
        other.load_state_dict({**sd, "shadow": {**sd["shadow"], "0.bias": torch.zeros(7)}})
    msd = ema.model_state_dict()
    assert list(msd) == list(m.state_dict())                            # the model's keys, buffers included
    for n, s in zip(ema.names, ema.shadows):
        assert torch.equal(msd[n], s) and msd[n].data_ptr() != s.data_ptr()
    assert torch.equal(msd["steps_seen"], m.steps_seen)                 # buffers are the model's, not averaged
    fresh = _cpu_model(seed=3)
    fresh.load_state_dict(msd)
    assert all(torch.equal(p, s) for p, s in zip(fresh.parameters(), ema.shadows))


def test_train_step_updates_the_average_behind_the_optimizer_step():
    m = build_model("tiny32_cls", None).train()
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(4, 3, 32, 32, generator=g), torch.softmax(torch.randn(4, 10, generator=g), 1)
    with calm.backend.use_backend(E.EmulatedEmaBackend()):
        ema = trainer.ModelEMA(m, decay=0.9, warmup=True)
        step = trainer.TrainStep(m, trainer.make_optimizer(m), ema=ema)
        for n in range(2):
            before = [s.clone() for s in ema.shadows]
            step(x, y)
            w = trainer.ema_weight(0.9, binding.EMA_WARMUP, n)
            for p, s, e0 in zip(m.parameters(), ema.shadows, before):  # the parameters AFTER the optimizer step
                F.check_update(e0.numpy(), p.detach().numpy(), s.numpy(), w)
        assert ema.num_updates == 2
        with pytest.raises(ValueError):
            trainer.evaluate(m, [], ema=trainer.ModelEMA(build_model("tiny32_cls", None)))
        labels = torch.zeros(4, dtype=torch.int64)
        live = [p.detach().clone() for p in m.parameters()]
        acc = trainer.evaluate(m, [(x, labels)], ema=ema)
        assert 0.0 <= acc <= 1.0 and not ema.is_swapped
        assert all(torch.equal(p, l) for p, l in zip(m.parameters(), live))


# ---- train() on two gloo ranks -------------------------------------------------------------------------------------------------
class _TinySet(torch.utils.data.Dataset):
    def __init__(self, n=16):
        g = torch.Generator().manual_seed(7)
        self.x = torch.randn(n, 3, 32, 32, generator=g)
        self.y = torch.randint(0, 10, (n,), generator=g)

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return self.x[i], int(self.y[i])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _train_worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    torch.manual_seed(50 + rank)                          # ranks start different: the average is built after the broadcast
    m = build_model("tiny32_cls", None).train()
    with calm.backend.use_backend(E.EmulatedEmaBackend()):
        out = trainer.train(m, trainer.make_optimizer(m), None, use_gpu=False, dataset=_TinySet(), epochs=1, batch_size=4,
                            num_classes=10, checkpoint_path=os.path.join(outdir, "models", "model_cls.pth"), log_every=1000,
                            ema=0.9)
    ema = out._calm_ema
    torch.save({"shadow": ema.state_dict(), "live": out.state_dict(), "msd": ema.model_state_dict()},
               os.path.join(outdir, f"rank{rank}.pt"))


@pytest.mark.timeout(600)
def test_train_with_ema_on_two_gloo_ranks(tmp_path):
    mp.spawn(_train_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(os.path.join(tmp_path, "rank0.pt"))
    r1 = torch.load(os.path.join(tmp_path, "rank1.pt"))
    assert r0["shadow"]["num_updates"] == r1["shadow"]["num_updates"] == 2          # 16 samples / 2 ranks / batch 4
    assert r0["shadow"]["decay"] == 0.9 and r0["shadow"]["warmup"] is True
    moved = 0
    for k, v in r0["shadow"]["shadow"].items():
        F.check_bits_equal(v.numpy(), r1["shadow"]["shadow"][k].numpy(), f"average of {k} on the two ranks")
        moved += int(not torch.equal(v, r0["live"][k]))
    assert moved > 0                                       # an average, not a copy of the live weights
    ck = torch.load(os.path.join(tmp_path, "models", "model_cls_ema.pth"))
    live_ck = torch.load(os.path.join(tmp_path, "models", "model_cls.pth"))
    assert list(ck) == list(live_ck) == list(r0["live"])    # the reference's keys
    for k in ck:
        assert torch.equal(ck[k], r0["msd"][k]), k         # written after the epoch's last step
    with pytest.raises(ValueError):
        trainer.train(torch.nn.Linear(4, 4), torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1), use_gpu=False,
                      dataset=_TinySet(), epochs=1, batch_size=2, num_classes=10, ema={"decay": 0.9, "every": 2})
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
