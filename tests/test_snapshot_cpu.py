"""Training snapshots without a GPU: the packed layout and the chunk table against the numpy emulation of the kernels
(tests/emulated_snapshot.py), the C-ABI additions (struct size, names, what is refused before a launch), the file format
and its refusals on a CPU model, RNG / generator state through JSON, the sampler tail of a resumed epoch, and exact resume
of trainer.train() on the gloo path — in one process and on two ranks with sidecars.  All comparisons are bit-exact."""
import ctypes
import json
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
import emulated_snapshot as E  # noqa: E402
from emulated_backend import EmulatedBackend  # noqa: E402
from test_host_logic_cpu import build_model  # noqa: E402
from importlib import import_module  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
backend = import_module("calm_vit_dte_amd.backend")
binding = import_module("calm_vit_dte_amd._lib")
HEADER = os.path.join(ROOT, "include", "calm_vit.h")
NAMES = ["calm_snapshot_chunk_bytes", "calm_snapshot_pack", "calm_snapshot_unpack"]


# ---- layout and chunk table ------------------------------------------------------------------------------------------
def test_layout_and_chunk_table_against_the_emulation():
    lib = binding.load()
    chunk_bytes = int(lib.calm_snapshot_chunk_bytes())
    assert chunk_bytes > 0 and chunk_bytes % 16 == 0
    C = chunk_bytes // 4
    entries = E.make_table(C, "cpu", seed=3)
    offsets, sizes, total = backend.snapshot_layout([(n, t.dtype, tuple(t.shape)) for n, t in entries])
    assert [nb // 4 for nb in sizes if nb] == [n for n in E.sizes_in_words(C) for _ in range(4)]
    assert all(off % 16 == 0 for off in offsets) and total % 16 == 0
    spans = sorted((off, off + nb) for off, nb in zip(offsets, sizes) if nb)
    assert all(b[0] >= a[1] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= total     # never overlap
    assert offsets == sorted(offsets)                                                       # the given order
    k = [n for n, _ in entries].index("empty")
    assert sizes[k] == 0                                                                    # no room for an empty tensor
    rows = E.live(entries, offsets, sizes)
    assert "empty" not in [r[0] for r in rows]
    chunk0, chunk_entry = backend.snapshot_chunks([r[3] for r in rows], chunk_bytes)
    assert len(chunk_entry) == sum(-(-r[3] // chunk_bytes) for r in rows)
    assert [chunk_entry.index(i) for i in range(len(rows))] == chunk0
    arrays = [E.words(r[1]) for r in rows]
    packed = np.full(total, E.SENTINEL, dtype=np.uint8)
    E.emulate_pack(arrays, [r[2] for r in rows], [r[3] for r in rows], chunk0, chunk_entry, chunk_bytes, packed)
    mask = E.payload_mask(offsets, sizes, total)
    assert (packed[~mask] == E.SENTINEL).all() and (~mask).any()                            # padding is never written
    for a, r in zip(arrays, rows):
        assert np.array_equal(packed[r[2]:r[2] + r[3]].view(np.uint32), a)
    back = E.emulate_unpack([np.zeros_like(a) for a in arrays], [r[2] for r in rows], [r[3] for r in rows], chunk0,
                            chunk_entry, chunk_bytes, packed)
    assert all(np.array_equal(a, b) for a, b in zip(arrays, back))
    with pytest.raises(ValueError, match="odd"):                                            # 6 bytes: not whole words
        backend.snapshot_layout([("ok", torch.float32, (4,)), ("odd", torch.bfloat16, (3,))])


def test_struct_size_and_names_agree_between_header_library_and_binding():
    src = '#include <stdio.h>\n#include "calm_vit.h"\nint main(void){printf("%zu\\n", sizeof(calm_snapshot_entry));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        size = int(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert size == 32 == ctypes.sizeof(binding.SnapshotEntry)
    assert np.dtype(binding.SnapshotEntry).itemsize == 32
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"^\s*(?:int|int32_t)\s+(calm_snapshot_\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == NAMES
    lib = binding.load()
    assert all(hasattr(lib, n) for n in NAMES)
    assert sorted(n for n in binding.SIGNATURES if n.startswith("calm_snapshot_")) == NAMES
    assert int(re.search(r"#define\s+CALM_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == binding.ABI_VERSION == 7


def test_pack_and_unpack_refuse_bad_arguments_before_any_launch():
    """No call below is a valid one, so nothing is launched and no address is read."""
    lib = binding.load()
    P = 0x7f0000010000
    valid = [P, 3, P, 5, P, 4096, None]
    for fn in (lib.calm_snapshot_pack, lib.calm_snapshot_unpack):
        for i in (0, 2, 4):                                         # one null pointer at a time
            args = list(valid)
            args[i] = None
            assert fn(*args) == binding.E_INVAL, (i,)
        for i, v in ((1, 0), (1, -1), (3, 0), (3, -7), (5, 0), (5, -16)):
            args = list(valid)
            args[i] = v
            assert fn(*args) == binding.E_INVAL, (i, v)


# ---- the file --------------------------------------------------------------------------------------------------------
def _batch(seed=0, B=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 32, 32, generator=g), torch.softmax(torch.randn(B, 10, generator=g), 1)


def _cpu_state(seed):
    torch.manual_seed(seed)
    m = build_model("tiny32_cls", None).train()
    opt = trainer.make_optimizer(m)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=5, eta_min=1e-6)
    scaler = torch.amp.GradScaler("cuda", enabled=False)
    step = trainer.TrainStep(m, opt)
    gen = np.random.default_rng(5)
    st = trainer.TrainState(m, opt, scaler=scaler, scheduler=sched, step=step, generators={"g": gen})
    return m, opt, sched, step, gen, st


def _optim_tensors(opt):
    return [v for s in opt.state_dict()["state"].values() for v in s.values() if isinstance(v, torch.Tensor)]


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """A CPU model with torch AdamW and a cosine schedule, three steps in, saved; what it held at the save."""
    d = tmp_path_factory.mktemp("snap")
    path = str(d / "state.snap")
    x, y = _batch()
    with calm.backend.use_backend(EmulatedBackend()):
        m, opt, sched, step, gen, st = _cpu_state(1)
        for _ in range(3):
            step(x, y)
        sched.step()
        gen.random(3)
        st.save_async(path, {"epoch": 1, "batch": 2, "step": 3})
        st.wait()
        want = {"sd": {k: v.clone() for k, v in m.state_dict().items()}, "optim": [t.clone() for t in _optim_tensors(opt)],
                "lr": opt.param_groups[0]["lr"], "sched": sched.state_dict(), "gen": gen.bit_generator.state,
                "rng": torch.get_rng_state().clone()}
        for _ in range(2):                                          # what the run does next
            step(x, y)
        want["next_sd"] = {k: v.clone() for k, v in m.state_dict().items()}
        want["next_draw"] = gen.random(4)
        st.close()
    return path, want


def test_file_round_trip_on_a_cpu_model(saved):
    path, want = saved
    x, y = _batch()
    raw = open(path, "rb").read()
    assert raw[:8] == trainer.TrainState.MAGIC
    hlen = int.from_bytes(raw[8:16], "little")
    header = json.loads(raw[16:16 + hlen])
    start = -(-(16 + hlen) // 4096) * 4096
    assert len(raw) == start + header["packed_bytes"] and not any(raw[16 + hlen:start])
    assert header["version"] == 1 and header["host"]["progress"] == {"epoch": 1, "batch": 2, "step": 3}
    names = [e["name"] for e in header["entries"]]
    assert names[0].startswith("model.") and any(n.startswith("optim.state.0.") for n in names)
    assert all(e["offset"] % 16 == 0 for e in header["entries"])
    with calm.backend.use_backend(EmulatedBackend()):
        m, opt, sched, step, gen, st = _cpu_state(2)               # another initialisation, another generator position
        gen.random(11)
        ptrs = [p.data_ptr() for p in m.parameters()]
        assert st.load(path) == {"epoch": 1, "batch": 2, "step": 3}
        assert ptrs == [p.data_ptr() for p in m.parameters()]      # in place
        sd = m.state_dict()
        assert all(torch.equal(sd[k].view(torch.int32), want["sd"][k].view(torch.int32)) for k in want["sd"])
        got = _optim_tensors(opt)
        assert len(got) == len(want["optim"]) and all(torch.equal(a, b) for a, b in zip(got, want["optim"]))
        assert opt.param_groups[0]["lr"] == want["lr"] and sched.state_dict() == want["sched"]
        assert gen.bit_generator.state == want["gen"] and torch.equal(torch.get_rng_state(), want["rng"])
        for _ in range(2):
            step(x, y)
        sd = m.state_dict()
        assert all(torch.equal(sd[k], want["next_sd"][k]) for k in sd)          # the trajectory continues exactly
        assert np.array_equal(gen.random(4), want["next_draw"])
        st.close()


def test_load_refuses_a_damaged_or_foreign_file_with_its_own_message(saved, tmp_path):
    path, _ = saved
    raw = open(path, "rb").read()
    hlen = int.from_bytes(raw[8:16], "little")
    header = json.loads(raw[16:16 + hlen])
    start = -(-(16 + hlen) // 4096) * 4096

    def rewritten(change):
        h = json.loads(raw[16:16 + hlen])
        change(h)
        text = json.dumps(h).encode()
        pad = -(16 + len(text)) % 4096
        return raw[:8] + len(text).to_bytes(8, "little") + text + b"\0" * pad + raw[start:]

    def rename(h):
        h["entries"][2]["name"] = "model.someone_else"

    def reshape(h):
        e = next(e for e in h["entries"] if len(e["shape"]) == 2)
        e["shape"] = [e["shape"][1], e["shape"][0] + 4]

    flipped = bytearray(raw)
    flipped[start + header["entries"][1]["offset"] + 1] ^= 0x10
    cases = [("truncated", raw[:len(raw) - 100], "short file"),
             ("flipped", bytes(flipped), "CRC32"),
             ("magic", b"NOTASNAP" + raw[8:], "not a training snapshot"),
             ("renamed", rewritten(rename), "model.someone_else in the file and " + header["entries"][2]["name"]),
             ("reshaped", rewritten(reshape), r"in the file and float32 \("),
             ("version", rewritten(lambda h: h.update(version=99)), "format version 99"),
             ("world", rewritten(lambda h: h["host"].update(world=4)), "world of 4 ranks")]
    with calm.backend.use_backend(EmulatedBackend()):
        m, opt, sched, step, gen, st = _cpu_state(3)
        before = {k: v.clone() for k, v in m.state_dict().items()}
        for name, data, message in cases:
            bad = str(tmp_path / (name + ".snap"))
            open(bad, "wb").write(data)
            with pytest.raises(ValueError, match=message):
                st.load(bad)
            sd = m.state_dict()
            assert all(torch.equal(sd[k], before[k]) for k in sd), name             # refused before a byte was scattered
        st.close()


def test_save_and_load_are_refused_while_the_ema_is_swapped_in(tmp_path):
    with calm.backend.use_backend(EmulatedBackend()):
        torch.manual_seed(4)
        m = build_model("tiny32_cls", None).train()
        opt = trainer.FusedClipAdamW(m)
        try:
            ema = trainer.ModelEMA(m, 0.99)
            st = trainer.TrainState(m, opt, ema=ema)
            path = str(tmp_path / "e.snap")
            st.save_async(path, {"epoch": 0, "batch": 0, "step": 0})
            st.wait()
            with ema.applied():
                with pytest.raises(RuntimeError, match="swapped"):
                    st.save_async(path, {"epoch": 0, "batch": 0, "step": 0})
                with pytest.raises(RuntimeError, match="swapped"):
                    st.load(path)
            assert st.load(path) == {"epoch": 0, "batch": 0, "step": 0}
            names = [e["name"] for e in trainer.TrainState.read_header(path)[0]["entries"]]
            assert "optim.step" in names and "ema.count" in names and "optim.exp_avg.0" in names
            st.close()
        finally:
            opt.close()


def test_a_step_without_the_growth_count_is_refused_where_the_state_needs_it(tmp_path):
    """Fused optimizer and an enabled scaler: `step.clean_steps` belongs to the file.  TrainStep makes the counter when it is
    built with that scaler; a step built without it is refused by name, not given one behind its back."""
    with calm.backend.use_backend(EmulatedBackend()):
        torch.manual_seed(4)
        m = build_model("tiny32_cls", None).train()
        opt = trainer.FusedClipAdamW(m)
        try:
            scaler = torch.amp.GradScaler("cpu")
            assert scaler.is_enabled()
            bare = trainer.RegTrainStep(m, opt)
            assert bare._clean_steps is None and bare._one is None
            with pytest.raises(ValueError, match="RegTrainStep keeps no GradScaler growth count"):
                trainer.TrainState(m, opt, scaler=scaler, step=bare)
            assert bare._clean_steps is None                        # no repair
            step = trainer.TrainStep(m, opt, scaler=scaler)
            assert step._clean_steps.dtype == torch.int32 and step._clean_steps.shape == () and step._one.shape == ()
            st = trainer.TrainState(m, opt, scaler=scaler, step=step)
            with pytest.raises(ValueError, match="RegTrainStep keeps no GradScaler growth count"):
                st.bind_step(bare)
            assert st.step is step                                  # the refused step was not bound
            path = str(tmp_path / "s.snap")
            st.save_async(path, {"epoch": 0, "batch": 0, "step": 0})
            st.wait()
            assert "step.clean_steps" in [e["name"] for e in trainer.TrainState.read_header(path)[0]["entries"]]
            st.close()
            st = trainer.TrainState(m, opt, step=bare)              # no scaler: nothing to keep, nothing to refuse
            st.close()
        finally:
            opt.close()


def test_generator_and_rng_states_round_trip_through_json():
    g = np.random.default_rng(2006)
    g.beta(0.8, 0.8, 5)
    torch.manual_seed(9)
    torch.randn(7)
    text = json.dumps({"g": g.bit_generator.state, "t": trainer._b64(torch.get_rng_state())})
    want_g, want_t = g.random(6), torch.randn(6)
    g2 = np.random.default_rng(1)
    torch.manual_seed(1)
    back = json.loads(text)
    g2.bit_generator.state = back["g"]
    torch.set_rng_state(trainer._unb64(back["t"]))
    assert np.array_equal(g2.random(6), want_g) and torch.equal(torch.randn(6), want_t)


# ---- the sampler tail ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2])
def test_resumed_epoch_yields_exactly_the_remaining_batches(world):
    from torch.utils.data import DataLoader, DistributedSampler
    data = torch.utils.data.TensorDataset(torch.arange(37))         # not a multiple of anything
    for rank in range(world):
        for epoch in (0, 3):
            sampler = DistributedSampler(data, num_replicas=world, rank=rank, shuffle=True, seed=2006)
            sampler.set_epoch(epoch)
            whole = [b[0].tolist() for b in DataLoader(data, batch_size=4, sampler=sampler)]
            for skip in (0, 1, 3, len(whole) - 1, len(whole)):
                tail = trainer.resume_tail(sampler, skip, 4)
                got = [b[0].tolist() for b in DataLoader(data, batch_size=4, sampler=tail)]
                assert got == whole[skip:], (rank, epoch, skip)
                assert len(DataLoader(data, batch_size=4, sampler=tail)) == len(whole) - skip


# ---- exact resume of train() on the gloo path ------------------------------------------------------------------------
class _TinySet(torch.utils.data.Dataset):
    def __init__(self, n):
        g = torch.Generator().manual_seed(7)
        self.x = torch.randn(n, 3, 32, 32, generator=g)
        self.y = torch.randint(0, 10, (n,), generator=g)

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return self.x[i], int(self.y[i])


def _run(optimizer_kind, n, seed=50, **kw):
    """train() on the CPU model the trainer tests train: 2 epochs of 4 steps, SoftMixCollate in the main process.  `seed`
    initialises the model (and leaves the torch generator wherever that ends): a resumed run is given another one, so it
    can equal the uninterrupted run only through what it loads."""
    torch.manual_seed(seed)
    m = build_model("tiny32_cls", None).train()
    with calm.backend.use_backend(EmulatedBackend()):
        opt = "fused" if optimizer_kind == "fused" else trainer.make_optimizer(m)
        out = trainer.train(m, opt, None, use_gpu=False, dataset=_TinySet(n), epochs=2, batch_size=4, num_classes=10,
                            collate_fn="mix", num_workers=0, log_every=1000, ema=0.99, **kw)
    return out


def _parts(path):
    header, start = trainer.TrainState.read_header(path)
    raw = open(path, "rb").read()
    return header, raw[start:start + header["packed_bytes"]]


def _assert_same_run(a, c, file_a, file_c, sidecars=()):
    sa, sc = a.state_dict() if hasattr(a, "state_dict") else a, c.state_dict() if hasattr(c, "state_dict") else c
    assert set(sa) == set(sc)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), f"resumed run differs at {k}"
    (ha, pa), (hc, pc) = _parts(file_a), _parts(file_c)
    assert pa == pc                                                   # payload bytes
    assert ha["entries"] == hc["entries"] and ha["crc32"] == hc["crc32"]
    assert ha["host"] == hc["host"]                                   # scheduler, lr, RNG, generators, progress
    for fa, fc in sidecars:
        assert json.load(open(fa)) == json.load(open(fc))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("optimizer_kind", ["adamw", "fused"])
def test_train_resumes_exactly_on_the_gloo_path(tmp_path, optimizer_kind):
    fa, fb, fc = (str(tmp_path / f"{n}.snap") for n in "abc")
    a = _run(optimizer_kind, 16, snapshot_path=fa)
    _run(optimizer_kind, 16, snapshot_path=fb, snapshot_every=3, max_steps=3)
    assert trainer.TrainState.read_header(fb)[0]["host"]["progress"] == {"epoch": 0, "batch": 3, "step": 3}
    c = _run(optimizer_kind, 16, seed=51, snapshot_path=fc, resume=fb)
    assert trainer.TrainState.read_header(fa)[0]["host"]["progress"] == {"epoch": 2, "batch": 0, "step": 8}
    _assert_same_run(a, c, fa, fc)
    for sa, sc in zip(a._calm_ema.shadows, c._calm_ema.shadows):
        assert torch.equal(sa, sc)
    assert a._calm_ema.num_updates == c._calm_ema.num_updates == 8


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _two_rank_worker(rank, world, ports, outdir):
    torch.set_num_threads(2)
    f = {n: os.path.join(outdir, f"{n}.snap") for n in "abc"}
    runs = [("a", dict(snapshot_path=f["a"])), ("b", dict(snapshot_path=f["b"], snapshot_every=3, max_steps=3)),
            ("c", dict(snapshot_path=f["c"], resume=f["b"], seed=51))]
    for (name, kw), port in zip(runs, ports):
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        out = _run("fused", 32, **kw)
        torch.save(out.state_dict(), os.path.join(outdir, f"{name}_rank{rank}.pt"))


@pytest.mark.timeout(600)
def test_train_resumes_exactly_on_two_gloo_ranks_with_sidecars(tmp_path):
    d = str(tmp_path)
    mp.spawn(_two_rank_worker, args=(2, [_free_port() for _ in range(3)], d), nprocs=2, join=True)
    fa, fc = os.path.join(d, "a.snap"), os.path.join(d, "c.snap")
    side = [(f"{fa}.rank{r}.json", f"{fc}.rank{r}.json") for r in range(2)]
    for r in range(2):
        a, c = torch.load(os.path.join(d, f"a_rank{r}.pt")), torch.load(os.path.join(d, f"c_rank{r}.pt"))
        _assert_same_run(a, c, fa, fc, side)
    s0, s1 = (json.load(open(fa + f".rank{r}.json")) for r in range(2))
    assert s0["rank"] == 0 and s1["rank"] == 1 and s0["generators"] != s1["generators"]     # each rank keeps its own
    assert "rng" not in trainer.TrainState.read_header(fa)[0]["host"]
