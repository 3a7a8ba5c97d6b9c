"""Training snapshots on the MI355X: calm_snapshot_pack / _unpack byte for byte against the numpy emulation
(tests/emulated_snapshot.py) on a table that reaches every path of the kernels, trainer.TrainState through training steps
(in place, exact continuation, saving perturbs nothing), trainer.train() resumed exactly — eager and captured — and a file
written by the CPU path loaded under a captured Predictor.  All comparisons are bit-exact."""
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import emulated_snapshot as E
from helpers import CONFIGS, load_golden
from test_host_logic_cpu import build_model

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
backend = import_module("calm_vit_dte_amd.backend")
NAME = "nano48_cls"


@pytest.fixture
def deterministic_gemm():
    be = calm.backend.get_backend()
    prev = be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, 1)
    yield be
    be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, prev)


# ---- the kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("many", [0, 1100], ids=["every-path", "1100-more-entries"])
def test_pack_and_unpack_against_the_emulation(many):
    be = calm.backend.get_backend()
    chunk_bytes = int(be.lib.calm_snapshot_chunk_bytes())
    entries = E.make_table(chunk_bytes // 4, "cuda", seed=7 + many, many=many)
    plan = be.snapshot_plan([t for _, t in entries], [n for n, _ in entries])
    rows = E.live(entries, plan.offsets, plan.sizes)
    assert plan.n == len(rows) == len(entries) - 1 and (many == 0 or plan.n > 1024)
    offs, sizes = [r[2] for r in rows], [r[3] for r in rows]
    chunk0, chunk_entry = backend.snapshot_chunks(sizes, chunk_bytes)
    assert plan.n_chunks == len(chunk_entry) and plan.entries["chunk0"].tolist() == chunk0
    assert {t.data_ptr() % 16 for _, t, _, _ in rows} == {0, 4, 8, 12}          # both kinds of chunk are there
    before = [E.base_words(t) for _, t, _, _ in rows]
    want = E.emulate_pack([E.words(t) for _, t, _, _ in rows], offs, sizes, chunk0, chunk_entry, chunk_bytes,
                          np.full(plan.packed_bytes, E.SENTINEL, dtype=np.uint8))
    plan.packed.fill_(E.SENTINEL)
    be.snapshot_pack(plan)
    torch.cuda.synchronize()
    got = plan.packed.cpu().numpy()
    mask = E.payload_mask(offs, sizes, plan.packed_bytes)
    assert np.array_equal(got[mask], want[mask])                                # every payload byte
    assert (got[~mask] == E.SENTINEL).all() and (~mask).any()                   # the padding keeps the sentinel
    for (_, t, _, _), b0 in zip(rows, before):                                  # a pack writes no tensor
        assert np.array_equal(E.base_words(t), b0)
    for _, t, _, _ in rows:                                                     # scramble the tensors (not the guards)
        t.view(torch.int32).bitwise_xor_(0x5A5A5A5A)
    torch.cuda.synchronize()
    assert all(not np.array_equal(E.base_words(t), b0) for (_, t, _, _), b0 in zip(rows, before))
    be.snapshot_unpack(plan)
    torch.cuda.synchronize()
    for (n, t, _, _), b0 in zip(rows, before):                                  # bits back, guard words untouched
        assert np.array_equal(E.base_words(t), b0), n
    assert np.array_equal(plan.packed.cpu().numpy(), got)                       # an unpack writes no packed byte


def test_plan_refuses_what_the_kernels_cannot_take():
    be = calm.backend.get_backend()
    a = torch.zeros(8, 6, device="cuda")
    with pytest.raises(TypeError, match="contiguous"):
        be.snapshot_plan([a.t()])
    with pytest.raises(TypeError, match="CUDA"):
        be.snapshot_plan([a.cpu()])
    buf = torch.zeros(100, device="cuda")
    with pytest.raises(ValueError, match="overlap"):
        be.snapshot_plan([buf[:60], buf[40:]])
    with pytest.raises(ValueError, match="whole 4-byte words"):
        be.snapshot_plan([torch.zeros(3, dtype=torch.bfloat16, device="cuda")])
    with pytest.raises(ValueError, match="at least one"):
        be.snapshot_plan([torch.zeros(0, device="cuda")])


# ---- TrainState through training steps -------------------------------------------------------------------------------
def _batches(n, bs=4):
    cfg = CONFIGS[NAME]
    g = np.random.default_rng(5)
    out = []
    for _ in range(n):
        x = torch.from_numpy(g.standard_normal((bs, 3, cfg.seq_length, cfg.seq_length)).astype(np.float32))
        a, b = g.integers(0, cfg.out_features, bs), g.integers(0, cfg.out_features, bs)
        y = np.zeros((bs, cfg.out_features), dtype=np.float32)
        y[np.arange(bs), a] += 0.7
        y[np.arange(bs), b] += 0.3
        out.append((x.cuda(), torch.from_numpy(y).cuda()))
    return out


def _setup():
    torch.manual_seed(21)
    torch.cuda.manual_seed(21)
    m = build_model(NAME, load_golden(NAME), "cuda").train()
    opt = trainer.FusedClipAdamW(m)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    ema = trainer.ModelEMA(m, 0.99)
    step = trainer.TrainStep(m, opt, scaler=scaler, ema=ema)
    st = trainer.TrainState(m, opt, scaler=scaler, ema=ema, step=step)
    return m, opt, scaler, ema, step, st


def _everything(m, opt, scaler, ema, step):
    """Clones of the whole state, by name."""
    out = {"model." + k: v.clone() for k, v in m.state_dict().items()}
    out.update({f"exp_avg.{i}": t.clone() for i, t in enumerate(opt.exp_avg)})
    out.update({f"exp_avg_sq.{i}": t.clone() for i, t in enumerate(opt.exp_avg_sq)})
    out.update({"shadow." + n: s.clone() for n, s in zip(ema.names, ema.shadows)})
    out["step_count"] = torch.tensor(opt.step_count)
    out["num_updates"] = torch.tensor(ema.num_updates)
    out["scale"] = torch.tensor(scaler.get_scale())
    out["clean_steps"] = step._clean_steps.clone()
    return out


def _assert_equal(got, want, what):
    assert set(got) == set(want)
    bad = [k for k in want if not torch.equal(got[k].view(torch.int32) if got[k].dtype == torch.float32 else got[k],
                                              want[k].view(torch.int32) if want[k].dtype == torch.float32 else want[k])]
    assert not bad, (what, bad[:5])


def test_train_state_restores_in_place_and_the_run_continues_exactly(deterministic_gemm, tmp_path):
    path = str(tmp_path / "s.snap")
    data = _batches(5)
    m, opt, scaler, ema, step, st = _setup()
    try:
        for x, y in data[:3]:
            step(x, y)
        st.save_async(path, {"epoch": 0, "batch": 3, "step": 3})
        st.wait()
        at_save = _everything(m, opt, scaler, ema, step)
        rng_at_save = torch.cuda.get_rng_state()
        assert int(at_save["step_count"]) > 0 and int(at_save["num_updates"]) > 0
        ptrs = [t.data_ptr() for t in list(m.parameters()) + opt.exp_avg + opt.exp_avg_sq + ema.shadows]
        for x, y in data[3:]:
            step(x, y)
        after_five = _everything(m, opt, scaler, ema, step)
        assert not torch.equal(after_five["model.autoencoder.ln_final.weight"], at_save["model.autoencoder.ln_final.weight"])
        assert st.load(path) == {"epoch": 0, "batch": 3, "step": 3}
        _assert_equal(_everything(m, opt, scaler, ema, step), at_save, "state after load")
        assert torch.equal(torch.cuda.get_rng_state(), rng_at_save)
        assert ptrs == [t.data_ptr() for t in list(m.parameters()) + opt.exp_avg + opt.exp_avg_sq + ema.shadows]
        for x, y in data[3:]:
            step(x, y)
        _assert_equal(_everything(m, opt, scaler, ema, step), after_five, "steps 4 and 5 after the load")
        st.close()
    finally:
        opt.close()


def test_saving_behind_every_step_perturbs_nothing(deterministic_gemm, tmp_path):
    data = _batches(4)
    ends = []
    for save in (False, True):
        m, opt, scaler, ema, step, st = _setup()
        try:
            for i, (x, y) in enumerate(data):
                step(x, y)
                if save:
                    st.save_async(str(tmp_path / "p.snap"), {"epoch": 0, "batch": i + 1, "step": i + 1})
                st.poll()
            st.close()
            ends.append(_everything(m, opt, scaler, ema, step))
        finally:
            opt.close()
    _assert_equal(ends[1], ends[0], "four steps with a snapshot behind each")
    header, _ = trainer.TrainState.read_header(str(tmp_path / "p.snap"))
    assert header["host"]["progress"]["step"] == 4                   # the last one is the one in place


# ---- train(): exact resume -------------------------------------------------------------------------------------------
def _train(tmp, tag, seed, graph=False, name=NAME, **kw):
    cfg = CONFIGS[name]
    S = cfg.seq_length
    gen = torch.Generator().manual_seed(0)
    data = torch.utils.data.TensorDataset(torch.randint(0, 256, (32, 3, S + 4, S + 4), generator=gen, dtype=torch.uint8),
                                          torch.randint(0, cfg.out_features, (32,), generator=gen))
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    m = build_model(name, load_golden(name), "cpu")
    if seed != 11:                                  # a resumed run starts from other weights: only the load can make it equal
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(1.01)
    path = str(tmp / f"{tag}.snap")
    out = trainer.train(m, "fused", scheduler=None, use_gpu=True, dataset=data, epochs=2, batch_size=8,
                        num_classes=cfg.out_features, device_collate=True, device_augment=True, crop=(S, S), ema=0.99,
                        log_every=1000, graph=graph, snapshot_path=path, **kw)
    return out, path


def _parts(path):
    header, start = trainer.TrainState.read_header(path)
    raw = open(path, "rb").read()
    return header, raw[start:start + header["packed_bytes"]]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Run A (uninterrupted) eager and captured, run B (stopped after 3 steps with a snapshot), shared by the cases."""
    tmp = tmp_path_factory.mktemp("resume")
    be = calm.backend.get_backend()
    prev = be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, 1)
    try:
        made = {"tmp": tmp, "A": _train(tmp, "a", 11), "B": _train(tmp, "b", 11, max_steps=3, snapshot_every=3)}
        yield made
    finally:
        be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, prev)


def _assert_same_run(a, c, file_a, file_c):
    sa, sc = a.state_dict(), c.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sc[k]), f"resumed run differs at {k}"
    for n, x, y in zip(a._calm_ema.names, a._calm_ema.shadows, c._calm_ema.shadows):
        assert torch.equal(x, y), f"resumed average differs at {n}"
    (ha, pa), (hc, pc) = _parts(file_a), _parts(file_c)
    assert ha["entries"] == hc["entries"]
    assert pa == pc and ha["crc32"] == hc["crc32"]                   # payload bytes
    assert ha["host"] == hc["host"], [k for k in ha["host"] if ha["host"][k] != hc["host"].get(k)]


@pytest.mark.parametrize("graph_a,graph_c", [(False, False), (False, True), (True, True)],
                         ids=["eager", "resumed-captured", "both-captured"])
def test_train_resumes_exactly(runs, graph_a, graph_c):
    tmp = runs["tmp"]
    header_b = trainer.TrainState.read_header(runs["B"][1])[0]
    assert header_b["host"]["progress"] == {"epoch": 0, "batch": 3, "step": 3}
    assert sorted(header_b["host"]["generators"]) == ["augment", "collate"]
    if graph_a and "A_graph" not in runs:
        runs["A_graph"] = _train(tmp, "a_graph", 11, graph=True)
    a, file_a = runs["A_graph" if graph_a else "A"]
    c, file_c = _train(tmp, f"c_{int(graph_a)}{int(graph_c)}", 12, graph=graph_c, resume=runs["B"][1])
    assert trainer.TrainState.read_header(file_c)[0]["host"]["progress"] == {"epoch": 2, "batch": 0, "step": 8}
    _assert_same_run(a, c, file_a, file_c)


def test_resume_into_another_model_names_the_first_differing_entry(runs):
    with pytest.raises(ValueError, match=r"entry .*model\.\S+ .*in the file and .* in the live state"):
        _train(runs["tmp"], "other", 11, name="tiny32_cls", resume=runs["B"][1])


# ---- a CPU file under a captured step --------------------------------------------------------------------------------
def test_cpu_file_loads_on_the_gpu_and_a_captured_predictor_sees_it(tmp_path):
    g = load_golden(NAME)
    path = str(tmp_path / "cpu.snap")
    cpu = build_model(NAME, g, "cpu").train()
    with torch.no_grad():
        gen = torch.Generator().manual_seed(3)
        for p in cpu.parameters():
            p.add_(torch.randn(p.shape, generator=gen) * 0.02 * p.abs().mean())
    st_cpu = trainer.TrainState(cpu, trainer.make_optimizer(cpu))
    st_cpu.save_async(path, {"epoch": 4, "batch": 0, "step": 40})
    st_cpu.close()
    want_model = build_model(NAME, g, "cuda")
    want_model.load_state_dict(cpu.state_dict())
    xs = torch.from_numpy(np.random.default_rng(1).standard_normal((4, 3, 48, 48)).astype(np.float32)).cuda()
    with torch.no_grad():
        want = want_model.eval()(xs)[0].reshape(4, -1).clone()
    m = build_model(NAME, g, "cuda").train()
    pred = trainer.Predictor(m, example_x=xs, graph=True)
    try:
        assert pred.graph is not None
        assert not torch.equal(pred(xs)[0].reshape(4, -1), want)
        st = trainer.TrainState(m, trainer.make_optimizer(m))
        ptrs = [p.data_ptr() for p in m.parameters()]
        assert st.load(path) == {"epoch": 4, "batch": 0, "step": 40}
        assert ptrs == [p.data_ptr() for p in m.parameters()]
        assert torch.equal(pred(xs)[0].reshape(4, -1), want)         # no re-capture: the replay reads the loaded weights
        back = str(tmp_path / "gpu.snap")                            # ... and the GPU writes the bytes the CPU wrote
        st.save_async(back, {"epoch": 4, "batch": 0, "step": 40})
        st.close()
        (h0, p0), (h1, p1) = _parts(path), _parts(back)
        assert h0["entries"] == h1["entries"] and p0 == p1 and h0["crc32"] == h1["crc32"]
    finally:
        pred.close()
