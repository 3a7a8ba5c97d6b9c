"""The k-NN probe without a GPU: the checker (tests/knn_f64.py) on the emulation of csrc/knn.hip (tests/emulated_knn.py), on its
fourteen planted faults and on the torch twins of trainer.py; the C-ABI surface (declared, exported, bound, every refusal on
fake addresses); ViT.features and Predictor(features=); KnnProbe's refusals, its report against tests/eval_f64.py on its own
score rows and against a float64 pipeline on a well-separated case; gather_bank and knn_evaluate on one and two gloo ranks;
train(knn=) on one and two gloo ranks against knn_evaluate by hand, with the parameters of the run without knn=."""
import ctypes
import json
import os
import re
import socket
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import calm_vit_dte_amd as calm
import emulated_knn as E
import eval_f64
import knn_f64 as F
from test_host_logic_cpu import build_model

trainer = import_module("calm_vit_dte_amd.trainer")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "calm_vit.h")
NEW = ("calm_knn_normalize", "calm_knn_merge", "calm_knn_vote")


@pytest.fixture(autouse=True)
def _restore():
    yield
    calm.backend.set_loss_kernels(False)


class EmuImpl:
    """The emulated backend behind the checker's interface."""

    def __init__(self, fault=None):
        self.be = E.EmulatedKnnBackend()
        self.be.knn_fault = fault

    def normalize(self, x, pad, lead):
        out, bad = torch.empty(x.shape, dtype=torch.float32), torch.zeros(1, dtype=torch.int64)
        self.be.knn_normalize(x, out, bad, x.shape[0], x.shape[1])
        return out, int(bad)

    def similarities(self, q, rows):
        return q @ rows.t()

    def merge(self, sims, base, best_sim, best_idx, pad, lead):
        s, i = best_sim.clone(), best_idx.clone()
        self.be.knn_merge(sims, base, s, i, sims.shape[0], sims.shape[1], s.shape[1])
        return s, i

    def vote(self, best_sim, best_idx, labels, inv_T, C):
        scores = torch.full((best_sim.shape[0], C), float("nan"))
        self.be.knn_vote(best_sim, best_idx, labels, inv_T, scores, best_sim.shape[0], best_sim.shape[1], C)
        return scores


class TorchImpl:
    """trainer.knn_*_torch behind the checker's interface."""

    def normalize(self, x, pad, lead):
        out, bad = trainer.knn_normalize_torch(x)
        return out, int(bad)

    def similarities(self, q, rows):
        return q @ rows.t()

    def merge(self, sims, base, best_sim, best_idx, pad, lead):
        s, i = best_sim.clone(), best_idx.clone()
        trainer.knn_merge_torch(sims, base, s, i)
        return s, i

    def vote(self, best_sim, best_idx, labels, inv_T, C):
        return trainer.knn_vote_torch(best_sim, best_idx, labels, inv_T, C)


# ---- the checker on the emulation, the twins and the planted faults -------------------------------------------------------------
@pytest.mark.parametrize("check", sorted(F.CHECKS))
@pytest.mark.parametrize("impl", [EmuImpl, TorchImpl], ids=["emulation", "twins"])
def test_healthy_implementations_pass_the_checker(impl, check):
    assert F.CHECKS[check](impl()) == []


@pytest.mark.parametrize("fault", E.FAULTS)
def test_every_planted_fault_is_caught_by_the_checks_it_concerns_and_by_no_other(fault):
    impl = EmuImpl(fault)
    caught = set()
    for name, check in F.CHECKS.items():
        found = check(impl, F.EXACT_CASES[:5]) if name == "exact" else check(impl)
        if found:
            caught.add(name)
            print(f"{fault}: {name}: {found[0]}")
    assert caught and caught <= E.CONCERNS[fault], (fault, caught)


# ---- the C-ABI surface --------------------------------------------------------------------------------------------------------
def test_the_three_names_are_declared_exported_and_bound_and_the_abi_is_still_7():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    binding = import_module("calm_vit_dte_amd._lib")
    lib = binding.load()
    for name in NEW:
        assert re.search(rf"^\s*int\s+{name}\s*\(", text, flags=re.M), name
        assert hasattr(lib, name) and name in binding.SIGNATURES
    assert lib.calm_abi_version() == binding.ABI_VERSION == 7
    assert int(re.search(r"#define\s+CALM_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 7
    for name in ("knn_normalize", "knn_merge", "knn_vote"):
        assert callable(getattr(calm.backend.HipBackend, name))


_P = 0x7f0000010000
_VALID = {
    "calm_knn_normalize": [_P, 144, 0, _P, _P, 8, 144, None],
    "calm_knn_merge": [_P, 1024, 0, _P, _P, 8, 1024, 20, None],
    "calm_knn_vote": [_P, _P, _P, 100, 1.0 / 0.07, _P, 10, 8, 20, 10, None],
}
_REQUIRED = {"calm_knn_normalize": (0, 3, 4), "calm_knn_merge": (0, 3, 4), "calm_knn_vote": (0, 1, 2, 5)}
_REFUSED = [
    ("calm_knn_normalize", {6: 0}, "E_INVAL", "D of 0"),
    ("calm_knn_normalize", {6: 4097, 1: 4097}, "E_UNSUPP", "D of 4097"),
    ("calm_knn_normalize", {2: 2}, "E_INVAL", "x_type fp8"),
    ("calm_knn_normalize", {2: -1}, "E_INVAL", "x_type negative"),
    ("calm_knn_normalize", {1: 143}, "E_INVAL", "ld below D"),
    ("calm_knn_normalize", {5: -1}, "E_INVAL", "N negative"),
    ("calm_knn_normalize", {0: _P + 2}, "E_LAYOUT", "x off its element"),
    ("calm_knn_merge", {7: 0}, "E_INVAL", "k of 0"),
    ("calm_knn_merge", {7: 257}, "E_UNSUPP", "k of 257"),
    ("calm_knn_merge", {6: 0}, "E_INVAL", "n of 0"),
    ("calm_knn_merge", {1: 1023}, "E_INVAL", "ld below n"),
    ("calm_knn_merge", {2: -1}, "E_INVAL", "base negative"),
    ("calm_knn_merge", {5: -1}, "E_INVAL", "Nq negative"),
    ("calm_knn_merge", {4: _P + 4}, "E_LAYOUT", "best_idx off its element"),
    ("calm_knn_vote", {8: 0}, "E_INVAL", "k of 0"),
    ("calm_knn_vote", {8: 257}, "E_UNSUPP", "k of 257"),
    ("calm_knn_vote", {9: 0}, "E_INVAL", "C of 0"),
    ("calm_knn_vote", {6: 9}, "E_INVAL", "ld below C"),
    ("calm_knn_vote", {4: 0.0}, "E_INVAL", "inv_T of 0"),
    ("calm_knn_vote", {4: float("inf")}, "E_INVAL", "inv_T infinite"),
    ("calm_knn_vote", {4: float("nan")}, "E_INVAL", "inv_T NaN"),
    ("calm_knn_vote", {3: -1}, "E_INVAL", "Nb negative"),
]


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """On fake addresses, on a host without a GPU: every call below has to be turned down by the argument checks, so no
    kernel is launched and nothing is dereferenced; an empty problem returns 0 without a launch."""
    binding = import_module("calm_vit_dte_amd._lib")
    lib = binding.load()
    for name, valid in _VALID.items():
        assert len(valid) == len(binding.SIGNATURES[name][1]), name
        for i in _REQUIRED[name]:
            args = list(valid)
            args[i] = None
            assert getattr(lib, name)(*args) == binding.E_INVAL, (name, "null pointer", i)
    for name, change, code, what in _REFUSED:
        args = list(_VALID[name])
        for i, v in change.items():
            args[i] = v
        assert getattr(lib, name)(*args) == getattr(binding, code), (name, what)
    for name, at in (("calm_knn_normalize", 5), ("calm_knn_merge", 5), ("calm_knn_vote", 7)):
        args = list(_VALID[name])
        args[at] = 0
        assert getattr(lib, name)(*args) == 0, (name, "empty")


# ---- ViT.features, Predictor(features=) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nano48_cls", "nano48_gen"])
def test_features_is_the_pooled_backbone_output_and_the_predictor_is_unchanged(name):
    with calm.backend.use_backend(E.EmulatedKnnBackend()):
        torch.manual_seed(5)
        m = build_model(name, None).eval()
        keys = list(m.state_dict())
        x = torch.randn(3, 3, 48, 48, generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            f = m.features(x)
            want = calm.ops.mean_seq(m.autoencoder(x)[0])
            y = m(x)
        assert tuple(f.shape) == (3, 144) and torch.equal(f, want)
        assert list(m.state_dict()) == keys and not hasattr(build_model("nano48_gen", None), "pool")
        m.train()
        plain = trainer.Predictor(m)(x)
        assert m.training and torch.equal(plain[0], y[0])                      # what it returned before
        feats = trainer.Predictor(m, features=True)(x)
        assert m.training and torch.equal(feats, f)


# ---- KnnProbe -----------------------------------------------------------------------------------------------------------------
def test_probe_refusals():
    for bad in (0, 257, -1, 2.5):
        with pytest.raises(ValueError, match="k is an integer within 1 .. 256"):
            trainer.KnnProbe(10, k=bad)
    for bad in (0.0, -0.07, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature is a positive finite number"):
            trainer.KnnProbe(10, temperature=bad)
    with pytest.raises(ValueError, match="chunk counts bank rows"):
        trainer.KnnProbe(10, chunk=0)
    with pytest.raises(ValueError, match="num_classes"):
        trainer.KnnProbe(0)
    p = trainer.KnnProbe(10, k=3)
    f, y = torch.randn(4, 8), torch.arange(4)
    with pytest.raises(ValueError, match="the bank is empty"):
        p.query(f, y)
    for bad in (y.int(), y[:3], y[:, None], [0, 1, 2, 3]):
        with pytest.raises(TypeError, match=r"labels is an int64 tensor \[N\]"):
            p.add_bank(f, bad)
    with pytest.raises(TypeError, match="floating-point tensor"):
        p.add_bank(f.long(), y)
    p.add_bank(f, y)
    with pytest.raises(ValueError, match="features are 9 wide, the probe has seen 8"):
        p.query(torch.randn(2, 9), torch.arange(2))
    with pytest.raises(TypeError, match=r"labels is an int64 tensor \[N\]"):
        p.query(f, y.float())
    with pytest.raises(ValueError, match="world_layout"):
        p.gather_bank(world_layout="blocked")
    p.reset()
    p.add_bank(torch.randn(2, 9), torch.arange(2))                                  # reset forgets the width


@pytest.mark.parametrize("emulated", [False, True], ids=["twins", "emulation"])
def test_report_is_the_eval_reference_on_the_probes_own_scores_and_a_small_bank_leaves_slots_empty(emulated):
    be = E.EmulatedKnnBackend() if emulated else None
    ctx = calm.backend.use_backend(be) if emulated else _null()
    bank, bl, q, ql = F.cluster_case(41, 300, 24, 7, 6.0)
    ql = ql.clone()
    ql[3], ql[5] = -100, 7                                                           # skipped labels
    bank[4], q[6] = 0.0, float("nan")                                                 # zeroed rows
    with ctx:
        p = trainer.KnnProbe(7, k=20, topk=(1, 3), chunk=128, confusion=True)
        p.add_bank(bank[:100], bl[:100])
        p.add_bank(bank[100:], bl[100:])
        scores = torch.cat([p.query(q[:17], ql[:17]), p.query(q[17:], ql[17:])])
        rep = p.read()
        if emulated:
            assert be.knn_calls > 6
        ref = eval_f64.reference(scores, ql, (1, 3))
        assert rep["n"] == int(ref["counts"][0]) == 39 and rep["skipped"] == 2
        assert rep["top1"] == int(ref["counts"][3]) / 39 and rep["top3"] == int(ref["counts"][4]) / 39
        assert torch.equal(rep["confusion"], torch.from_numpy(ref["confusion"]))
        assert (rep["bank"], rep["bank_zeroed"], rep["query_zeroed"], rep["k"], rep["temperature"]) == (300, 1, 1, 20, 0.07)
        assert set(rep) == {"n", "skipped", "bank", "bank_zeroed", "query_zeroed", "k", "temperature", "top1", "top3",
                            "per_class_accuracy", "mean_per_class_accuracy", "confusion"}
        assert 0.2 < rep["top1"] < 1.0                                               # (noise 6: hits and misses both occur)
        small = trainer.KnnProbe(7, k=8)
        small.add_bank(bank[:5], bl[:5])
        s, i = small.neighbours(q[:3])
        assert bool((i[:, 5:] == -1).all()) and bool((s[:, 5:] == float("-inf")).all()) and bool((i[:, :5] >= 0).all())
        votes = small.query(q[:3], ql[:3])
        assert bool(torch.isfinite(votes).all()) and bool((votes.sum(dim=1) > 0).all())


class _null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def test_well_separated_case_reports_what_the_float64_pipeline_reports():
    Nb, Nq, D, C, k, T = 5000, 257, 96, 10, 20, 0.07
    bank, bl, q, ql = F.cluster_case(Nq, Nb, D, C, 2.0)
    s64 = (F.unit64(q) @ F.unit64(bank).T).numpy()
    votes = np.zeros((Nq, C))
    for i in range(Nq):
        order = np.lexsort((np.arange(Nb), -s64[i]))[:k]
        np.add.at(votes[i], bl[order].numpy(), np.exp((s64[i, order] - s64[i, order[0]]) / T))
    srt = np.sort(votes, axis=1)
    assert (votes.argmax(axis=1) == ql.numpy()).all() and (srt[:, -1] - srt[:, -2]).min() > 1e-3   # no query is close
    ref = eval_f64.reference(torch.from_numpy(votes), ql, (1, 5))
    for be in (None, E.EmulatedKnnBackend()):
        with (calm.backend.use_backend(be) if be is not None else _null()):
            p = trainer.KnnProbe(C, k=k, temperature=T, chunk=2048, confusion=True)
            p.add_bank(bank, bl)
            p.query(q, ql)
            rep = p.read()
            assert eval_f64.mismatches(p.metrics.counts, p.metrics.confusion, ref, 2) == []
            assert rep["top1"] == 1.0 and rep["top5"] == 1.0 and rep["n"] == Nq and rep["mean_per_class_accuracy"] == 1.0


# ---- gather_bank and knn_evaluate on one and two gloo ranks -------------------------------------------------------------------
class _FeatSet(torch.utils.data.Dataset):
    """Samples whose `x` is their feature row: features= below is a deterministic per-sample function of it."""

    def __init__(self, n, seed, C=5, D=12):
        g = torch.Generator().manual_seed(seed)
        cent = torch.randn(C, D, generator=g) * 2
        self.y = torch.arange(n) % C
        self.x = (cent[self.y] + torch.randint(-2, 3, (n, D), generator=g).float() / 2)   # a coarse grid: ties occur

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return self.x[i], int(self.y[i])


def _shard_batches(data, rank, world, bs):
    shard = trainer.validation_shard(data, rank, world)
    return [(torch.stack([shard[i][0] for i in range(j, min(j + bs, len(shard)))]),
             torch.tensor([shard[i][1] for i in range(j, min(j + bs, len(shard)))], dtype=torch.int64))
            for j in range(0, len(shard), bs)]


def _feature(x):
    return x * 2.0 + x.roll(1, dims=1)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _join(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)


def _probe_run(rank, world, n_bank=37):
    """(bank, labels, neighbours of the whole query set, report) as rank `rank` of `world` sees them."""
    bank, queries = _FeatSet(n_bank, 3), _FeatSet(22, 4)
    group = torch.distributed.group.WORLD if world > 1 else None
    p = trainer.KnnProbe(5, k=6, chunk=16)
    for x, y in _shard_batches(bank, rank, world, 4):
        p.add_bank(_feature(x), y)
    p.gather_bank(group)
    for x, y in _shard_batches(queries, rank, world, 5):
        p.query(_feature(x), y)
    if world > 1:
        p.all_reduce(group)
    nb = p.neighbours(_feature(queries.x))
    rep = trainer.knn_evaluate(torch.nn.Linear(1, 1), _shard_batches(bank, rank, world, 4), _shard_batches(queries, rank, world, 5),
                               5, k=6, features=_feature, confusion=True)
    return dict(bank=p.bank(), nb=nb, rep=p.read(), rep_eval=rep)


def _probe_worker(rank, world, port, outdir):
    _join(rank, world, port)
    torch.distributed.init_process_group(backend="gloo")
    out = {n: _probe_run(rank, world, n) for n in (37, 38)}                    # unequal and equal shard lengths
    torch.save(out, os.path.join(outdir, f"probe{rank}.pt"))
    torch.distributed.destroy_process_group()


def _same_report(a, b):
    assert set(a) == set(b)
    for key in a:
        if isinstance(a[key], torch.Tensor):
            assert torch.equal(a[key].double().nan_to_num(nan=-1.0), b[key].double().nan_to_num(nan=-1.0)), key
        else:
            assert a[key] == b[key], key


@pytest.mark.timeout(600)
def test_bank_neighbours_and_report_do_not_depend_on_the_world_size(tmp_path):
    mp.spawn(_probe_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for n in (37, 38):
        one = _probe_run(0, 1, n)
        assert one["rep"]["n"] == 22 and one["rep"]["bank"] == n
        _same_report(one["rep"], {k: v for k, v in one["rep_eval"].items() if k != "confusion"})
        for rank in range(2):
            two = torch.load(os.path.join(tmp_path, f"probe{rank}.pt"))[n]
            assert torch.equal(two["bank"][0], one["bank"][0]) and torch.equal(two["bank"][1], one["bank"][1])
            assert torch.equal(two["nb"][1], one["nb"][1]) and torch.equal(F.bits(two["nb"][0]), F.bits(one["nb"][0]))
            _same_report(two["rep"], one["rep"])
            _same_report(two["rep_eval"], one["rep_eval"])


def test_knn_evaluate_restores_the_model_and_refuses_bad_settings():
    with calm.backend.use_backend(E.EmulatedKnnBackend()):
        torch.manual_seed(5)
        m = build_model("nano48_gen", None).train()
        data = _ImageSet(6, 3)
        batches = _shard_batches(data, 0, 1, 4)
        lean = calm.backend.get_lean_inference()
        rep = trainer.knn_evaluate(m, batches, batches, 10, k=1)
        assert m.training and calm.backend.get_lean_inference() == lean
        hand, pred = trainer.KnnProbe(10, k=1), trainer.Predictor(m, features=True)
        for x, y in batches:
            hand.add_bank(pred(x), y)
        for x, y in batches:
            hand.query(pred(x), y)
        assert rep["n"] == 6 and rep["bank"] == 6 and _scalars(rep) == _scalars(hand.read())
        assert _scalars(trainer.knn_evaluate(m, batches, batches, 10, k=1, lean=False)) == _scalars(rep)

        def broken(x):
            raise RuntimeError("no features today")
        with pytest.raises(RuntimeError, match="no features today"):
            trainer.knn_evaluate(m, batches, batches, 10, features=broken)
        assert m.training and calm.backend.get_lean_inference() == lean
        with pytest.raises(ValueError, match="k is an integer"):
            trainer.knn_evaluate(m, batches, batches, 10, k=300)
        with pytest.raises(ValueError, match="at least one batch"):
            trainer.knn_evaluate(m, [], batches, 10)
        with pytest.raises(TypeError, match="features is a callable"):
            trainer.knn_evaluate(m, batches, batches, 10, features=3)


# ---- train(knn=) ----------------------------------------------------------------------------------------------------------------
class _ImageSet(torch.utils.data.Dataset):
    """Images [3,48,48] in normalised space with a label in 0 .. 9."""

    def __init__(self, n=16, seed=7):
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randn(n, 3, 48, 48, generator=g) * 0.5
        self.y = torch.randint(0, 10, (n,), generator=g)

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return self.x[i], int(self.y[i])


BANK, VAL = (13, 21), (7, 22)                                   # (samples, seed): odd sizes, the shards differ in length


def _train(task, outdir=None, knn=True, every=2, epochs=2, **kw):
    torch.manual_seed(50)
    m = build_model("nano48_gen" if task == "reg" else "nano48_cls", None).train()
    extra = dict(task="reg", mim={"patch": 8, "ratio": 0.6}, ema=0.5) if task == "reg" else dict(num_classes=10)
    knn_kw = {"bank": _ImageSet(*BANK), "k": 5, "temperature": 0.1, "every": every, "batch_size": 4} if knn else None
    path = os.path.join(outdir, "model.pth") if outdir else None
    with calm.backend.use_backend(E.EmulatedKnnBackend()):
        return trainer.train(m, "fused", None, use_gpu=False, dataset=_ImageSet(8, 5), epochs=epochs, batch_size=2,
                             num_workers=0, log_every=1000, checkpoint_path=path, val_dataset=_ImageSet(*VAL),
                             val_batch_size=4, knn=knn_kw, **extra, **kw)


def _by_hand(model, ema=None):
    """knn_evaluate in one process on the whole sets, with train()'s settings."""
    with calm.backend.use_backend(E.EmulatedKnnBackend()):
        return trainer.knn_evaluate(model, _shard_batches(_ImageSet(*BANK), 0, 1, 4), _shard_batches(_ImageSet(*VAL), 0, 1, 4),
                                    10, k=5, temperature=0.1, ema=ema)


def _scalars(rep):
    return {k: v for k, v in rep.items() if not isinstance(v, torch.Tensor)}


def _check_log(outdir, model, task):
    lines = [json.loads(x) for x in open(os.path.join(outdir, "model_val.jsonl"))]
    assert [x["epoch"] for x in lines] == [1, 2]
    assert "knn" not in lines[0] and "knn" not in lines[0].get("ema", {})        # every=2: the first validation has no probe
    assert lines[1]["knn"] == _scalars(_by_hand(model))                           # the epoch's checkpoint is the model returned
    assert lines[1]["knn"]["n"] == VAL[0] and lines[1]["knn"]["bank"] == BANK[0] and "loss" not in lines[1]["knn"]
    if task == "reg":
        assert lines[1]["ema"]["knn"] == _scalars(_by_hand(model, ema=model._calm_ema))
        assert "huber" in lines[1] and "huber" in lines[1]["ema"]                  # the report it follows is still there


@pytest.mark.timeout(900)
@pytest.mark.parametrize("task", ["reg", "cls"])
def test_train_with_knn_logs_the_probe_and_does_not_move_the_run(task, tmp_path, capsys):
    out = _train(task, str(tmp_path))
    text = capsys.readouterr().out
    assert re.search(r"Epoch: 2, k-NN \(k=5, T=0\.1\): top-1: [\d.]+%, top-5: [\d.]+%, Bank: 13, Samples: 7", text)
    assert "Epoch: 1, k-NN" not in text and (("Epoch: 2, k-NN (EMA)" in text) == (task == "reg"))
    _check_log(str(tmp_path), out, task)
    plain = _train(task, knn=False)
    for (k, a), b in zip(out.state_dict().items(), plain.state_dict().values()):
        assert torch.equal(a, b), f"knn= moved the run at {k}"
    assert out.training


def _train_worker(rank, world, ports, outdir):
    for task, port_a, port_b in (("reg", ports[0], ports[1]), ("cls", ports[2], ports[3])):
        _join(rank, world, port_a)
        d = os.path.join(outdir, task)
        os.makedirs(d, exist_ok=True)
        out = _train(task, d)
        _join(rank, world, port_b)
        plain = _train(task, knn=False)
        torch.save(dict(run=out.state_dict(), plain=plain.state_dict(),
                        ema=out._calm_ema.state_dict() if task == "reg" else None), os.path.join(outdir, f"{task}{rank}.pt"))


@pytest.mark.timeout(900)
def test_train_with_knn_on_two_gloo_ranks(tmp_path):
    mp.spawn(_train_worker, args=(2, [_free_port() for _ in range(4)], str(tmp_path)), nprocs=2, join=True)
    for task in ("reg", "cls"):
        r0, r1 = (torch.load(os.path.join(tmp_path, f"{task}{r}.pt"), weights_only=False) for r in range(2))
        for k in r0["run"]:
            assert torch.equal(r0["run"][k], r0["plain"][k]), f"knn= moved the run at {k}"
            assert torch.equal(r0["run"][k], r1["run"][k]), f"the ranks diverged at {k}"
        torch.manual_seed(50)
        m = build_model("nano48_gen" if task == "reg" else "nano48_cls", None).train()
        m.load_state_dict(r0["run"])
        if task == "reg":
            with calm.backend.use_backend(E.EmulatedKnnBackend()):
                m._calm_ema = trainer.ModelEMA(m, decay=0.5)
                m._calm_ema.load_state_dict(r0["ema"])
        _check_log(os.path.join(tmp_path, task), m, task)


def test_train_knn_refusals_come_before_any_process_group():
    data = _ImageSet(4)
    lin = torch.nn.Linear(4, 4)
    kw = dict(use_gpu=False, dataset=data, epochs=1, batch_size=2, num_classes=10)
    with pytest.raises(ValueError, match="knn= needs val_dataset"):
        trainer.train(lin, "fused", knn=data, **kw)
    with pytest.raises(ValueError, match="knn takes a bank dataset"):
        trainer.train(lin, "fused", knn={"k": 5}, val_dataset=data, **kw)
    with pytest.raises(ValueError, match="knn takes a bank dataset"):
        trainer.train(lin, "fused", knn={"bank": data, "neighbours": 5}, val_dataset=data, **kw)
    with pytest.raises(ValueError, match="k is an integer within"):
        trainer.train(lin, "fused", knn={"bank": data, "k": 0}, val_dataset=data, **kw)
    with pytest.raises(ValueError, match="temperature is a positive"):
        trainer.train(lin, "fused", knn={"bank": data, "temperature": 0}, val_dataset=data, **kw)
    with pytest.raises(ValueError, match=r'knn\["every"\]'):
        trainer.train(lin, "fused", knn={"bank": data, "every": 0}, val_dataset=data, **kw)
    with pytest.raises(ValueError, match=r'knn\["batch_size"\]'):
        trainer.train(lin, "fused", knn={"bank": data, "batch_size": 0}, val_dataset=data, **kw)
    with pytest.raises(ValueError, match=r'knn\["bank"\] is a map-style dataset'):
        trainer.train(lin, "fused", knn={"bank": iter(())}, val_dataset=data, **kw)
    assert not torch.distributed.is_initialized()
