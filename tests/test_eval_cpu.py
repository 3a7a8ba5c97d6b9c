"""Validation metrics on a host without a GPU:
  * calm_eval_metrics is declared, exported and bound, the ABI version is still 7, the scratch plan answers 4 floats per
    row and every refusal comes before any launch;
  * the fp32 emulation of the two launches (tests/emulated_eval.py) agrees with the float64 checker (tests/eval_f64.py) on
    the shapes the GPU test uses, and the checker catches planted faults;
  * trainer.EvalMetrics: its torch fallback and the emulation agree to the integer; read / reset / refusals;
  * trainer.validation_shard, evaluate(report=...) alone and on two gloo ranks, train(val_dataset=...) on two gloo ranks."""
import ctypes
import json
import os
import re
import socket
import sys
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import calm_vit_dte_amd as calm  # noqa: E402
import eval_f64 as F  # noqa: E402
import emulated_eval as E  # noqa: E402
from test_host_logic_cpu import build_model  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
HEADER = os.path.join(ROOT, "include", "calm_vit.h")
KS = (1, 5)
# the emulation's fp32 formula against float64: each row's nll carries a few fp32 roundings (the subtraction, exp, the sum
# of C terms, log) of magnitudes up to |max - z_l| + log C ~ 25, and the row sum adds B more: 1e-5 relative is 40 ulp
LOSS_TOL = 1e-5


@pytest.fixture(autouse=True)
def _restore_switch():
    prev = calm.backend.get_loss_kernels()
    yield
    calm.backend.set_loss_kernels(prev)


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_bound_and_the_scratch_plan_answers():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(calm_\w+)\s*\(", text, flags=re.M))
    lib = binding.load()
    assert "calm_eval_metrics" in declared
    assert "calm_eval_metrics" in binding.SIGNATURES and hasattr(lib, "calm_eval_metrics")
    assert len(binding.SIGNATURES["calm_eval_metrics"][1]) == 13
    assert int(re.search(r"#define\s+CALM_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 7   # an addition only
    assert binding.ABI_VERSION == 7 and lib.calm_abi_version() == 7
    assert re.search(r"CALM_RED_EVAL\s*=\s*7\b", open(HEADER).read()) and binding.RED_EVAL == 7
    for rows, cols in [(1, 1), (7, 1000), (256, 1000), (1030, 10), (1 << 20, 65536)]:
        assert int(lib.calm_reduce_scratch_floats(binding.RED_EVAL, rows, cols)) == 4 * rows
    assert int(lib.calm_reduce_scratch_floats(binding.RED_EVAL, 0, 10)) == 0
    assert int(lib.calm_reduce_scratch_floats(99, 10, 10)) == 0


_P = 0x7f0000010000            # a fake, 16-byte aligned device address: every call below is turned down before any launch


def _args(**change):
    ks = change.pop("ks", [1, 5])
    a = dict(logits=_P, ld=1000, logits_type=binding.ST_F32, labels=_P,
             ks=None if ks is None else (ctypes.c_int32 * len(ks))(*ks), nk=2 if ks is None else len(ks),
             counts=_P, loss_sum=_P, confusion=None, B=8, C=1000, partials=_P, stream=None)
    a.update(change)
    return list(a.values())


def test_every_refusal_comes_before_any_launch():
    lib = binding.load()
    call = lib.calm_eval_metrics
    for name in ("logits", "labels", "ks", "counts", "loss_sum", "partials"):
        assert call(*_args(**{name: None})) == binding.E_INVAL, name
    for nk in (0, 5, -1):
        assert call(*_args(ks=[1, 2, 3, 4, 5], nk=nk)) == binding.E_INVAL, nk
    assert call(*_args(ks=[1, 0])) == binding.E_INVAL
    assert call(*_args(ks=[-3])) == binding.E_INVAL
    for st in (binding.ST_FP8_E4M3, binding.ST_FP8_E5M2, 7, -1):
        assert call(*_args(logits_type=st)) == binding.E_INVAL, st
    for kw in (dict(B=0), dict(C=0), dict(B=-4), dict(ld=999)):
        assert call(*_args(**kw)) == binding.E_INVAL, kw
    assert call(*_args(C=65537, ld=65537)) == binding.E_UNSUPP
    assert call(*_args(C=1 << 20, ld=1 << 20, logits_type=binding.ST_BF16)) == binding.E_UNSUPP
    assert call(*_args(partials=_P + 4)) == binding.E_LAYOUT


# ---- emulation against the checker ----------------------------------------------------------------------------------------
def _emulate(z, labels, ks=KS, fault=None, confusion=True):
    be = E.EmulatedEvalBackend()
    be.eval_fault = fault
    C = z.shape[1]
    counts, loss = torch.zeros(7 + 2 * C, dtype=torch.int64), torch.zeros(1, dtype=torch.float64)
    conf = torch.zeros(C, C, dtype=torch.int64) if confusion else None
    be.eval_metrics(z, labels, ks, counts, loss, conf, z.shape[0], C)
    return counts, float(loss), conf


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,C", F.SHAPES)
def test_emulation_agrees_with_the_checker(B, C, dtype):
    for inf_row in (True, False):
        z, labels = F.make_case(B, C, dtype, inf_row=inf_row)
        ref = F.reference(z, labels, KS)
        counts, loss, conf = _emulate(z, labels)
        assert F.mismatches(counts, conf, ref, len(KS)) == []
        err = F.loss_error(loss, ref["loss_sum"])
        print(f"\neval {B}x{C} {dtype} inf_row={inf_row}: loss sum {loss!r} vs {ref['loss_sum']!r}, rel err {err:.2e}")
        assert err <= LOSS_TOL
        assert np.isnan(ref["loss_sum"]) == (inf_row and B > 4)          # the all -inf row makes the loss NaN, as in torch
    assert int(ref["counts"][0]) == B - min(max(B - 1, 0), 2)            # the inputs hold what they promise
    assert int(ref["counts"][2]) == (B > 3)


def test_the_inputs_exercise_hits_misses_and_ties():
    z, labels = F.make_case(130, 257)
    ref = F.reference(z, labels, (1, 5, 300))
    rows, top1, top5, topall = (int(ref["counts"][i]) for i in (0, 3, 4, 5))
    assert 0 < top1 < top5 < topall == rows - 1                          # k > C counts every finite row
    l = int(labels[0])
    assert z[0, l - 1] == z[0, l] or z[0, l + 1] == z[0, l]


@pytest.mark.parametrize("fault,names", [("tie_high", "hits"), ("le_k", "hits"), ("nan_hit", "nonfinite"),
                                         ("skipped_in_rows", "rows"), ("confusion_T", "confusion")])
def test_the_checker_catches_planted_faults(fault, names):
    z, labels = F.make_case(130, 257)
    ref = F.reference(z, labels, KS)
    counts, _, conf = _emulate(z, labels, fault=fault)
    bad = F.mismatches(counts, conf, ref, len(KS))
    assert bad and any(names in b for b in bad), (fault, bad)


# ---- trainer.EvalMetrics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,C", F.SHAPES)
def test_torch_fallback_and_emulated_kernel_path_agree_to_the_integer(B, C, dtype):
    z, labels = F.make_case(B, C, dtype, inf_row=False)
    be = E.EmulatedEvalBackend()
    with calm.backend.use_backend(be):
        calm.backend.set_loss_kernels(False)
        a = trainer.EvalMetrics(C, topk=(1, 5, 2), confusion=True)
        a.update(z, labels)
        assert getattr(be, "eval_calls", 0) == 0
        calm.backend.set_loss_kernels(True)
        b = trainer.EvalMetrics(C, topk=(1, 5, 2), confusion=True)
        b.update(z, labels)
        assert be.eval_calls == 1
    assert torch.equal(a.counts, b.counts) and torch.equal(a.confusion, b.confusion)
    ref = F.reference(z, labels, (1, 5, 2))
    assert F.mismatches(a.counts, a.confusion, ref, 3) == []
    assert F.loss_error(float(a.loss_sum), ref["loss_sum"]) <= LOSS_TOL
    assert F.loss_error(float(b.loss_sum), ref["loss_sum"]) <= LOSS_TOL


def test_eval_metrics_accumulates_reads_and_resets():
    C = 10
    z, labels = F.make_case(1030, C, inf_row=False)
    m = trainer.EvalMetrics(C, confusion=True)
    addresses = [t.data_ptr() for t in m.tensors()]
    for part in (slice(0, 7), slice(7, 500), slice(500, 1030)):
        m.update(z[part], labels[part])
    one = trainer.EvalMetrics(C, confusion=True)
    one.update(z, labels)
    assert torch.equal(m.counts, one.counts) and torch.equal(m.confusion, one.confusion)
    rep = m.read()
    ref = F.reference(z, labels, (1, 5))
    n, nonfinite = int(ref["counts"][0]), int(ref["counts"][2])
    assert (rep["n"], rep["skipped"], rep["nonfinite"]) == (n, 2, 1) and n == 1028
    assert rep["top1"] == int(ref["counts"][3]) / n and rep["top5"] == int(ref["counts"][4]) / n
    assert abs(rep["loss"] - ref["loss_sum"] / (n - nonfinite)) <= LOSS_TOL * rep["loss"]
    support, hits1 = ref["counts"][7:7 + C], ref["counts"][7 + C:]
    assert torch.equal(rep["per_class_accuracy"], torch.from_numpy(hits1 / support))
    assert rep["mean_per_class_accuracy"] == pytest.approx(float(np.mean(hits1 / support)), rel=1e-12)
    assert torch.equal(rep["confusion"], torch.from_numpy(ref["confusion"]))
    assert set(rep) == {"n", "skipped", "nonfinite", "loss", "top1", "top5", "per_class_accuracy",
                        "mean_per_class_accuracy", "confusion"}
    json.dumps({k: v for k, v in rep.items() if not isinstance(v, torch.Tensor)})      # plain Python numbers
    m.reset()
    assert [t.data_ptr() for t in m.tensors()] == addresses and all(int(t.abs().sum()) == 0 for t in m.tensors())
    empty = m.read()
    assert (empty["n"], empty["top1"], empty["loss"], empty["mean_per_class_accuracy"]) == (0, 0.0, 0.0, 0.0)
    # a class without support is NaN in the per-class list and left out of the mean
    few = trainer.EvalMetrics(4, topk=(1,))
    few.update(torch.tensor([[3.0, 1.0, 0.0, 0.0], [0.0, 0.0, 2.0, 1.0]]), torch.tensor([0, 3]))
    r = few.read()
    assert r["mean_per_class_accuracy"] == 0.5 and "confusion" not in r and "top5" not in r
    assert torch.isnan(r["per_class_accuracy"][1]) and r["per_class_accuracy"][0] == 1.0


def test_eval_metrics_refuses_malformed_arguments():
    for topk in ((), (1, 2, 3, 4, 5), (0,), (1, 1), (1.5,)):
        with pytest.raises(ValueError, match="topk"):
            trainer.EvalMetrics(10, topk=topk)
    for C in (0, 65537):
        with pytest.raises(ValueError, match="num_classes"):
            trainer.EvalMetrics(C)
    m = trainer.EvalMetrics(10)
    with pytest.raises(ValueError, match="logits"):
        m.update(torch.zeros(4, 9), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="labels"):
        m.update(torch.zeros(4, 10), torch.zeros(3, dtype=torch.int64))


# ---- validation_shard, evaluate ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 3])
def test_validation_shard_covers_every_index_exactly_once(world):
    data = torch.utils.data.TensorDataset(torch.arange(17))                 # 17: no world above 1 divides it
    seen = []
    for rank in range(world):
        shard = trainer.validation_shard(data, rank, world)
        mine = [int(shard[i][0]) for i in range(len(shard))]
        assert mine == list(range(rank, 17, world))
        seen += mine
    assert sorted(seen) == list(range(17))
    with pytest.raises(ValueError):
        trainer.validation_shard(data, world, world)


class _TinySet(torch.utils.data.Dataset):
    def __init__(self, n=16, seed=7):
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randn(n, 3, 32, 32, generator=g)
        self.y = torch.randint(0, 10, (n,), generator=g)

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return self.x[i], int(self.y[i])


def _val_batches(data, rank=0, world=1, bs=4):
    shard = trainer.validation_shard(data, rank, world)
    return [(torch.stack([shard[i][0] for i in range(j, min(j + bs, len(shard)))]),
             torch.tensor([shard[i][1] for i in range(j, min(j + bs, len(shard)))])) for j in range(0, len(shard), bs)]


def _model_and_labelled_set(n=11):
    """tiny32 classification model and a set whose labels are its own predictions, every third one moved off by one."""
    torch.manual_seed(3)
    m = build_model("tiny32_cls", None).train()
    data = _TinySet(n)
    with torch.no_grad():
        logits = m.eval()(data.x)[0].reshape(n, -1)
    m.train()
    data.y = logits.argmax(dim=1)
    data.y[::3] = (data.y[::3] + 1) % 10
    return m, data, logits


def test_evaluate_without_report_is_unchanged_and_the_report_agrees_with_it():
    with calm.backend.use_backend(E.EmulatedEvalBackend()):
        m, data, logits = _model_and_labelled_set()
        batches = _val_batches(data)
        acc = trainer.evaluate(m, batches)
        assert isinstance(acc, float) and acc == int((logits.argmax(1) == data.y).sum()) / 11 == 7 / 11
        assert trainer.evaluate(m, batches, report=False, topk=(1, 2), confusion=True) == acc
        rep = trainer.evaluate(m, batches, report=True, confusion=True)
        lean = trainer.evaluate(m, batches, report=True, lean=True, topk=(1, 3))
        assert m.training
    ref = F.reference(logits, data.y, (1, 5))
    assert rep["top1"] == acc and rep["n"] == 11 and rep["top5"] == int(ref["counts"][4]) / 11
    assert abs(rep["loss"] - ref["loss_sum"] / 11) <= LOSS_TOL * rep["loss"]
    assert torch.equal(rep["confusion"], torch.from_numpy(ref["confusion"]))
    assert lean["top1"] == acc and "top3" in lean and "top5" not in lean
    with pytest.raises(ValueError, match="at least one batch"):
        trainer.evaluate(m, [], report=True)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _join(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)


def _evaluate_worker(rank, world, port, outdir):
    _join(rank, world, port)
    torch.distributed.init_process_group(backend="gloo")
    with calm.backend.use_backend(E.EmulatedEvalBackend()):
        m, data, _ = _model_and_labelled_set()
        rep = trainer.evaluate(m, _val_batches(data, rank, world), report=True, confusion=True)
    torch.save(rep, os.path.join(outdir, f"rep{rank}.pt"))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_gloo_ranks_produce_the_single_process_report(tmp_path):
    mp.spawn(_evaluate_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    with calm.backend.use_backend(E.EmulatedEvalBackend()):
        m, data, _ = _model_and_labelled_set()
        one = trainer.evaluate(m, _val_batches(data), report=True, confusion=True)
    for rank in range(2):
        rep = torch.load(os.path.join(tmp_path, f"rep{rank}.pt"))
        assert set(rep) == set(one) and rep["n"] == len(data) == 11
        for k in one:
            if isinstance(one[k], torch.Tensor):                            # (NaN: a class without support)
                assert torch.equal(rep[k].double().nan_to_num(nan=-1.0), one[k].double().nan_to_num(nan=-1.0)), k
            elif k == "loss":
                assert abs(rep[k] - one[k]) <= 1e-6 * abs(one[k])            # (fp32 batch sums, other batch boundaries)
            else:
                assert rep[k] == one[k], k


# ---- train(val_dataset=...) on two gloo ranks -------------------------------------------------------------------------------
EPOCHS = 3


def _train_worker(rank, world, ports, outdir):
    """Four runs in one pair of processes: with / without val_dataset, each with / without ema."""
    saves = []
    real_save = torch.save
    for port, (val, ema) in zip(ports, [(True, True), (False, True), (True, False), (False, False)]):
        _join(rank, world, port)
        tag = f"val{int(val)}_ema{int(ema)}"
        path = os.path.join(outdir, tag, "model_cls.pth")
        epoch_of = {}

        def spy(obj, f, *a, **kw):
            if isinstance(f, str) and "_best" in f:
                saves.append((tag, os.path.basename(f), epoch_of.get("n", 0)))
            if isinstance(f, str) and f == path:
                epoch_of["n"] = epoch_of.get("n", 0) + 1                      # the per-epoch checkpoint comes first
            return real_save(obj, f, *a, **kw)
        torch.manual_seed(50 + rank)
        m = build_model("tiny32_cls", None).train()
        torch.save = spy
        try:
            with calm.backend.use_backend(E.EmulatedEvalBackend()):
                out = trainer.train(m, trainer.make_optimizer(m), None, use_gpu=False, dataset=_TinySet(), epochs=EPOCHS,
                                    batch_size=4, num_classes=10, checkpoint_path=path, log_every=1000,
                                    ema=0.9 if ema else None, val_dataset=_TinySet(11, seed=9) if val else None,
                                    val_every=1, val_batch_size=3, val_topk=(1, 5))
        finally:
            torch.save = real_save
        assert out.training
        torch.save({k: v for k, v in out.state_dict().items()}, os.path.join(outdir, f"{tag}_rank{rank}.pt"))
    if rank == 0:
        json.dump(saves, open(os.path.join(outdir, "saves.json"), "w"))


@pytest.mark.timeout(900)
def test_train_validates_logs_keeps_the_best_and_does_not_move_the_run(tmp_path):
    mp.spawn(_train_worker, args=(2, [_free_port() for _ in range(4)], str(tmp_path)), nprocs=2, join=True)
    saves = [tuple(s) for s in json.load(open(os.path.join(tmp_path, "saves.json")))]
    for ema in (1, 0):
        with_val = torch.load(os.path.join(tmp_path, f"val1_ema{ema}_rank0.pt"))
        without = torch.load(os.path.join(tmp_path, f"val0_ema{ema}_rank0.pt"))
        other = torch.load(os.path.join(tmp_path, f"val1_ema{ema}_rank1.pt"))
        assert set(with_val) == set(without)
        for k in with_val:
            assert torch.equal(with_val[k], without[k]), k                    # validation did not move the run
            assert torch.equal(with_val[k], other[k]), k
        d = os.path.join(tmp_path, f"val1_ema{ema}")
        lines = [json.loads(x) for x in open(os.path.join(d, "model_cls_val.jsonl"))]
        assert [x["epoch"] for x in lines] == list(range(1, EPOCHS + 1))       # one line per validated epoch
        assert [x["step"] for x in lines] == [2 * e for e in range(1, EPOCHS + 1)]     # 16 samples / 2 ranks / batch 4
        for x in lines:
            assert x["n"] == 11 and x["skipped"] == 0 and 0.0 <= x["top1"] <= x["top5"] <= 1.0 and x["loss"] > 0
            assert "per_class_accuracy" not in x and "mean_per_class_accuracy" in x
            assert ("ema" in x) == bool(ema)
        for name, key in (("model_cls_best.pth", None),) + ((("model_cls_ema_best.pth", "ema"),) if ema else ()):
            tops = [(x if key is None else x[key])["top1"] for x in lines]
            improved = [e + 1 for e, t in enumerate(tops) if t > max(tops[:e], default=-1.0)]   # strictly
            assert [e for t, n, e in saves if t == f"val1_ema{ema}" and n == name] == improved, (name, tops)
            assert os.path.exists(os.path.join(d, name))
        assert os.path.exists(os.path.join(d, "model_cls_ema_best.pth")) == bool(ema)
        assert not os.path.exists(os.path.join(tmp_path, f"val0_ema{ema}", "model_cls_val.jsonl"))
        assert not [s for s in saves if s[0] == f"val0_ema{ema}"]


def test_best_values_come_back_from_an_existing_log(tmp_path):
    log = os.path.join(tmp_path, "m_val.jsonl")
    assert trainer._val_best_so_far(log) == {}
    with open(log, "w") as f:
        f.write(json.dumps({"epoch": 1, "step": 2, "top1": 0.25, "ema": {"top1": 0.125}}) + "\n")
        f.write(json.dumps({"epoch": 2, "step": 4, "top1": 0.5, "ema": {"top1": 0.0625}}) + "\n\n")
        f.write(json.dumps({"epoch": 3, "step": 6, "top1": 0.375}) + "\n")
    assert trainer._val_best_so_far(log) == {"top1": 0.5, "ema_top1": 0.125}


def test_validation_argument_errors_come_before_any_process_group():
    data = _TinySet(4)
    sgd = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    kw = dict(use_gpu=False, dataset=data, epochs=1, batch_size=2, num_classes=10)
    for bad, match in ((dict(val_every=0), "val_every"), (dict(val_every=1.5), "val_every"),
                       (dict(val_transform=object()), "val_transform"),
                       (dict(val_dataset=data, val_topk=(5,)), "val_topk"),
                       (dict(val_dataset=data, val_topk=(1, 2, 3, 4, 5)), "topk"),
                       (dict(val_dataset=data, val_batch_size=0), "val_batch_size")):
        with pytest.raises(ValueError, match=match):
            trainer.train(torch.nn.Linear(4, 4), sgd, **kw, **bad)
    assert not torch.distributed.is_initialized()
