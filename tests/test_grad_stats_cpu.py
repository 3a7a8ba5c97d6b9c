"""The gradient monitor without a GPU: the float64 checker (tests/grad_stats_f64.py) on the fp32 emulation of
calm_grad_stats (tests/emulated_grad_stats.py) and on its planted faults, the C-ABI addition (calm_grad_stat, the two entry
points, the refusals), GradMonitor with the torch fallback on CPU parameters against the same checker, and
train(monitor=) on one and two gloo ranks."""
import ctypes
import json
import math
import os
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
import grad_stats_f64 as gs  # noqa: E402
import optim_groups_f64 as gf  # noqa: E402
import tail_f64 as tf  # noqa: E402
from emulated_backend import EmulatedBackend  # noqa: E402
from emulated_grad_stats import FAULTS, EmulatedGradStats  # noqa: E402
from test_host_logic_cpu import build_model  # noqa: E402
from test_snapshot_cpu import _TinySet  # noqa: E402
from importlib import import_module  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
TABLE = tf.optim_table()
DTYPE = np.dtype(binding.GradStat)


def fresh(n):
    out = np.zeros(n, dtype=DTYPE)
    out["first_bad_call"] = -1
    return out, np.asarray([0, 0, -1, -1], dtype=np.int32)


def names(failures):
    return {n for n, _ in failures}


# ---- the checker on the emulation ------------------------------------------------------------------------------------------
def _calls(sc, case=None):
    """Two calls of a scenario: (recs, grads, step) — another state and other gradients for the second, one step later;
    case: a tail_f64.optim_nonfinite_cases entry planted into the FIRST call's gradients."""
    out = []
    for call in (1, 2):
        recs = tf.optim_state(TABLE, seed=call - 1)
        grads = tf.optim_grads(TABLE, recs, seed=call, scale=sc["grad_scale"] or 1.0)
        if case is not None and call == 1:
            grads[case[1]][case[2]] = case[3]
        out.append((recs, grads, sc["t_prev"] + call - 1))
    return out


def _run(emu, sc, case=None, strict=True):
    """-> the failures of both calls (strict: raises at the first)"""
    out, summary = fresh(len(TABLE))
    sticky, failures = gs.Sticky(len(TABLE)), []
    for recs, grads, step in _calls(sc, case):
        hp = gf.hp_of(sc)
        ref, bound = gs.reference(recs, grads, hp, sc["grad_scale"], step)
        emu.call(recs, grads, hp, sc["grad_scale"], step, out, summary)
        worst, f = gs.check(out, summary, ref, bound, sticky.after(ref["nonfinite"].numpy()), strict=strict)
        if strict:
            print(f"grad stats {sc['name']} step {step}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
            if step < 1:
                assert not out["dir_sq"].any()
        failures += f
    return failures


@pytest.mark.parametrize("name", gf.SCENARIOS)
def test_emulation_inside_every_bound(name):
    _run(EmulatedGradStats(TABLE), gf.scenario(name))


@pytest.mark.parametrize("case", tf.optim_nonfinite_cases(TABLE), ids=lambda c: c[0])
def test_emulation_with_a_non_finite_gradient(case):
    _run(EmulatedGradStats(TABLE), gf.scenario("clip_t1000"), case)


# the scenario each fault shows in, the non-finite case it needs, and the fields the checker must name
PLANTED = {"no_correction": ("clip_t1000", None, {"grad_sq", "grad_absmax"}),
           "no_unscale": ("scaled_t100000", None, {"grad_sq", "grad_absmax"}),
           "expanded_norm": ("clip_t1000", None, {"grad_sq"}),
           "span_off_by_one": ("clip_t1000", None, {"grad_sq", "param_sq", "dir_sq", "param_absmax"}),
           "no_bias_correction": ("below_t2", None, {"dir_sq"}),
           "nonfinite_to_neighbour": ("clip_t1000", "nan_sn", {"nonfinite", "bad_calls", "first_bad_call", "summary"}),
           "not_sticky": ("clip_t1000", "inf_last", {"bad_calls", "first_bad_call"})}


@pytest.mark.parametrize("fault", FAULTS)
def test_checker_rejects_the_planted_fault(fault):
    scenario, case, must = PLANTED[fault]
    case = next(c for c in tf.optim_nonfinite_cases(TABLE) if c[0] == case) if case else None
    failures = _run(EmulatedGradStats(TABLE, fault), gf.scenario(scenario), case, strict=False)
    assert must <= names(failures), (fault, failures)
    _run(EmulatedGradStats(TABLE), gf.scenario(scenario), case)          # the clean emulation on the same inputs: strict


def test_planted_faults_cover_the_list():
    assert set(PLANTED) == set(FAULTS) and len(FAULTS) == 7


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------
def test_grad_stat_record_matches_the_header():
    fields = [n for n, _ in binding.GradStat._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "calm_vit.h"\nint main(void){printf("%zu", sizeof(calm_grad_stat));\n' + \
          "".join(f'printf(" %zu", offsetof(calm_grad_stat, {f}));\n' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert fields == ["grad_sq", "grad_absmax", "param_sq", "param_absmax", "dir_sq", "nonfinite", "bad_calls", "first_bad_call"]
    assert got == [32, 0, 4, 8, 12, 16, 20, 24, 28]
    assert got == [ctypes.sizeof(binding.GradStat)] + [getattr(binding.GradStat, f).offset for f in fields]
    assert DTYPE.itemsize == 32 and [DTYPE.fields[f][1] for f in fields] == got[1:]
    assert [DTYPE.fields[f][0] for f in fields] == [np.dtype(np.float32)] * 5 + [np.dtype(np.int32)] * 3


def test_abi_version_stays_and_the_scratch_query_needs_no_gpu():
    lib = binding.load()
    assert lib.calm_abi_version() == binding.ABI_VERSION == 7
    assert {"calm_grad_stats", "calm_grad_stats_scratch_floats"} <= set(binding.SIGNATURES)
    first, n_chunks = tf.optim_chunks(TABLE)
    need = lib.calm_grad_stats_scratch_floats(len(TABLE), n_chunks)
    assert need == 7 * n_chunks                             # <G, W_orig> and a six-float record per chunk
    assert lib.calm_grad_stats_scratch_floats(521, 2700) == 7 * 2700
    assert lib.calm_grad_stats_scratch_floats(0, 5) < 0 and lib.calm_grad_stats_scratch_floats(5, 0) < 0


_P = 0x7f0000010000          # a fake, 16-byte aligned device address: every call below is refused before any launch


@pytest.mark.parametrize("change,what", [({0: None}, "null tensors_dev"), ({2: None}, "null chunk_tensor_dev"),
                                         ({4: None}, "null hparams"), ({7: None}, "null out_dev"),
                                         ({8: None}, "null summary_dev"), ({9: None}, "null scratch"), ({1: 0}, "n_tensors 0"),
                                         ({1: -3}, "n_tensors negative"), ({3: 0}, "n_chunks 0"), ({"beta1": 1.0}, "beta1 1"),
                                         ({"beta1": -0.1}, "beta1 negative"), ({"beta2": 1.5}, "beta2 above 1")],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_calm_grad_stats_refuses_before_any_launch(change, what):
    lib, change = binding.load(), dict(change)
    h = binding.OptimHparams(1e-3, change.pop("beta1", 0.9), change.pop("beta2", 0.999), 1e-8, 0.0, 1.0, 1)
    args = [_P, 3, _P, 5, ctypes.byref(h), None, None, _P, _P, _P, None]
    for i, v in change.items():
        args[i] = v
    assert lib.calm_grad_stats(*args) == binding.E_INVAL, what


# ---- GradMonitor on CPU parameters: the torch fallback ------------------------------------------------------------------------
def _batch(seed=0, B=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 32, 32, generator=g), torch.softmax(torch.randn(B, 10, generator=g), 1)


def test_fallback_on_the_table_inside_every_bound():
    """grad_stats_torch on tail_f64's table, every scenario, with the sticky state across a non-finite first call."""
    case = tf.optim_nonfinite_cases(TABLE)[0]
    for name in gf.SCENARIOS:
        sc = gf.scenario(name)
        out, summary = fresh(len(TABLE))
        sticky = gs.Sticky(len(TABLE))
        for recs, grads, step in _calls(sc, case):
            scale = torch.tensor([sc["grad_scale"]]) if sc["grad_scale"] else None
            ref, bound = gs.reference(recs, grads, gf.hp_of(sc), sc["grad_scale"], step)
            trainer.grad_stats_torch(recs, torch.tensor([step], dtype=torch.int32), grads, gf.hp_of(sc), scale, out, summary)
            gs.check(out, summary, ref, bound, sticky.after(ref["nonfinite"].numpy()))
        assert list(summary) == [2, 1, 0, case[1]]


@pytest.mark.parametrize("window", [False, True], ids=["eager", "window-of-2"])
def test_monitor_on_cpu_parameters_reports_what_the_checker_expects(window):
    """Three optimizer steps of tiny32_cls with parameter groups; every observe() is checked against the float64 reference
    of the records and gradients it was handed, and read() against the records."""
    rules = [("*ls_*", {"lr_scale": 0.1}), (lambda name, p: p.ndim <= 1, {"weight_decay": 0.0})]
    with calm.backend.use_backend(EmulatedBackend()):
        torch.manual_seed(4)
        m = build_model("tiny32_cls", None).train()
        cls = trainer.FusedClipAdamWindow if window else trainer.FusedClipAdamW
        opt = cls(m, groups=trainer.param_groups(m, rules)[0])
        with pytest.raises(ValueError, match="FusedClipAdamW"):
            trainer.GradMonitor(m, torch.optim.SGD(m.parameters(), lr=0.1))
        with pytest.raises(ValueError, match="not parameters of this model"):
            trainer.GradMonitor(torch.nn.Linear(2, 2), opt)
        mon = trainer.GradMonitor(m, opt).attach()
        assert opt.monitor is mon and not mon.native
        assert mon.names == [n for n, p in m.named_parameters() if p.requires_grad]
        seen, real = [], mon.observe

        def spy(plan, grads, divisor, records):
            flat = lambda t: t.detach().clone().reshape(-1)           # noqa: E731  (tail_f64's records are flat)
            recs = [dict(param=flat(r["param"]), exp_avg=flat(r["exp_avg"]), exp_avg_sq=flat(r["exp_avg_sq"]),
                         sn=None if r["sn"] is None else tuple(flat(t) if torch.is_tensor(t) else t for t in r["sn"]))
                    for r in records]
            seen.append((recs, [flat(g) for g in grads], None if divisor is None else float(divisor), int(plan.step_dev), opt._hparams()))
            real(plan, grads, divisor, records)

        mon.observe = spy
        step = trainer.AccumTrainStep(m, opt, accumulate=2) if window else trainer.TrainStep(m, opt)
        sticky = gs.Sticky(mon.n)
        try:
            for k in range(6 if window else 3):
                step(*_batch(k))
                if window and not step.boundary:
                    continue
                recs, grads, divisor, t, hp = seen[-1]
                assert t == len(seen) - 1 and divisor == (2.0 if window else None)
                assert all((r["sn"] is None) for r in recs) == window         # the window's plan steps finished gradients
                ref, bound = gs.reference(recs, grads, hp, divisor, t)
                got, summary = mon._views(mon._host)
                worst, _ = gs.check(got, summary, ref, bound, sticky.after(ref["nonfinite"].numpy()))
                print(f"monitor step {t}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
                rep = mon.read()
                assert rep["calls"] == t + 1 and rep["skipped"] == 0 and rep["first_bad"] is None
                norm, e_norm = gs.norm_bound(ref, bound)
                assert abs(rep["norm"] - norm) <= e_norm
                o_ref, o_bound = tf.optim_reference(recs, grads, hp, divisor, t)     # the step's own (unclipped) norm:
                assert abs(float(opt.stats[0]) - o_ref["norm"]) <= o_bound["norm"]   # each inside its derived bound of the
                assert abs(rep["norm"] - float(opt.stats[0])) <= e_norm + o_bound["norm"]    # same float64 norm
                assert len(rep["groups"]) == 3 and sum(g["tensors"] for g in rep["groups"]) == mon.n
                rates = [g["lr"] for g in opt.param_groups]
                assert [g["lr"] for g in rep["groups"]] == rates
                for name, g, r in zip(mon.names, mon.group_of, got):
                    e = rep["tensors"][name]
                    assert e["group"] == g and e["grad_sq"] == float(r["grad_sq"]) and e["grad_norm"] == math.sqrt(float(r["grad_sq"]))
                    want = rates[g] * math.sqrt(float(r["dir_sq"]) / float(r["param_sq"])) if r["param_sq"] > 0 else 0.0
                    assert e["update_ratio"] == want and e["weight_norm"] == math.sqrt(float(r["param_sq"]))
                assert all(e["update_ratio"] == 0.0 for e in rep["tensors"].values()) == (t == 0)
            assert len(seen) == 3
            mon.reset()
            rep = mon.read()
            assert (rep["calls"], rep["skipped"], rep["first_bad"], rep["norm"]) == (0, 0, None, 0.0)
            assert all(e["bad_calls"] == 0 and e["first_bad_call"] == -1 for e in rep["tensors"].values())
            mon.detach()
            assert opt.monitor is None
        finally:
            opt.close()


# ---- train(monitor=) ---------------------------------------------------------------------------------------------------------
def _train(tmp=None, seed=50, n=8, epochs=2, plant=None, **kw):
    """train("fused") on the CPU model: `epochs` epochs of n / 4 batches (per rank).  plant = (name, k): the k-th backward
    (0-based) leaves an inf in that parameter's gradient."""
    torch.manual_seed(seed)
    m = build_model("tiny32_cls", None).train()
    if plant is not None:
        count = [0]

        def hook(g):
            count[0] += 1
            if count[0] - 1 == plant[1]:
                g = g.clone()
                g.view(-1)[0] = float("inf")
            return g

        dict(m.named_parameters())[plant[0]].register_hook(hook)
    if tmp is not None:
        kw["checkpoint_path"] = os.path.join(str(tmp), "model.pth")
    with calm.backend.use_backend(EmulatedBackend()):
        return trainer.train(m, "fused", None, use_gpu=False, dataset=_TinySet(n), epochs=epochs, batch_size=4,
                             num_classes=10, collate_fn="mix", num_workers=0, log_every=1000, **kw)


def _lines(tmp):
    with open(os.path.join(str(tmp), "model_grad.jsonl")) as f:
        return [json.loads(line, parse_constant=lambda c: pytest.fail(f"not strict JSON: {c}")) for line in f]


def _same_bits(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"the monitored run differs at {k}"


PLANT = "blocks.0.mlp.fc1.bias"


def _plant_name():
    names_ = [n for n, p in build_model("tiny32_cls", None).named_parameters() if n.endswith(".bias")]
    return PLANT if PLANT in names_ else names_[0]


@pytest.mark.timeout(600)
def test_train_with_a_monitor_writes_the_log_and_trains_the_same_parameters(tmp_path, capsys):
    plain = _train()
    capsys.readouterr()
    out = _train(tmp_path, monitor={"every": 1, "top": 3, "per_tensor": True}, param_groups="no_decay")
    printed = capsys.readouterr().out
    _same_bits(out, _train(param_groups="no_decay"))
    _same_bits(_train(monitor=True), plain)
    mon = out._calm_monitor
    assert isinstance(mon, trainer.GradMonitor) and mon.optimizer.monitor is None
    lines = _lines(tmp_path)
    # 2 epochs of 2 steps: a line behind every step and one at every epoch end
    assert [(e["epoch"], e["step"]) for e in lines] == [(1, 1), (1, 2), (1, 2), (2, 3), (2, 4), (2, 4)]
    assert printed.count("Gradient norm:") == 6 and "Non-finite gradient" not in printed
    for k, e in enumerate(lines):
        assert e["skipped"] == 0 and e["first_bad"] is None and e["nonfinite"] == [] and e["norm"] > 0
        assert e["calls"] == e["step"] and len(e["groups"]) == 2
        assert len(e["top_grad_norm"]) == 3 and len(e["top_update_ratio"]) == 3
        assert e["top_grad_norm"][0]["grad_norm"] >= e["top_grad_norm"][2]["grad_norm"]
        assert ("tensors" in e) == (k in (2, 5))                       # the full table at the epoch ends only
    assert set(lines[5]["tensors"]) == set(mon.names) and lines[0]["top_update_ratio"][0]["update_ratio"] == 0.0
    assert lines[1]["top_update_ratio"][0]["update_ratio"] > 0.0


@pytest.mark.timeout(600)
def test_train_names_the_tensor_that_made_a_step_skip(tmp_path, capsys):
    name = _plant_name()
    out = _train(tmp_path, plant=(name, 1), monitor={"every": 1})
    printed = capsys.readouterr().out
    lines = _lines(tmp_path)
    assert [e["skipped"] for e in lines] == [0, 1, 1, 1, 1, 1]
    assert lines[1]["first_bad"] == {"call": 1, "tensor": name}
    assert lines[1]["nonfinite"] == [{"name": name, "bad_calls": 1, "first_bad_call": 1}] and lines[2]["nonfinite"] == []
    assert printed.count(f"Non-finite gradient in: {name}") == 1
    rep = out._calm_monitor.read()
    assert rep["skipped"] == 1 and rep["calls"] == 4 and rep["tensors"][name]["bad_calls"] == 1
    assert out._calm_monitor.optimizer.step_count == 3              # the optimizer skipped that step


def test_monitor_refusals_come_before_any_process_group():
    data = torch.utils.data.TensorDataset(torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,)))
    lin = torch.nn.Linear(4, 4)
    sgd = torch.optim.SGD(lin.parameters(), lr=0.1)
    kw = dict(use_gpu=False, dataset=data, epochs=1, batch_size=2, num_classes=10)
    with pytest.raises(ValueError, match='monitor= needs optimizer="fused"'):
        trainer.train(lin, sgd, monitor=True, **kw)
    with pytest.raises(ValueError, match='"every", "top", "per_tensor"'):
        trainer.train(lin, "fused", monitor={"each": 2}, **kw)
    with pytest.raises(ValueError, match=r'monitor\["every"\]'):
        trainer.train(lin, "fused", monitor={"every": 0}, **kw)
    with pytest.raises(ValueError, match="None, True or a dict"):
        trainer.train(lin, "fused", monitor=3, **kw)
    assert not torch.distributed.is_initialized()


# ---- two gloo ranks ------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _two_rank_worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    plain = _train(n=16, destroy_process_group=False)
    tmp = os.path.join(outdir, f"rank{rank}")
    os.makedirs(tmp)
    out = _train(tmp, n=16, monitor={"every": 1}, destroy_process_group=False)
    bad = _train(n=16, plant=(_plant_name(), 2), monitor=True, destroy_process_group=False)
    torch.save({"plain": plain.state_dict(), "monitored": out.state_dict(), "calls": out._calm_monitor.read()["calls"],
                "bad": {k: bad._calm_monitor.read()[k] for k in ("skipped", "first_bad", "calls")}},
               os.path.join(outdir, f"rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_train_with_a_monitor_on_two_gloo_ranks(tmp_path):
    mp.spawn(_two_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(2))
    for k in r0["plain"]:
        assert torch.equal(r0["plain"][k], r0["monitored"][k]), f"the monitored run differs at {k}"
        assert torch.equal(r0["monitored"][k], r1["monitored"][k]), f"ranks diverged at {k}"
    # every rank ran the kernels; rank 0 alone wrote
    assert r0["calls"] == r1["calls"] == 4
    assert os.path.exists(tmp_path / "rank0" / "model_grad.jsonl") and not os.path.exists(tmp_path / "rank1" / "model_grad.jsonl")
    lines = _lines(tmp_path / "rank0")
    assert [(e["epoch"], e["step"]) for e in lines] == [(1, 1), (1, 2), (1, 2), (2, 3), (2, 4), (2, 4)]
    # the planted inf reaches both ranks through the all-reduce
    want = {"skipped": 1, "first_bad": {"call": 2, "tensor": _plant_name()}, "calls": 4}
    assert r0["bad"] == want and r1["bad"] == want
