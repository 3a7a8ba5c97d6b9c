"""calm_grad_stats of libcalmvit_hip.so against the float64 checker (tests/grad_stats_f64.py) on tail_f64.optim_table() —
the smallest table at which the chunk walk, the deferred correction, the two access paths and the sticky update can each
go wrong — then GradMonitor on tiny32_cls and train(monitor=True, graph=True).  tail_f64's arenas put tensors at whatever
float offset the running sizes give: there every deferred tensor is read as single words and only a few plain ones as
16-byte vectors, so the table is run a second time in arenas that start every tensor 16-byte aligned.  tests/test_grad_stats_cpu.py proves the checker on an fp32 emulation and on planted
faults.  Outputs and scratch sit between NaN-pattern guards; every input arena must come back bit for bit."""
import functools
import json
import math
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import grad_stats_f64 as gs
import optim_groups_f64 as gf
import tail_f64 as tf
import weights as W
from helpers import CONFIGS, load_golden
from test_host_logic_cpu import build_model
from test_rowwise_f64_gpu import GUARD, Out, place
from test_tail_f64_gpu import Arena, Device, _state_from, show
from test_trainer_gpu import _batch

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
TABLE = tf.optim_table()
N = len(TABLE)
DTYPE = np.dtype(binding.GradStat)
NAME = "tiny32_cls"


@pytest.fixture(scope="module")
def hip():
    return calm.backend.get_backend()


def _initial():
    rec = np.zeros(N, dtype=DTYPE)
    rec["first_bad_call"] = -1
    return np.concatenate([rec.view(np.int32), np.asarray([0, 0, -1, -1], dtype=np.int32)])


def _aligned(t):
    return t.data_ptr() % 16 == 0


class StatsDevice(Device):
    """tail_f64's device state with the monitor's buffers: the records and the summary in one guarded output (initialised
    as the host must: counts 0, firsts -1), the scratch in another.  aligned: every tensor of every arena, the gradients'
    included, starts on a multiple of 16 bytes (a pad in front of it) instead of where tail_f64's layout puts it."""

    def __init__(self, hip, table, recs, aligned=False):
        self.goff = [e["goff"] for e in table]
        if not aligned:
            super().__init__(hip, table, recs)
        else:
            self.hip, self.table, self.goff, at = hip, table, [], 0
            for e in table:                                  # Arena: at += GUARD + offset; tensor; at += numel
                self.goff.append(-(at + GUARD) % 4)
                at += GUARD + self.goff[-1] + e["numel"]
            self.p, self.m, self.v = (Arena([r[k] for r in recs], self.goff) for k in ("param", "exp_avg", "exp_avg_sq"))
            self.sn = [None if r["sn"] is None else tuple(place(t) for t in r["sn"][:3]) + tuple(r["sn"][3:]) for r in recs]
            self.plan = hip.optim_plan([dict(param=p, exp_avg=m, exp_avg_sq=v, sn=s)
                                        for p, m, v, s in zip(self.p.views, self.m.views, self.v.views, self.sn)])
        self.out = Out((8 * N + 4,), init=torch.from_numpy(_initial()).view(torch.float32))
        self.scratch = Out((hip.grad_stats_scratch_floats(self.plan),))
        assert self.scratch.t.numel() == 7 * self.plan.n_chunks

    def reset(self):
        self.out.t.copy_(torch.from_numpy(_initial()).view(torch.float32))

    def launch(self, views, sc):
        gs_dev = place(torch.tensor([sc["grad_scale"]])) if sc["grad_scale"] else None
        self.hip.grad_stats(self.plan, views, gf.hp_of(sc), gs_dev, self.out.t[:8 * N].view(torch.uint8),
                            self.out.t[8 * N:].view(torch.int32), self.scratch.t)

    def result(self):
        """(records, summary) on the host; the guards of the outputs must be untouched"""
        host = self.out.check(written=False).numpy().view(np.int32)
        self.scratch.check(written=False)
        return host[:8 * N].view(DTYPE).copy(), host[8 * N:].copy()

    def vector_path(self, grad_views):
        """per tensor: are its four operands 16-byte aligned (every chunk starts a multiple of 4 elements further)?"""
        return [all(_aligned(t) for t in q) for q in zip(grad_views, self.p.views, self.m.views, self.v.views)]

    def stats(self, grads, sc):
        G = Arena(grads, self.goff)
        self.paths = self.vector_path(G.views)
        self.launch(G.views, sc)
        out = self.result()
        assert torch.equal(G.read().view(torch.int32), G.before[~G.gap]), "the call changed a gradient"
        return out

    def state_bits(self):
        return [a.read().view(torch.int32) for a in (self.p, self.m, self.v)] + \
            [t.cpu().view(torch.int32) for s in self.sn if s is not None for t in s[:3]]


@functools.lru_cache(maxsize=None)
def _scenario_run(name):
    """Two rounds of (calm_grad_stats, calm_optim_step) of a scenario, the second from the state the first step left:
    per round the checker's verdict, the report's norm with its bound, and the step's own norm with its bound."""
    hip, sc = calm.backend.get_backend(), gf.scenario(name)
    recs, step = tf.optim_state(TABLE), sc["t_prev"]
    dev = StatsDevice(hip, TABLE, recs)
    dev.plan.step_dev.fill_(step)
    sticky, rounds = gs.Sticky(N), []
    for call in (1, 2):
        grads = tf.optim_grads(TABLE, recs, seed=call, scale=sc["grad_scale"] or 1.0)
        ref, bound = gs.reference(recs, grads, gf.hp_of(sc), sc["grad_scale"], step)
        before = dev.state_bits()
        got, summary = dev.stats(grads, sc)
        same = all(torch.equal(a, b) for a, b in zip(before, dev.state_bits()))
        worst, failures = gs.check(got, summary, ref, bound, sticky.after(ref["nonfinite"].numpy()), strict=False)
        show(f"grad stats {name} call {call}", worst)
        o_ref, o_bound = tf.optim_reference(recs, grads, tf.optim_hp(sc), sc["grad_scale"], step)
        after = dev.step(grads, sc)
        norm, e_norm = gs.norm_bound(ref, bound)
        rounds.append(dict(failures=failures, same=same, step=step, dir_sq=got["dir_sq"].copy(), summary=list(summary),
                           norm=math.sqrt(float(np.sum(got["grad_sq"].astype(np.float64)))), ref_norm=norm, e_norm=e_norm,
                           optim_norm=after["norm"], optim_ref=o_ref["norm"], optim_e=o_bound["norm"]))
        recs, step = _state_from(recs, after), after["step"]
    return rounds


@pytest.mark.parametrize("name", gf.SCENARIOS)
def test_scenarios_inside_every_bound(name):
    rounds = _scenario_run(name)
    for r in rounds:
        assert not r["failures"], r["failures"]
    assert [r["summary"] for r in rounds] == [[1, 0, -1, -1], [2, 0, -1, -1]]
    if gf.scenario(name)["t_prev"] == 0:                     # no step applied yet: no direction
        assert rounds[0]["step"] == 0 and not rounds[0]["dir_sq"].any() and rounds[1]["dir_sq"].all()


@pytest.mark.parametrize("name", gf.SCENARIOS)
def test_report_norm_equals_the_norm_of_the_step(name):
    """sqrt(sum grad_sq) against stats_out[0] of calm_optim_step on the same inputs, within the sum of the two checkers'
    norm bounds (each of the two is inside its own bound of the same float64 norm)."""
    for r in _scenario_run(name):
        assert abs(r["ref_norm"] - r["optim_ref"]) <= 1e-12 * r["ref_norm"]
        assert abs(r["norm"] - r["ref_norm"]) <= r["e_norm"] and abs(r["optim_norm"] - r["optim_ref"]) <= r["optim_e"]
        assert abs(r["norm"] - r["optim_norm"]) <= r["e_norm"] + r["optim_e"]


@pytest.mark.parametrize("name", gf.SCENARIOS)
def test_call_writes_nothing_but_its_own_buffers(name):
    """params, moments, u / v / sigma bit for bit (StatsDevice.stats compares the gradients' bits at every call)"""
    assert all(r["same"] for r in _scenario_run(name))


def test_which_access_path_the_two_placements_take(hip):
    """tail_f64's layout: some plain tensor on the 16-byte path, every deferred one on single words; the aligned layout:
    every tensor on the 16-byte path."""
    recs = tf.optim_state(TABLE)
    grads = tf.optim_grads(TABLE, recs, seed=1)
    sn = [e["sn"] is not None for e in TABLE]
    dev = StatsDevice(hip, TABLE, recs)
    paths = dev.vector_path(Arena(grads, dev.goff).views)
    assert any(p and not s for p, s in zip(paths, sn)) and any(not p and not s for p, s in zip(paths, sn))
    assert not any(p for p, s in zip(paths, sn) if s)
    dev = StatsDevice(hip, TABLE, recs, aligned=True)
    assert all(dev.vector_path(Arena(grads, dev.goff).views))


@pytest.mark.parametrize("name", ["below_t2", "scaled_t100000"])
def test_every_tensor_on_the_16_byte_path(hip, name):
    """The table in 16-byte aligned arenas: the deferred tensors (3x32, 200x1, 1x300, 144x288, 300x260 with a chunk
    boundary inside a row, the cancelling 64x48) take the vector path with its row / column walk.  Two calls, the first
    with a NaN inside the 144x288 tensor; gradients, params, moments, u / v / sigma keep their bits."""
    sc, case = gf.scenario(name), tf.optim_nonfinite_cases(TABLE)[1]
    recs, step = tf.optim_state(TABLE), sc["t_prev"] + 1
    dev = StatsDevice(hip, TABLE, recs, aligned=True)
    dev.plan.step_dev.fill_(step)
    sticky, before = gs.Sticky(N), dev.state_bits()
    for call in (1, 2):
        grads = tf.optim_grads(TABLE, recs, seed=call, scale=sc["grad_scale"] or 1.0)
        if call == 1:
            grads[case[1]][case[2]] = case[3]
        ref, bound = gs.reference(recs, grads, gf.hp_of(sc), sc["grad_scale"], step)
        got, summary = dev.stats(grads, sc)
        assert all(dev.paths)
        worst, _ = gs.check(got, summary, ref, bound, sticky.after(ref["nonfinite"].numpy()))
        show(f"grad stats aligned {name} call {call}", worst)
    assert list(summary) == [2, 1, 0, case[1]] and all(torch.equal(a, b) for a, b in zip(before, dev.state_bits()))


def test_two_calls_give_identical_bits(hip):
    sc = gf.scenario("scaled_t100000")
    recs = tf.optim_state(TABLE)
    grads = tf.optim_grads(TABLE, recs, seed=1, scale=sc["grad_scale"])
    dev = StatsDevice(hip, TABLE, recs)
    dev.plan.step_dev.fill_(sc["t_prev"])
    a, sa = dev.stats(grads, sc)
    dev.reset()
    b, sb = dev.stats(grads, sc)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and list(sa) == list(sb) == [1, 0, -1, -1]
    assert a["grad_sq"].all() and a["dir_sq"].all()


@pytest.mark.parametrize("case", tf.optim_nonfinite_cases(TABLE), ids=lambda c: c[0])
def test_non_finite_gradient_is_counted_attributed_and_remembered(hip, case):
    _, tensor, element, value = case
    sc = gf.scenario("clip_t1000")
    recs, step = tf.optim_state(TABLE), sc["t_prev"]
    dev = StatsDevice(hip, TABLE, recs)
    dev.plan.step_dev.fill_(step)
    sticky = gs.Sticky(N)
    grads = tf.optim_grads(TABLE, recs, seed=1)
    grads[tensor][element] = value
    ref, bound = gs.reference(recs, grads, gf.hp_of(sc), None, step)
    got, summary = dev.stats(grads, sc)
    worst, _ = gs.check(got, summary, ref, bound, sticky.after(ref["nonfinite"].numpy()))        # strict: every other tensor too
    show(f"grad stats {case[0]}", worst)
    assert got["nonfinite"][tensor] == 1 and int(got["nonfinite"].sum()) == 1 and list(summary) == [1, 1, 0, tensor]
    # a clean call: the sticky fields stay, nonfinite clears
    grads = tf.optim_grads(TABLE, recs, seed=2)
    ref, bound = gs.reference(recs, grads, gf.hp_of(sc), None, step)
    got, summary = dev.stats(grads, sc)
    gs.check(got, summary, ref, bound, sticky.after(ref["nonfinite"].numpy()))
    assert not got["nonfinite"].any() and got["bad_calls"][tensor] == 1 and got["first_bad_call"][tensor] == 0
    assert list(summary) == [2, 1, 0, tensor]
    dev.reset()
    got, summary = dev.result()
    assert np.array_equal(np.concatenate([got.view(np.int32), summary]), _initial())
    got, summary = dev.stats(grads, sc)
    gs.check(got, summary, ref, bound, gs.Sticky(N).after(ref["nonfinite"].numpy()))


def test_captured_with_the_step_and_replayed_on_new_gradients(hip):
    """calm_grad_stats and calm_optim_step captured into one graph (six sequential launches behind one table upload, no
    parallel branch); three replays, each on new gradients copied into the static arena and on the state the previous
    replay left."""
    sc = gf.scenario("clip_t1000")
    recs, step = tf.optim_state(TABLE), sc["t_prev"]
    dev = StatsDevice(hip, TABLE, recs)
    dev.plan.step_dev.fill_(step)
    goff = [e["goff"] for e in TABLE]
    G = Arena(tf.optim_grads(TABLE, recs, seed=9), goff)
    stats = torch.zeros(2, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dev.launch(G.views, sc)
        hip.optim_step(dev.plan, G.views, tf.optim_hp(sc), None, stats)
    got, summary = dev.result()
    assert list(summary) == [0, 0, -1, -1] and int(dev.plan.step_dev.item()) == step          # a capture runs nothing
    sticky = gs.Sticky(N)
    for replay in (1, 2, 3):
        grads = tf.optim_grads(TABLE, recs, seed=replay)
        fresh = Arena(grads, goff)
        G.buf.copy_(fresh.buf)
        ref, bound = gs.reference(recs, grads, gf.hp_of(sc), None, step)
        graph.replay()
        torch.cuda.synchronize()
        got, summary = dev.result()
        worst, _ = gs.check(got, summary, ref, bound, sticky.after(ref["nonfinite"].numpy()))
        show(f"grad stats replay {replay}", worst)
        assert torch.equal(G.buf.cpu().view(torch.int32), fresh.before), "the replay changed the static gradient arena"
        after = dict(p=dev.p.read(), m=dev.m.read(), v=dev.v.read())
        recs, step = _state_from(recs, after), int(dev.plan.step_dev.item())
        assert step == sc["t_prev"] + replay
    assert list(summary) == [3, 0, -1, -1]


# ---- model level ---------------------------------------------------------------------------------------------------------
RULES = [("*ls_*", {"lr_scale": 0.1}), (lambda name, p: p.ndim <= 1, {"weight_decay": 0.0})]


def _two_steps(attach, window):
    """Two optimizer steps of tiny32_cls (windows of two micro-batches with `window`) -> the parameters, and with
    `attach` the report, the float64 norm with its bounds and the step's own norm of the last step."""
    _, x, y = _batch(NAME, bs=8)
    xs, y = [x.cuda(), x.cuda().flip(0)], y.cuda()
    m = build_model(NAME, load_golden(NAME), "cuda").train()
    cls = trainer.FusedClipAdamWindow if window else trainer.FusedClipAdamW
    opt = cls(m, groups=trainer.param_groups(m, RULES)[0])
    step = trainer.AccumTrainStep(m, opt, accumulate=2) if window else trainer.TrainStep(m, opt)
    seen, report = [], None
    try:
        if attach:
            mon = trainer.GradMonitor(m, opt).attach()
            assert mon.native
            real = mon.observe

            def spy(plan, grads, divisor, records):
                flat = lambda t: t.detach().cpu().clone().reshape(-1)         # noqa: E731
                recs = [dict(param=flat(r["param"]), exp_avg=flat(r["exp_avg"]), exp_avg_sq=flat(r["exp_avg_sq"]),
                             sn=None if r["sn"] is None else tuple(flat(t) if torch.is_tensor(t) else t for t in r["sn"]))
                        for r in records]
                seen[:] = [(recs, [flat(g) for g in grads], None if divisor is None else float(divisor),
                            int(plan.step_dev.item()), opt._hparams())]
                real(plan, grads, divisor, records)

            mon.observe = spy
        for k in range(4 if window else 2):
            calm.ops.set_noise_override(W.NoiseStream(70 + k))
            step(xs[k % 2], y)
        torch.cuda.synchronize()
        if attach:
            recs, grads, divisor, t, hp = seen[0]
            ref, bound = gs.reference(recs, grads, hp, divisor, t)
            got, summary = mon._views(mon._buf.cpu().numpy())
            gs.check(got, summary, ref, bound, gs.Sticky(mon.n).after([0] * mon.n).after([0] * mon.n))
            o_ref, o_bound = tf.optim_reference(recs, grads, hp, divisor, t)
            report = dict(rep=mon.read(), norm=gs.norm_bound(ref, bound), optim=(float(opt.stats[0]), o_ref["norm"], o_bound["norm"]), t=t)
        assert opt.step_count == 2
    finally:
        calm.ops.set_noise_override(None)
        opt.close()
    return [p.detach().clone() for p in opt.params], report


@pytest.mark.parametrize("window", [False, True], ids=["eager", "accumulate-2"])
def test_monitor_leaves_the_parameters_bit_equal_and_reports_the_norm_of_the_step(hip, window):
    prev = hip.gemm_set_option(hip.GEMM_OPT_DETERMINISTIC, 1)
    try:
        plain, _ = _two_steps(False, window)
        watched, r = _two_steps(True, window)
    finally:
        hip.gemm_set_option(hip.GEMM_OPT_DETERMINISTIC, prev)
    for a, b in zip(plain, watched):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    rep, (norm, e_norm), (o_got, o_ref, o_e) = r["rep"], r["norm"], r["optim"]
    assert r["t"] == 1 and rep["calls"] == 2 and rep["skipped"] == 0 and rep["first_bad"] is None and len(rep["groups"]) == 3
    assert abs(rep["norm"] - norm) <= e_norm and abs(o_got - o_ref) <= o_e
    assert abs(rep["norm"] - o_got) <= e_norm + o_e
    assert all(g["update_ratio"] > 0 and g["grad_norm"] > 0 and g["weight_norm"] > 0 for g in rep["groups"])


def test_train_with_a_monitor_and_a_captured_step_writes_the_log(tmp_path):
    cfg = CONFIGS[NAME]
    S = cfg.seq_length
    gen = torch.Generator().manual_seed(0)
    data = torch.utils.data.TensorDataset(torch.randint(0, 256, (16, 3, S + 4, S + 4), generator=gen, dtype=torch.uint8),
                                          torch.randint(0, cfg.out_features, (16,), generator=gen))
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    m = build_model(NAME, load_golden(NAME), "cpu")
    out = trainer.train(m, "fused", scheduler=None, use_gpu=True, dataset=data, epochs=1, batch_size=4,
                        num_classes=cfg.out_features, device_collate=True, crop=(S, S), log_every=1000, max_steps=2,
                        checkpoint_path=str(tmp_path / "model.pth"), graph=True, monitor={"every": 1, "per_tensor": True})
    with open(tmp_path / "model_grad.jsonl") as f:
        lines = [json.loads(line) for line in f]
    # the captured step's warm-up is not counted: a line behind each of the two steps, and the epoch's
    assert [(e["epoch"], e["step"], e["calls"]) for e in lines] == [(1, 1, 1), (1, 2, 2), (1, 2, 2)]
    mon = out._calm_monitor
    assert set(lines[2]["tensors"]) == set(mon.names) and "tensors" not in lines[0]
    assert all(e["skipped"] <= e["calls"] and len(e["top_grad_norm"]) == 8 for e in lines)
    rep = mon.read()
    assert rep["calls"] == 2 and (rep["skipped"] > 0 or rep["norm"] > 0)
