"""calm_optim_step_lamb of libcalmvit_hip.so against the float64 checker (tests/lamb_f64.py) on tail_f64.optim_table() — the
smallest table at which the chunk walk, the deferred correction with its cancelling tensor, the row-split chunks, the
per-tensor sums over several chunks and the two access paths can each go wrong — once where tail_f64's arenas put the tensors
and once with every tensor 16-byte aligned; then FusedClipAdamW(lamb=) on tiny32_cls against a hand-written loop over
backend.optim_step_lamb, a captured step, and train(lamb=).  tests/test_lamb_cpu.py proves the checker on an fp32 emulation and
on planted faults.  Parameters, moments, scratch, stats_out and trust_out sit between NaN-pattern guards; every input arena
must come back bit for bit.  The inf / NaN of the non-finite cases are values planted in input data."""
from importlib import import_module

import pytest
import torch

import calm_vit_dte_amd as calm
import lamb_f64 as lf
import tail_f64 as tf
import weights as W
from helpers import CONFIGS, load_golden
from test_grad_stats_gpu import StatsDevice
from test_host_logic_cpu import build_model
from test_rowwise_f64_gpu import Out, place
from test_sam_gpu import _scale_update
from test_tail_f64_gpu import Arena, show
from test_trainer_gpu import _batch

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
TABLE = lf.TABLE
N = len(TABLE)
NAME = "tiny32_cls"
RUN_IDS = [f"{n}-{'grouped' if g else 'one'}-{m}" for n, g, m in lf.RUNS]
NONFINITE = [c[0] for c in tf.optim_nonfinite_cases(TABLE)]


@pytest.fixture(scope="module")
def hip():
    return calm.backend.get_backend()


def _aligned(t):
    return t.data_ptr() % 16 == 0


class LambDevice(StatsDevice):
    """tail_f64's device state (aligned: every tensor on a multiple of 16 bytes) with the plan of a case — its groups, if it
    has any — and the buffers of the entry point between guards: scratch, stats_out, trust_out."""

    def __init__(self, hip, c, aligned=False, trust_init=None):
        super().__init__(hip, TABLE, c["recs"], aligned=aligned)
        if c["groups"] is not None:
            self.plan = hip.optim_plan([dict(param=p, exp_avg=m, exp_avg_sq=v, sn=s, group=g) for p, m, v, s, g in
                                        zip(self.p.views, self.m.views, self.v.views, self.sn, c["groups"])], n_groups=len(c["group_hp"]))
        self.plan.step_dev.fill_(c["step"])
        self.lamb_scratch = Out((hip.lamb_scratch_floats(self.plan),))
        assert self.lamb_scratch.t.numel() == 6 * N + 4 + 5 * self.plan.n_chunks
        self.stats = Out((2,))
        self.trust = Out((N, 3), init=trust_init)

    def step(self, c, applied=True):
        """one call -> what lamb_f64.check takes; every guard and every input is compared on the way"""
        G = Arena(c["grads"], self.goff)
        quads = list(zip(G.views, self.p.views, self.m.views, self.v.views))
        self.paths3 = [all(_aligned(t) for t in q) for q in quads]              # pass 3: grad, param, both moments
        self.paths4 = [all(_aligned(t) for t in q[1:]) for q in quads]          # pass 4: param, both moments
        inputs = self.state_bits()[3:]                                           # u / v / sigma
        gs = place(torch.tensor([c["scale"]])) if c["scale"] else None
        lr_dev = place(torch.tensor([c["lr_dev"]])) if c["lr_dev"] is not None else None
        self.hip.optim_step_lamb(self.plan, G.views, c["hp"], c["lamb_hp"], gs, self.stats.t, group_hp=c["group_hp"],
                                 lr_dev=lr_dev, scratch=self.lamb_scratch.t, trust_out=self.trust.t)
        st = self.stats.check()
        self.lamb_scratch.check(written=False)
        trust = self.trust.check(written=applied)             # an applied step writes every row
        assert torch.equal(G.read().view(torch.int32), G.before[~G.gap]), "the call changed a gradient"
        assert all(torch.equal(a, b) for a, b in zip(inputs, self.state_bits()[3:])), "the call changed u / v / sigma"
        return dict(p=self.p.read(), m=self.m.read(), v=self.v.read(), norm=float(st[0]), found_inf=float(st[1]),
                    step=int(self.plan.step_dev.item()), trust=trust.clone())


@pytest.mark.parametrize("aligned", [False, True], ids=["tail-layout", "aligned16"])
@pytest.mark.parametrize("name,grouped,mode", lf.RUNS, ids=RUN_IDS)
def test_every_result_inside_every_bound(hip, name, grouped, mode, aligned):
    c = lf.case(name, grouped, mode)
    dev = LambDevice(hip, c, aligned=aligned)
    got = dev.step(c)
    if aligned:
        assert all(dev.paths3) and all(dev.paths4)
    else:                                                    # some tensors on each path where tail_f64 puts them
        assert any(dev.paths3) and not all(dev.paths3) and any(dev.paths4) and not all(dev.paths4)
    worst, failures = lf.check(got, c["ref"], c["bound"], strict=False)
    w_len, f_len, checked = lf.check_length(got, c["ref"], c["bound"], strict=False)
    show(f"lamb {name} {'grouped' if grouped else 'one'} {mode} {'aligned' if aligned else 'tail layout'}", {**worst, **w_len})
    assert not failures and not f_len, (failures, f_len)
    assert got["step"] == c["step"] + 1
    if mode == "always":
        # LAMB's defining property on EVERY tensor with positive norms: ||w_after - w_before||_2 = lr_t ||w||
        assert checked == sum(1 for a, b in zip(c["ref"]["wn"], c["ref"]["un"]) if a > 0 and b > 0) >= N - 2


@pytest.mark.parametrize("aligned", [False, True], ids=["tail-layout", "aligned16"])
@pytest.mark.parametrize("grouped", [False, True], ids=["one", "grouped"])
@pytest.mark.parametrize("nonfinite", NONFINITE)
def test_step_skipped_on_a_non_finite_gradient(hip, nonfinite, grouped, aligned):
    c = lf.case("clip_t1000", grouped, "always_clip", nonfinite)
    before = torch.rand(N, 3, generator=tf.gen(3))
    dev = LambDevice(hip, c, aligned=aligned, trust_init=before)
    got = dev.step(c, applied=False)
    lf.check_skipped(got, tf.optim_flat(c["recs"]), c["step"], before)


@pytest.mark.parametrize("aligned", [False, True], ids=["tail-layout", "aligned16"])
def test_two_calls_and_another_stream_give_identical_bits(hip, aligned):
    c = lf.case("scaled_t100000", True, "always_clip")
    a = LambDevice(hip, c, aligned=aligned).step(c)
    b = LambDevice(hip, c, aligned=aligned).step(c)
    other = LambDevice(hip, c, aligned=aligned)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s = other.step(c)
    side.synchronize()
    for o in (b, s):
        assert (a["norm"], a["found_inf"], a["step"]) == (o["norm"], o["found_inf"], o["step"])
        for k in ("p", "m", "v", "trust"):
            assert torch.equal(a[k].view(torch.int32), o[k].view(torch.int32)), k
    assert a["found_inf"] == 0.0 and not torch.equal(a["p"], tf.optim_flat(c["recs"])["p"])


def test_passes_1_and_2_have_the_bits_of_calm_optim_step(hip):
    """The norm, found_inf and the step count of a LAMB call and of calm_optim_step on the same state: the same kernels."""
    c = lf.case("clip_t1000", False, "plain")
    got = LambDevice(hip, c).step(c)
    plain = StatsDevice(hip, TABLE, c["recs"])
    plain.plan.step_dev.fill_(c["step"])
    want = plain.step(c["grads"], c["sc"])
    one = lambda x: torch.tensor([x], dtype=torch.float32).view(torch.int32)  # noqa: E731
    assert torch.equal(one(got["norm"]), one(want["norm"])) and (got["found_inf"], got["step"]) == (want["found_inf"], want["step"])
    assert want["found_inf"] == 0.0 and want["step"] == c["step"] + 1


# ---- model level ---------------------------------------------------------------------------------------------------------
def _three_steps(hip, hand, autocast):
    """Three LAMB steps of tiny32_cls under a GradScaler and an EMA: TrainStep over FusedClipAdamW(lamb=True), or the same
    from public pieces — forward, backward, backend.optim_step_lamb on the optimizer's plan, the EMA, the scale update."""
    _, x, y = _batch(NAME, bs=8)
    xs, y = [x.cuda(), x.cuda().flip(0)], y.cuda()
    m = build_model(NAME, load_golden(NAME), "cuda").train()
    opt = trainer.FusedClipAdamW(m, lamb=True)
    ema = trainer.ModelEMA(m, 0.9)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    dtype = torch.bfloat16 if autocast else None
    trace, clean = [], 0
    try:
        one = torch.ones((), device="cuda")
        step = trainer.TrainStep(m, opt, scaler=scaler, autocast_dtype=dtype, ema=ema)
        for k in range(3):
            calm.ops.set_noise_override(W.NoiseStream(70 + k))
            if hand:
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    loss = trainer.soft_target_cross_entropy(m(xs[k % 2])[0].squeeze(), y)
                with calm.ops.grad_tail(opt.params, enabled=True):
                    scaler.scale(loss).backward()
                loss = loss.detach()
                scale = scaler.scale(one)
                hip.optim_step_lamb(opt._plan, opt._contiguous_grads(keep=True), opt._hparams(), (None, False), scale, opt.stats)
                for p in opt.params:
                    p.grad = None
                ema.update(skip=opt.stats[1:2])
                clean = _scale_update(scaler, scale, bool(opt.stats[1] > 0), clean)
            else:
                loss, _ = step(xs[k % 2], y)
            torch.cuda.synchronize()
            bits = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).view(torch.int32).cpu()      # noqa: E731
            trace.append((loss.cpu(), bits(opt.params), bits(opt.exp_avg), bits(ema.shadows), float(scaler.get_scale()),
                          float(opt.stats[1]), bits([opt._plan.lamb_trust])))
        assert opt.step_count == 3 - sum(t[5] for t in trace)
        ratios = opt.trust_ratios()
        assert list(ratios) == opt.param_names and any(v[2] != 1.0 for v in ratios.values())
    finally:
        calm.ops.set_noise_override(None)
        opt.close()
    return trace


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast-bf16"])
def test_train_step_with_lamb_equals_the_hand_written_loop_bit_for_bit(hip, autocast):
    prev = hip.gemm_set_option(hip.GEMM_OPT_DETERMINISTIC, 1)
    try:
        a = _three_steps(hip, False, autocast)
        b = _three_steps(hip, True, autocast)
    finally:
        hip.gemm_set_option(hip.GEMM_OPT_DETERMINISTIC, prev)
    for k, (s, h) in enumerate(zip(a, b)):
        assert torch.equal(s[0], h[0]), f"step {k}: the loss"
        assert all(torch.equal(s[i], h[i]) for i in (1, 2, 3, 6)), f"step {k}: parameters, moments, the EMA or the trust table differ"
        assert s[4:6] == h[4:6], f"step {k}: scale / found_inf"
    assert any(t[5] == 0.0 for t in a) and not torch.equal(a[0][1], a[2][1])      # at least one step was applied


def _data(n=16, seed=0, u8=True):
    cfg = CONFIGS[NAME]
    S = cfg.seq_length
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, 3, S + 4, S + 4), generator=gen, dtype=torch.uint8) if u8 else torch.randn(n, 3, S, S, generator=gen)
    return torch.utils.data.TensorDataset(x, torch.randint(0, cfg.out_features, (n,), generator=gen))


def _train(data, **kw):
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    m = build_model(NAME, load_golden(NAME), "cpu")
    return trainer.train(m, "fused", use_gpu=True, dataset=data, epochs=1, num_classes=CONFIGS[NAME].out_features, log_every=1000,
                         **kw)


def test_a_captured_lamb_step_replays_the_eager_trajectory_under_a_per_step_schedule(hip):
    """train(graph=True, lamb=True) with a cosine schedule that moves at every optimizer step: the replays read the rate from
    the device scalar, and four of them leave exactly the model four eager steps leave (deterministic GEMM mode)."""
    data = _data(32, seed=3, u8=False)
    prev = hip.gemm_set_option(hip.GEMM_OPT_DETERMINISTIC, 1)
    try:
        outs = [_train(data, scheduler=None, scheduler_step="step", batch_size=8, graph=graph, lamb=True) for graph in (False, True)]
    finally:
        hip.gemm_set_option(hip.GEMM_OPT_DETERMINISTIC, prev)
    eager, replay = (o.state_dict() for o in outs)
    assert all(torch.equal(eager[k], replay[k]) for k in eager), [k for k in eager if not torch.equal(eager[k], replay[k])][:5]
    assert outs[0]._calm_lamb.trust_ratios() == outs[1]._calm_lamb.trust_ratios()
    assert outs[1]._calm_lamb.step_count == 4 and outs[1]._calm_lamb.lr < 3.1e-3      # the schedule moved the rate


def test_train_with_lamb_groups_a_monitor_and_the_device_collate(capsys):
    S = CONFIGS[NAME].seq_length
    out = _train(_data(), scheduler=None, batch_size=4, device_collate=True, crop=(S, S), max_steps=3,
                 lamb={"trust_clip": 10.0}, param_groups="no_decay", monitor=True)
    assert all(bool(torch.isfinite(p).all()) for p in out.parameters())
    opt = out._calm_lamb
    assert opt is out._calm_monitor.optimizer and opt.lamb == {"trust_clip": 10.0, "always_adapt": False}
    ratios = opt.trust_ratios()
    decay = {n: g["weight_decay"] for g in opt.param_groups for n, p in zip(opt.param_names, opt.params) if any(p is q for q in g["params"])}
    assert set(decay) == set(ratios) and any(wd == 0.0 for wd in decay.values()) and any(wd != 0.0 for wd in decay.values())
    if float(opt.stats[1]) == 0.0 or any(v[:2] != (0.0, 0.0) for v in ratios.values()):      # a step was applied
        assert all(ratios[n][2] == 1.0 for n, wd in decay.items() if wd == 0.0)
        assert all(0.0 < ratios[n][2] <= 10.0 for n, wd in decay.items() if wd != 0.0)
        assert any(ratios[n][2] != 1.0 for n, wd in decay.items() if wd != 0.0)
    text = capsys.readouterr().out
    assert "LAMB: per-tensor trust ratios on, trust_clip 10.0, always_adapt False" in text
    assert "Trust ratio min / median / max:" in text


@pytest.mark.parametrize("kw", [dict(sam=0.05), dict(accumulate=2)], ids=["sam", "accumulate"])
def test_train_with_lamb_under_sam_and_under_a_window(kw):
    data = _data(32)
    S = CONFIGS[NAME].seq_length
    common = dict(scheduler=None, batch_size=4, device_collate=True, crop=(S, S), max_steps=3, **kw)
    lamb, plain = _train(data, lamb=True, **common), _train(data, **common)
    assert all(bool(torch.isfinite(p).all()) for p in lamb.parameters())
    assert isinstance(lamb._calm_lamb, trainer.FusedClipAdamWindow) and not hasattr(plain, "_calm_lamb")
    assert any(not torch.equal(a, b) for a, b in zip(lamb.parameters(), plain.parameters()))
