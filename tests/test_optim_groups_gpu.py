"""calm_optim_step_groups of libcalmvit_hip.so: bit-equal to calm_optim_step where the groups do not differ, inside the
per-group float64 bounds (tests/optim_groups_f64.py) where they do, skipped as a whole on a non-finite gradient, captured
into a hipGraph with the rates following the device table; then FusedClipAdamW / FusedClipAdamWindow / GraphedTrainStep
with groups on tiny32_cls, and train(param_groups=) on one GPU.  tests/test_optim_groups_cpu.py proves the checker on the
torch fallback and on planted faults.  The table is tail_f64.optim_table(): the smallest at which chunking, the deferred
correction and the group lookup can each go wrong."""
from importlib import import_module

import pytest
import torch

import calm_vit_dte_amd as calm
import optim_groups_f64 as gf
import tail_f64 as tf
import weights as W
from helpers import CONFIGS, load_golden, rel_err
from test_host_logic_cpu import build_model
from test_rowwise_f64_gpu import Out, place
from test_tail_f64_gpu import Arena, Device, _state_from, show
from test_trainer_gpu import _batch

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
TABLE = tf.optim_table()
GROUPS = gf.table_groups(TABLE)
NAME = "tiny32_cls"
RULES = [("*ls_*", {"lr_scale": 0.1}), (lambda name, p: p.ndim <= 1, {"weight_decay": 0.0})]     # three groups with the base


@pytest.fixture(scope="module")
def hip():
    return calm.backend.get_backend()


class GroupedDevice(Device):
    """tail_f64's device state with a plan whose records carry their group."""

    def __init__(self, hip, table, recs, groups, n_groups):
        super().__init__(hip, table, recs)
        self.plan = hip.optim_plan([dict(param=p, exp_avg=m, exp_avg_sq=v, sn=s, group=g) for p, m, v, s, g in
                                    zip(self.p.views, self.m.views, self.v.views, self.sn, groups)], n_groups=n_groups)

    def step_groups(self, grads, sc, group_hp):
        G = Arena(grads, [e["goff"] for e in self.table])
        stats = Out((2,))
        gs = place(torch.tensor([sc["grad_scale"]])) if sc["grad_scale"] else None
        self.hip.optim_step_groups(self.plan, G.views, gf.hp_of(sc), group_hp, gs, stats.t)
        st = stats.check()
        G.read()
        return self.read(st)

    def read(self, st):
        return dict(p=self.p.read(), m=self.m.read(), v=self.v.read(), norm=float(st[0]), found_inf=float(st[1]),
                    step=int(self.plan.step_dev.item()))


def _assert_same_bits(a, b, label):
    for k in ("p", "m", "v"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{label}: {k} differs"
    one = lambda x: torch.tensor([x], dtype=torch.float32).view(torch.int32)  # noqa: E731
    assert torch.equal(one(a["norm"]), one(b["norm"])) and (a["found_inf"], a["step"]) == (b["found_inf"], b["step"]), label


@pytest.mark.parametrize("n_groups", [1, 3], ids=["one-group", "three-equal-groups"])
@pytest.mark.parametrize("name", gf.SCENARIOS)
def test_equal_rates_give_the_bits_of_calm_optim_step(hip, name, n_groups):
    """One group, and three groups with identical (lr, weight_decay): p, m, v, stats_out and step_dev of two consecutive
    calls equal calm_optim_step's bit for bit — the lookup changes no arithmetic."""
    sc = gf.scenario(name)
    recs = tf.optim_state(TABLE)
    plain = Device(hip, TABLE, recs)
    grouped = GroupedDevice(hip, TABLE, recs, [g % n_groups for g in GROUPS], n_groups)
    for d in (plain, grouped):
        d.plan.step_dev.fill_(sc["t_prev"])
    for call in (1, 2):
        grads = tf.optim_grads(TABLE, recs, seed=call, scale=sc["grad_scale"] or 1.0)
        want = plain.step(grads, sc)
        got = grouped.step_groups(grads, sc, [(tf.OPT_LR, sc["wd"])] * n_groups)
        _assert_same_bits(got, want, f"{name} call {call}")
    assert got["step"] == sc["t_prev"] + 2 and got["found_inf"] == 0.0


@pytest.mark.parametrize("name", gf.SCENARIOS)
def test_three_groups_and_an_empty_fourth_against_the_per_group_reference(hip, name):
    sc = gf.scenario(name)
    recs, step = tf.optim_state(TABLE), sc["t_prev"]
    dev = GroupedDevice(hip, TABLE, recs, GROUPS, len(gf.GROUP_HP))
    dev.plan.step_dev.fill_(step)
    frozen = gf.element_groups(recs, GROUPS) == 2
    for call in (1, 2):
        grads = tf.optim_grads(TABLE, recs, seed=call, scale=sc["grad_scale"] or 1.0)
        ref, bound = gf.grouped_reference(recs, grads, sc, gf.GROUP_HP, GROUPS, step)
        before = tf.optim_flat(recs)
        got = dev.step_groups(grads, sc, gf.GROUP_HP)
        worst, failures = tf.check_optim(got, ref, bound, strict=False)
        show(f"grouped optim {name} call {call}", worst)
        assert not failures, failures
        # lr = 0: every parameter of the group keeps its bits while its moments move
        assert torch.equal(got["p"][frozen].view(torch.int32), before["p"][frozen].view(torch.int32))
        assert not torch.equal(got["m"][frozen], before["m"][frozen]) and not torch.equal(got["v"][frozen], before["v"][frozen])
        recs, step = _state_from(recs, got), got["step"]
    assert step == sc["t_prev"] + 2


@pytest.mark.parametrize("case", tf.optim_nonfinite_cases(TABLE), ids=lambda c: c[0])
def test_grouped_step_skipped_on_non_finite_gradient(hip, case):
    _, tensor, element, value = case
    sc = gf.scenario("clip_t1000")
    recs = tf.optim_state(TABLE)
    grads = tf.optim_grads(TABLE, recs, seed=1)
    grads[tensor][element] = value
    dev = GroupedDevice(hip, TABLE, recs, GROUPS, len(gf.GROUP_HP))
    dev.plan.step_dev.fill_(sc["t_prev"])
    tf.check_optim_skipped(dev.step_groups(grads, sc, gf.GROUP_HP), tf.optim_flat(recs), sc["t_prev"])


def test_captured_grouped_step_follows_the_rewritten_group_table(hip):
    """One grouped step captured with the OLD rates in the table (three sequential launches, no parallel branch); the
    table is then rewritten the way sync_lr_to_device does it, and the replay equals the eager call with the NEW rates."""
    sc = gf.scenario("clip_t1000")
    recs = tf.optim_state(TABLE)
    grads = tf.optim_grads(TABLE, recs, seed=1)
    old = [(2 * lr + 1e-4, wd) for lr, wd in gf.GROUP_HP]
    eager = GroupedDevice(hip, TABLE, recs, GROUPS, len(gf.GROUP_HP))
    eager.plan.step_dev.fill_(sc["t_prev"])
    want = eager.step_groups(grads, sc, gf.GROUP_HP)
    dev = GroupedDevice(hip, TABLE, recs, GROUPS, len(gf.GROUP_HP))
    dev.plan.step_dev.fill_(sc["t_prev"])
    G = Arena(grads, [e["goff"] for e in TABLE])
    stats = torch.zeros(2, device="cuda")
    assert dev.plan.groups.set(old)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.optim_step_groups(dev.plan, G.views, gf.hp_of(sc), old, None, stats)
    assert int(dev.plan.step_dev.item()) == sc["t_prev"]              # a capture runs nothing
    assert dev.plan.groups.set(gf.GROUP_HP) and not dev.plan.groups.set(gf.GROUP_HP)     # written once, then unchanged
    graph.replay()
    torch.cuda.synchronize()
    G.read()
    _assert_same_bits(dev.read(stats.cpu()), want, "replay with rewritten rates")


# ---- model level ---------------------------------------------------------------------------------------------------------
def _model(groups=True, window=False, **kw):
    m = build_model(NAME, load_golden(NAME), "cuda").train()
    cls = trainer.FusedClipAdamWindow if window else trainer.FusedClipAdamW
    return m, cls(m, groups=trainer.param_groups(m, RULES)[0] if groups else None, **kw)


def _updates_agree(params, twins, starts):
    """The bar of test_trainer_gpu.test_fused_optimizer_side_step_matches_clip_plus_adamw: per element, with 0.1 % of
    outliers allowed (Adam's first update is lr * g / (|g| + eps): an element with a gradient of ~0 flips)."""
    bad = tot = 0
    for p, t, s in zip(params, twins, starts):
        bad += int((((p - s) - (t - s)).abs() > 1e-3 * 3.1e-3 + 1e-7).sum())
        tot += p.numel()
    assert bad <= 1e-3 * tot, (bad, tot)


def test_grouped_fused_step_equals_the_torch_fallback_on_identical_gradients():
    _, x, y = _batch(NAME, bs=8)
    x, y = x.cuda(), y.cuda()
    m, opt = _model()
    step = trainer.TrainStep(m, opt)
    try:
        assert opt.grouped and len(opt.param_groups) == 3 and opt._plan.n_groups == 3
        starts = [p.detach().clone() for p in opt.params]
        twin = [dict(r, param=r["param"].clone(), exp_avg=r["exp_avg"].clone(), exp_avg_sq=r["exp_avg_sq"].clone())
                for r in opt._records]
        t_step, t_stats = opt._plan.step_dev.clone(), torch.zeros(2, device="cuda")
        for k in range(2):
            calm.ops.set_noise_override(W.NoiseStream(40 + k))
            y_hat, _ = m(x)
            step._backward(step._loss(y_hat, y))
            grads = [g.clone() for g in opt._contiguous_grads(keep=True)]
            hp = (0.5, opt.betas[0], opt.betas[1], opt.eps, 0.9, 1.0, 0)
            trainer.optim_step_groups_torch(twin, t_step, grads, hp, opt.group_hparams(), None, t_stats)
            opt.step()
            assert abs(float(opt.stats[0]) - float(t_stats[0])) <= 1e-4 * float(t_stats[0]) and float(opt.stats[1]) == 0.0
            _updates_agree([p.detach() for p in opt.params], [r["param"] for r in twin], starts)
            for g in opt.param_groups:                   # what a scheduler's step() does
                g["lr"] *= 0.5
        assert opt.step_count == int(t_step) == 2
        for r, t in zip(opt._records, twin):
            assert rel_err(r["exp_avg_sq"], t["exp_avg_sq"]) < 1e-3
    finally:
        calm.ops.set_noise_override(None)
        opt.close()


def test_grouped_window_of_two_equals_the_eager_grouped_step_on_the_mean_gradient():
    _, x, y = _batch(NAME, bs=8)
    xs = [x.cuda(), x.cuda().flip(0)]
    y = y.cuda()
    m_w, opt_w = _model(window=True)
    m_e, opt_e = _model(defer_sn=False)                 # its backward corrects every micro-batch's gradient itself
    step_w, step_e = trainer.AccumTrainStep(m_w, opt_w, accumulate=2), trainer.TrainStep(m_e, opt_e)
    try:
        starts = [p.detach().clone() for p in opt_e.params]
        for k, xk in enumerate(xs):
            calm.ops.set_noise_override(W.NoiseStream(50 + k))
            step_w(xk, y)
            calm.ops.set_noise_override(W.NoiseStream(50 + k))
            y_hat, _ = m_e(xk)
            step_e._loss(y_hat, y).backward()            # autograd sums into .grad
        assert step_w.boundary and opt_w.step_count == 1
        torch._foreach_mul_([p.grad for p in opt_e.params], 0.5)
        opt_e.step()
        _updates_agree([p.detach() for p in opt_w.params], [p.detach() for p in opt_e.params], starts)
        assert abs(float(opt_w.stats[0]) - float(opt_e.stats[0])) <= 1e-3 * float(opt_e.stats[0])
    finally:
        calm.ops.set_noise_override(None)
        opt_w.close()
        opt_e.close()


def _scaled_run(graphed, n, scales, y, x):
    """test_trainer_gpu._scaled_run with parameter groups: every group's rate is its initial one times scales[i]."""
    m, opt = _model()
    scaler = torch.amp.GradScaler("cuda", init_scale=256.0, growth_interval=2000)
    base = [g["lr"] for g in opt.param_groups]
    try:
        if graphed:
            step = trainer.GraphedTrainStep(m, opt, x, y, warmup=1, scaler=scaler, autocast_dtype=torch.bfloat16)
        else:
            step = trainer.TrainStep(m, opt, None, scaler=scaler, autocast_dtype=torch.bfloat16)
            step(x, y)                                    # the graphed run's warm-up step
        for i in range(n):
            for g, lr in zip(opt.param_groups, base):     # what a scheduler's step() does
                g["lr"] = lr * scales[i]
            step(x, y)
        torch.cuda.synchronize()
        assert opt.step_count == n + 1
    finally:
        opt.close()
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def test_graphed_grouped_step_follows_a_schedule_of_every_group_without_recapture():
    """The pattern and the bound of test_trainer_gpu.test_graphed_step_follows_a_learning_rate_schedule_without_recapture."""
    _, x, y = _batch(NAME, bs=8)
    x, y = x.cuda(), y.cuda()
    scales = [1.0, 1.0, 0.3, 0.3, 0.06, 3e-4]
    sd_e = _scaled_run(False, len(scales), scales, y, x)
    sd_g = _scaled_run(True, len(scales), scales, y, x)
    sd_c = _scaled_run(True, len(scales), [1.0] * len(scales), y, x)
    worst = max(rel_err(sd_g[k].float(), sd_e[k].float()) for k in sd_e)
    moved = max(rel_err(sd_c[k].float(), sd_e[k].float()) for k in sd_e)
    assert worst < 5e-2, worst
    assert moved > 4 * worst, (moved, worst)


# ---- train() on one GPU -----------------------------------------------------------------------------------------------------
FROZEN_RULES = [("*inv_freq", {"frozen": True})] + RULES


def _train(tmp, tag, seed, **kw):
    cfg = CONFIGS[NAME]
    S = cfg.seq_length
    gen = torch.Generator().manual_seed(0)
    data = torch.utils.data.TensorDataset(torch.randint(0, 256, (16, 3, S + 4, S + 4), generator=gen, dtype=torch.uint8),
                                          torch.randint(0, cfg.out_features, (16,), generator=gen))
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    m = build_model(NAME, load_golden(NAME), "cpu")
    if seed != 11:                                  # a resumed run starts from other weights: only the load can make it equal
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(1.01)
    path = str(tmp / f"{tag}.snap")
    out = trainer.train(m, "fused", scheduler=None, use_gpu=True, dataset=data, epochs=2, batch_size=4,
                        num_classes=cfg.out_features, device_collate=True, crop=(S, S), log_every=1000, snapshot_path=path,
                        param_groups=FROZEN_RULES, scheduler_step="step", **kw)
    return out, path


def test_train_with_groups_resumes_exactly_and_leaves_frozen_parameters_alone(tmp_path):
    from test_snapshot_gpu import _parts
    be = calm.backend.get_backend()
    prev = be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, 1)
    try:
        a, file_a = _train(tmp_path, "a", 11)
        _, file_b = _train(tmp_path, "b", 11, max_steps=3, snapshot_every=3)
        host = trainer.TrainState.read_header(file_b)[0]["host"]
        assert host["progress"] == {"epoch": 0, "batch": 3, "step": 3} and len(host["lrs"]) == 3
        c, file_c = _train(tmp_path, "c", 12, resume=file_b)
    finally:
        be.gemm_set_option(be.GEMM_OPT_DETERMINISTIC, prev)
    sa, sc = a.state_dict(), c.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sc[k]), f"resumed run differs at {k}"
    (ha, pa), (hc, pc) = _parts(file_a), _parts(file_c)
    assert ha["entries"] == hc["entries"] and pa == pc and ha["crc32"] == hc["crc32"] and ha["host"] == hc["host"]
    assert ha["host"]["progress"] == {"epoch": 2, "batch": 0, "step": 8} and ha["host"]["scheduler"]["last_epoch"] == 8
    first = build_model(NAME, load_golden(NAME), "cpu").state_dict()
    frozen = [k for k in sa if k.endswith("inv_freq")]
    assert frozen and all(torch.equal(sa[k].view(torch.int32), first[k].view(torch.int32)) for k in frozen)
    assert all(p.grad is None and not p.requires_grad for n, p in a.named_parameters() if n.endswith("inv_freq"))
    assert any(not torch.equal(sa[k], first[k]) for k in sa if k.endswith("weight_orig"))
