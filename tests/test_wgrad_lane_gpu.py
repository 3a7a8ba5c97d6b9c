"""The side lane of calm_gemm on the MI355X (include/calm_vit.h: calm_gemm_lane / _fork / _join; csrc/gemm_lane.h): the
weight-gradient GEMMs of a backward on a second, lowest-priority stream of the library's, joined before the backward ends.

  library   fork + lane launch + join against the plain call: bit-identical, the float64 product, nothing outside the
            output, operands produced on the main stream right before the fork, result read right after the join
  model     nano48, TrainStep + FusedClipAdamW, deterministic k-split: lane on == lane off in every bit of the state
  drop      a backward that raises after weight gradients went to the lane leaves the lane joined and the next step right
  capture   GraphedTrainStep with the switch on captures, replays, and equals the eager lane-off run: the lane is off
            inside a capture

Operands are integers from +-1..8 (tests/gemm_f64.py): every partial sum is an integer below 2^24, so the fp32 result of
any kernel, split and order is the float64 product itself — the bound gemm_f64.compare_exact applies is zero."""
from importlib import import_module

import pytest
import torch

import calm_vit_dte_amd as calm
import weights as W
from gemm_f64 import MAX_TERMS, compare_exact
from helpers import CONFIGS, load_golden
from test_host_logic_cpu import build_model
from test_loss_cpu import ce_inputs

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
GUARD = 64
STAGE = 16 << 20          # floats of the buffer whose tail the operands are cut from (64 MiB: several passes over it
                          # are still running when a launch that did not wait for them would start)


@pytest.fixture
def be():
    """the backend with the deterministic k-split on and the lane switch restored afterwards"""
    b = calm.backend.get_backend()
    prev_det = b.gemm_set_option(b.GEMM_OPT_DETERMINISTIC, 1)
    prev_lane = calm.backend.get_wgrad_lane()
    yield b
    calm.backend.set_wgrad_lane(prev_lane)                       # (the library option with it)
    b.gemm_set_option(b.GEMM_OPT_DETERMINISTIC, prev_det)


class Guarded:
    """[M, N] output in the middle of a NaN-filled allocation: GUARD floats in front of it and behind it"""

    def __init__(self, M, N):
        self.buf = torch.full((M * N + 2 * GUARD,), float("nan"), device="cuda")
        self.t = self.buf[GUARD:GUARD + M * N].view(M, N)

    def guards_untouched(self):
        return bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all())


def _produce(stage):
    """Main-stream kernels that turn the whole NaN-filled stage into exact operands, in place: normal draws, scaled,
    rounded, clamped to +-8, zeros replaced by one."""
    stage.normal_()
    stage.mul_(4.0).round_().clamp_(-8.0, 8.0)
    stage.masked_fill_(stage == 0, 1.0)


@pytest.mark.parametrize("M,N,K,groups", [(96, 48, 4096, 1), (528, 176, 2048, 1), (240, 240, 1536, 3)],
                         ids=["96x48x4096", "528x176x2048", "3x240x240x1536"])
def test_lane_launch_equals_the_plain_launch_and_the_float64_product(be, M, N, K, groups):
    assert K <= MAX_TERMS
    stage = torch.full((STAGE,), float("nan"), device="cuda")
    n_a, n_b = K * M, K * N
    cut = STAGE - groups * (n_a + n_b)
    dys = [stage[cut + g * (n_a + n_b):][:n_a].view(K, M) for g in range(groups)]        # A(m, k) = dy[k, m]
    xs = [stage[cut + g * (n_a + n_b) + n_a:][:n_b].view(K, N) for g in range(groups)]   # B(n, k) = x[k, n]
    grouped = groups > 1
    pack = (lambda ts: list(ts)) if grouped else (lambda ts: ts[0])
    layout = (M, N, K, (1, M, 0, 0), (1, N, 0, 0), (N, 0, 0))
    kw = dict(batch=(groups, 1)) if grouped else {}

    lane = [Guarded(M, N) for _ in range(groups)]
    plan = be.gemm_describe(pack(dys), pack(xs), pack([o.t for o in lane]), *layout, **kw)
    assert plan["k_slices"] > 1, plan                            # a weight-gradient shape that k-splits
    be.gemm_set_option(be.GEMM_OPT_LANE, 1)
    before = be.gemm_lane_stats()
    torch.cuda.synchronize()
    _produce(stage)                                              # enqueued immediately before the fork ...
    be.gemm(pack(dys), pack(xs), pack([o.t for o in lane]), *layout, lane=True, **kw)
    assert len(be._lane_ws) == 1                                 # deterministic k-split: the workspace path
    be.gemm_lane_join()
    got = [o.t.clone() for o in lane]                            # ... and read immediately after the join: no device sync
    ref64 = [dy.double().T @ x.double() for dy, x in zip(dys, xs)]
    plain = [Guarded(M, N) for _ in range(groups)]
    be.gemm(pack(dys), pack(xs), pack([o.t for o in plain]), *layout, **kw)              # the plain call, same operands
    torch.cuda.synchronize()
    after = be.gemm_lane_stats()
    assert len(be._lane_ws) == 0                                 # the workspace was kept until the join, then released
    assert (after["forks"] - before["forks"], after["launches"] - before["launches"],
            after["joins"] - before["joins"]) == (1, 1, 1)

    for g in range(groups):
        assert not torch.isnan(lane[g].t).any() and lane[g].guards_untouched(), g
        assert not torch.isnan(plain[g].t).any() and plain[g].guards_untouched(), g
        assert torch.equal(got[g], plain[g].t), g                # bit-identical with the plain call
        compare_exact(got[g].cpu()[None, None], ref64[g].cpu()[None, None], plan)
    # a join with nothing on the lane issues nothing
    be.gemm_lane_join()
    assert be.gemm_lane_stats() == after


# ---------------------------------------------------------------------------------------------------------- model level
NAME = "nano48_cls"
BS = 8


def _batch():
    cfg = CONFIGS[NAME]
    x = torch.from_numpy(W.make_input((BS, 3, cfg.seq_length, cfg.seq_length), 2)).cuda()
    return x, ce_inputs(BS, cfg.out_features, 1.0)[1].cuda()


class _Boom(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError("boom")


def _run(be, lane, steps=3, graphed=False, fail_first=False):
    """`steps` training steps of nano48 from the same seed -> (state_dict, peak bytes, lane launches, lane joins).
    fail_first: a backward that raises in the node of the model's input — the last one, after every weight gradient —
    runs in front of them."""
    calm.backend.set_wgrad_lane(lane)
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    x, y = _batch()
    m = build_model(NAME, load_golden(NAME), "cuda").train()
    opt = trainer.FusedClipAdamW(m)
    before = be.gemm_lane_stats()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    try:
        if graphed:
            step = trainer.GraphedTrainStep(m, opt, x, y, restore_after_warmup=True)
            captured = be.gemm_lane_stats()
        else:
            step = trainer.TrainStep(m, opt, None)
        if fail_first:
            y_hat, _ = m(_Boom.apply(x.clone().requires_grad_(True)))
            loss = trainer.soft_target_cross_entropy(y_hat.squeeze(), y)
            mid = be.gemm_lane_stats()
            with pytest.raises(RuntimeError, match="boom"):
                with calm.ops.grad_tail(step.params) as on:
                    loss.backward()
            assert on
            now = be.gemm_lane_stats()
            if lane:                                   # weight gradients went to the lane, and drop() joined it
                assert now["launches"] > mid["launches"] and now["joins"] == mid["joins"] + 1
            assert calm.ops._tail.lane == [] and not calm.ops._tail.pending
            del loss, y_hat
            for p in m.parameters():
                p.grad = None
        for _ in range(steps):
            step(x, y)
        if graphed:                                    # the replays put nothing on the lane
            assert be.gemm_lane_stats() == captured
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    finally:
        opt.close()
    after = be.gemm_lane_stats()
    return sd, peak, after["launches"] - before["launches"], after["joins"] - before["joins"]


@pytest.fixture(scope="module")
def eager_lane_off():
    """the reference run, computed once: three eager steps without the lane (deterministic k-split)"""
    b = calm.backend.get_backend()
    prev_det = b.gemm_set_option(b.GEMM_OPT_DETERMINISTIC, 1)
    prev_lane = calm.backend.get_wgrad_lane()
    try:
        out = _run(b, False)
    finally:
        calm.backend.set_wgrad_lane(prev_lane)
        b.gemm_set_option(b.GEMM_OPT_DETERMINISTIC, prev_det)
    assert out[2] == 0 and out[3] == 0
    return out


def _assert_same_state(a, b):
    assert a.keys() == b.keys()
    differing = [k for k in a if not torch.equal(a[k], b[k])]
    assert not differing, differing[:8]


def test_three_steps_with_the_lane_equal_three_steps_without_it(be, eager_lane_off):
    sd_off, peak_off, _, _ = eager_lane_off
    sd_on, peak_on, launches, joins = _run(be, True)
    print(f"\n{NAME} bs {BS}: {launches} lane launches, {joins} joins in 3 steps; peak memory lane off {peak_off} B, "
          f"lane on {peak_on} B, difference {peak_on - peak_off:+d} B")
    assert launches >= 3 and joins >= 3                 # the lane carried weight gradients in every step
    _assert_same_state(sd_on, sd_off)
    moved = [k for k in sd_on if k.endswith("weight_orig")]
    assert moved


def test_a_backward_that_raises_leaves_the_lane_joined_and_the_next_step_right(be):
    sd_on, _, launches, _ = _run(be, True, steps=1, fail_first=True)
    sd_off, _, none, _ = _run(be, False, steps=1, fail_first=True)
    assert launches > 0 and none == 0
    _assert_same_state(sd_on, sd_off)


def test_a_captured_step_keeps_the_lane_out_of_the_graph(be, eager_lane_off):
    sd_graph, _, _, _ = _run(be, True, graphed=True)
    _assert_same_state(sd_graph, eager_lane_off[0])
