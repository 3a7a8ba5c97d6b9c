"""The gradient tail's plumbing (ops._GradTail, ops.grad_tail, the trainer's step classes, BucketedGradReducer) without a
GPU, on emulated_grad_tail.TailBackend: what is queued in which order, one flush per backward, the flush from the reducer's
hook, the fallbacks (a .grad that exists, a backend without the batch calls, the switch) and a second backward after a
flush.  The emulation adds 0 + s, so deferred and immediate gradients are compared with torch.equal."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import calm_vit_dte_amd as calm  # noqa: E402
from calm_vit_dte_amd import ops  # noqa: E402
from emulated_backend import EmulatedBackend  # noqa: E402
from emulated_grad_tail import TailBackend  # noqa: E402
from test_host_logic_cpu import build_model  # noqa: E402
from importlib import import_module  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")


def _batch(seed=0, B=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 32, 32, generator=g), torch.softmax(torch.randn(B, 10, generator=g), 1)


def _models(n):
    first = build_model("tiny32_cls", None).train()
    out = [first]
    for _ in range(n - 1):
        m = build_model("tiny32_cls", None).train()
        m.load_state_dict(first.state_dict())
        out.append(m)
    return out


def _backward(m, be, x, y, arm=True):
    """Forward, loss, backward under the tail (as TrainStep._finish arms it): -> (armed, gradients by name)."""
    with calm.backend.use_backend(be):
        opt = trainer.FusedClipAdamW(m)             # marks the spectral-norm deferral, as in a training run
        try:
            y_hat, _ = m(x)
            loss = trainer.soft_target_cross_entropy(y_hat.squeeze(), y)
            params = [p for p in m.parameters() if p.requires_grad]
            if arm:
                with ops.grad_tail(params) as on:
                    loss.backward()
            else:
                on = False
                loss.backward()
        finally:
            opt.close()
    return on, {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def test_queue_order_and_one_flush_per_backward():
    m_ref, m = _models(2)
    x, y = _batch()
    _, want = _backward(m_ref, EmulatedBackend(), x, y, arm=False)
    be = TailBackend()
    before = ops._tail.flushes
    on, got = _backward(m, be, x, y)
    assert on and ops._tail.flushes == before + 1
    assert not ops._tail.armed and not ops._tail.reduce and not ops._tail.sn and not ops._tail.pending
    parts = [e for e in be.log if e[0] == "part"]
    batches = [e for e in be.log if e[0] in ("reduce", "sn")]
    # every kind of producer deferred; one batch of each kind, behind every producer, entries in the order produced
    assert {kind for _, kind, _ in parts} == {"layernorm", "rope", "colsum", "cnn"}
    assert [e[0] for e in batches] == ["reduce", "sn"] and be.log[-2:] == batches
    assert batches[0][1] == [pid for _, _, pid in parts]
    assert len(batches[1][1]) > 0 and len(set(batches[1][1])) == len(batches[1][1])
    assert sorted(got) == sorted(want)
    assert not [k for k in want if not torch.equal(got[k], want[k])]


def test_the_steps_of_the_trainer_arm_the_tail_and_a_second_backward_flushes_again():
    m_ref, m = _models(2)
    x, y = _batch(1)
    states = []
    for model, be in ((m_ref, EmulatedBackend()), (m, TailBackend())):
        with calm.backend.use_backend(be):
            opt = trainer.FusedClipAdamW(model)
            step = trainer.TrainStep(model, opt)
            before = ops._tail.flushes
            try:
                for _ in range(2):
                    step(x, y)
            finally:
                opt.close()
        flushes = ops._tail.flushes - before
        states.append({k: v.clone() for k, v in model.state_dict().items()})
    assert flushes == 2 and [e[0] for e in be.log if e[0] != "part"] == ["reduce", "sn"] * 2
    assert not [k for k in states[0] if not torch.equal(states[0][k], states[1][k])]


def test_falls_back_when_a_grad_exists_or_the_backend_has_no_batch_calls_or_the_switch_is_off(monkeypatch):
    x, y = _batch(2)
    m_ref, m_grad, m_plain, m_off = _models(4)
    _, want = _backward(m_ref, EmulatedBackend(), x, y, arm=False)
    # a parameter that already holds a gradient: autograd adds to it, so nothing may be handed over unfinished
    name, p = next((k, q) for k, q in m_grad.named_parameters() if k.endswith("ln_final.weight"))
    p.grad = torch.full_like(p, 0.25)
    be = TailBackend()
    before = ops._tail.flushes
    on, got = _backward(m_grad, be, x, y)
    assert not on and be.log == [] and ops._tail.flushes == before
    assert torch.equal(got[name], want[name] + 0.25)
    assert not [k for k in want if k != name and not torch.equal(got[k], want[k])]
    # a backend without the batch calls: armed, but every backward takes the immediate path
    on, got = _backward(m_plain, EmulatedBackend(), x, y)
    assert on and ops._tail.flushes == before
    assert not [k for k in want if not torch.equal(got[k], want[k])]
    # CALM_GRAD_TAIL=0
    monkeypatch.setattr(ops, "GRAD_TAIL", False)
    be = TailBackend()
    on, got = _backward(m_off, be, x, y)
    assert not on and be.log == [] and ops._tail.flushes == before
    assert not [k for k in want if not torch.equal(got[k], want[k])]


def test_a_parameter_used_twice_in_one_graph_flushes_early_and_sums_both_uses():
    g = torch.Generator().manual_seed(3)
    w = torch.nn.Parameter(torch.randn(24, generator=g))
    xa, xb = torch.randn(6, 24, generator=g, requires_grad=True), torch.randn(5, 24, generator=g, requires_grad=True)
    ga, gb = torch.randn(6, 24, generator=g), torch.randn(5, 24, generator=g)

    def run(be, arm):
        w.grad = None
        with calm.backend.use_backend(be):
            loss = (ops.LayerNormFn.apply(xa, w, 1e-6) * ga).sum() + (ops.LayerNormFn.apply(xb, w, 1e-6) * gb).sum()
            if arm:
                with ops.grad_tail([w]) as on:
                    loss.backward()
                assert on
            else:
                loss.backward()
        return w.grad.clone()

    want = run(EmulatedBackend(), False)
    be = TailBackend()
    got = run(be, True)
    # the first use is deferred; the second finds it in the queue: flush, then the immediate path
    assert [e[0] for e in be.log] == ["part", "reduce"]
    assert torch.allclose(got, want, rtol=0, atol=0)


def test_the_reducer_flushes_the_queue_before_it_packs_a_bucket(tmp_path):
    """A world of one gloo rank with the reducer forced on (1 MiB buckets, its smallest): a bucket launch finds deferred
    gradients in the queue and none behind it — the flush happened inside _launch, before the bucket was packed — and the
    reduced gradients are the immediate ones."""
    import torch.distributed as dist
    x, y = _batch(4)
    m_ref, m = _models(2)
    _, want = _backward(m_ref, EmulatedBackend(), x, y, arm=False)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", world_size=1, rank=0)
    try:
        be = TailBackend()
        with calm.backend.use_backend(be):
            opt = trainer.FusedClipAdamW(m)
            try:
                red = trainer.BucketedGradReducer(m, bucket_mb=1, tail_mb=1, force=True)
                assert red.enabled
                packed = []
                launch = red._launch

                def spy(b):
                    queued = (len(ops._tail.reduce), len(ops._tail.sn))
                    flushes = ops._tail.flushes
                    launch(b)
                    packed.append((queued, (len(ops._tail.reduce), len(ops._tail.sn)), ops._tail.flushes - flushes))
                red._launch = spy
                before = ops._tail.flushes
                y_hat, _ = m(x)
                loss = trainer.soft_target_cross_entropy(y_hat.squeeze(), y)
                with ops.grad_tail(red.params) as on:
                    loss.backward()
                red.finish()
            finally:
                opt.close()
        assert on and packed and all(after == (0, 0) for _, after, _ in packed)
        # at least one launch found work and flushed it itself (the engine callback runs only after the last launch)
        assert any(queued != (0, 0) and n == 1 for queued, _, n in packed), packed
        assert ops._tail.flushes - before >= 1 and any(e[0] == "reduce" for e in be.log)
        got = {k: p.grad.clone() for k, p in m.named_parameters()}
        assert not [k for k in want if not torch.equal(got[k], want[k])]
    finally:
        dist.destroy_process_group()


def test_a_parameter_with_a_hook_gets_its_gradient_in_line():
    """A tensor hook reads (here: replaces) the gradient before AccumulateGrad, a post-accumulate hook reads .grad right
    after it: both must see the finished sum, so such a parameter is never deferred — the others still are."""
    x, y = _batch(5)
    m_ref, m = _models(2)
    _, want = _backward(m_ref, EmulatedBackend(), x, y, arm=False)
    params = dict(m.named_parameters())
    replaced = next(k for k in params if k.endswith("ln_final.weight"))
    watched = next(k for k in params if k.endswith("bias") and k != replaced)
    seen = {}
    h1 = params[replaced].register_hook(lambda g: (seen.setdefault("hook", g.clone()), torch.full_like(g, 3.0))[1])
    h2 = params[watched].register_post_accumulate_grad_hook(lambda p: seen.update(post=p.grad.clone()))
    be = TailBackend()
    try:
        on, got = _backward(m, be, x, y)
    finally:
        h1.remove()
        h2.remove()
    assert on and any(e[0] == "reduce" for e in be.log)
    assert torch.equal(seen["hook"], want[replaced]) and torch.equal(got[replaced], torch.full_like(want[replaced], 3.0))
    assert torch.equal(seen["post"], want[watched]) and torch.equal(got[watched], want[watched])
    assert not [k for k in want if k != replaced and not torch.equal(got[k], want[k])]


def test_the_step_classes_do_not_arm_the_tail_under_stock_ddp(tmp_path):
    """DistributedDataParallel copies .grad into its buckets from C++ hooks on the AccumulateGrad nodes, which no Python
    hook table shows, and copies the reduced buckets back over .grad at the end of the backward: a deferred gradient would
    be exchanged unfinished.  A TrainStep on a DDP model (world of one, gloo) with a backend that has the batch calls
    therefore defers nothing, and the gradients its optimizer sees are those of the same step on a backend without the
    batch calls; the same model without DDP does defer."""
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    x, y = _batch(6)
    m_ref, m_ddp, m_plain = _models(3)

    def run(model, be, wrap):
        """One TrainStep; -> (gradients as the optimizer's zero_grad finds them, i.e. after the exchange and the clip)"""
        grads = {}
        with calm.backend.use_backend(be):
            opt = trainer.make_optimizer(model)
            step = trainer.TrainStep(DDP(model) if wrap else model, opt, None)
            assert step._tail_enabled() == (not wrap)
            opt.zero_grad = lambda *a, **k: grads.update({n: p.grad.clone() for n, p in model.named_parameters()})
            step(x, y)
        return grads

    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", world_size=1, rank=0)
    try:
        want = run(m_ref, EmulatedBackend(), False)
        be = TailBackend()
        got = run(m_ddp, be, True)
        assert be.log == []
        be = TailBackend()
        plain = run(m_plain, be, False)
        assert any(e[0] == "reduce" for e in be.log) and any(e[0] == "sn" for e in be.log)
    finally:
        dist.destroy_process_group()
    assert sorted(got) == sorted(want) == sorted(plain) and len(want) > 10
    assert not [k for k in want if not torch.equal(got[k], want[k])]
    assert not [k for k in want if not torch.equal(plain[k], want[k])]
