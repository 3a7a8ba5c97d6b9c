"""Weight EMA on the MI355X: calm_ema_update / calm_ema_swap element by element against float64 (tests/ema_f64.py) on a
table that reaches every path of the kernels, and trainer.ModelEMA through the training steps, evaluate() and a captured
Predictor."""
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import ema_f64 as F
import weights as W
from helpers import CONFIGS, load_golden
from test_host_logic_cpu import build_model

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")


def _table(seed=0):
    be = calm.backend.get_backend()
    chunk = int(be.lib.calm_ema_chunk_elems())
    assert chunk % 4 == 0
    pairs = F.make_table(chunk, "cuda", seed)
    plan = be.ema_plan(pairs)
    assert plan.n == len(pairs) - 1                       # the pair without elements has no entry
    assert plan.n_chunks == sum((s.numel() + chunk - 1) // chunk for s, _ in pairs)
    return be, plan, [(s, a) for s, a in pairs if s.numel() > 0]


def _host(t):
    return t.detach().cpu().numpy()


def _bases(pairs):
    """Clones of the whole buffers the table's tensors are views of (8 spare floats each)."""
    return [(s._base.clone(), a._base.clone()) for s, a in pairs]


def _check_outside_untouched(pairs, bases):
    """Not a word outside a tensor's own range was written."""
    for (s, a), (bs, ba) in zip(pairs, bases):
        for t, b0 in ((s, bs), (a, ba)):
            off, n = t.storage_offset(), t.numel()
            assert torch.equal(t._base[:off].view(torch.int32), b0[:off].view(torch.int32))
            assert torch.equal(t._base[off + n:].view(torch.int32), b0[off + n:].view(torch.int32))


@pytest.mark.parametrize("decay,schedule,n", [(0.999, F.EMA_CONSTANT, 0), (0.9999, F.EMA_WARMUP, 0), (0.9999, F.EMA_WARMUP, 57)],
                         ids=["constant", "warmup-n0", "warmup-n57"])
def test_update_every_element_against_float64(decay, schedule, n):
    be, plan, pairs = _table()
    plan.count_dev.fill_(n)
    bases = _bases(pairs)
    before = [(_host(s), _host(a)) for s, a in pairs]
    be.ema_update(plan, decay, schedule)
    torch.cuda.synchronize()
    assert int(plan.count_dev.item()) == n + 1            # advanced by exactly 1
    w, skipped = plan.weight_out.tolist()
    assert skipped == 0.0
    err_w = F.check_weight(w, decay, schedule, n)
    assert np.float32(w) == np.float32(trainer.ema_weight(decay, schedule, n))       # the host formula, bit for bit
    worst = 0.0
    for (s, a), (s0, e0) in zip(pairs, before):
        F.check_bits_equal(_host(s), s0, "parameter after an update")
        worst = max(worst, F.check_update(e0, s0, _host(a), w))
    _check_outside_untouched(pairs, bases)
    print(f"w error {err_w:.3e}, worst element error {worst:.3f} of the bound")


def test_skipped_update_leaves_averages_and_counter_bit_unchanged():
    be, plan, pairs = _table()
    plan.count_dev.fill_(11)
    plan.weight_out.fill_(0.5)
    before = [_host(a) for _, a in pairs]
    skip = torch.ones(1, device="cuda")
    be.ema_update(plan, 0.999, F.EMA_WARMUP, skip)
    torch.cuda.synchronize()
    assert plan.weight_out.tolist() == [0.0, 1.0] and int(plan.count_dev.item()) == 11
    for (_, a), e0 in zip(pairs, before):
        F.check_bits_equal(_host(a), e0, "average after a skipped update")
    skip.zero_()                                          # the same call with skip = 0 is an ordinary update
    be.ema_update(plan, 0.999, F.EMA_WARMUP, skip)
    torch.cuda.synchronize()
    w, skipped = plan.weight_out.tolist()
    assert skipped == 0.0 and int(plan.count_dev.item()) == 12
    F.check_weight(w, 0.999, F.EMA_WARMUP, 11)
    for (s, a), e0 in zip(pairs, before):
        F.check_update(e0, _host(s), _host(a), w)


def test_swap_is_bit_exact_and_two_swaps_are_the_identity():
    be, plan, pairs = _table(seed=40)
    nan = torch.tensor([0x7fc00001, -0x3edcba, 0x7f800001, -0x7fffff], dtype=torch.int32, device="cuda").view(torch.float32)
    for k in (3, 6, 10, 12, 13):                          # vector body, scalar tail and both misaligned pairs carry NaN payloads
        s, a = pairs[k]
        s.reshape(-1)[-4:] = nan
        a.reshape(-1)[:4] = nan.flip(0)
    bases = _bases(pairs)
    before = [(_host(s), _host(a)) for s, a in pairs]
    be.ema_swap(plan)
    torch.cuda.synchronize()
    for (s, a), (s0, a0) in zip(pairs, before):
        F.check_swap(s0, a0, _host(s), _host(a))
    _check_outside_untouched(pairs, bases)
    be.ema_swap(plan)
    torch.cuda.synchronize()
    for (s, a), (s0, a0) in zip(pairs, before):
        F.check_bits_equal(_host(s), s0, "parameter after two swaps")
        F.check_bits_equal(_host(a), a0, "average after two swaps")


def test_plan_refuses_what_the_kernels_cannot_take():
    be = calm.backend.get_backend()
    a, b = torch.zeros(8, 6, device="cuda"), torch.zeros(8, 6, device="cuda")
    with pytest.raises(TypeError, match="fp32"):
        be.ema_plan([(a.half(), b.half())])
    with pytest.raises(TypeError, match="contiguous"):
        be.ema_plan([(a.t(), b.t())])
    with pytest.raises(ValueError, match="shape mismatch"):
        be.ema_plan([(a, b.reshape(6, 8))])
    buf = torch.zeros(100, device="cuda")
    with pytest.raises(ValueError, match="overlap"):
        be.ema_plan([(buf[:60], buf[40:])])
    with pytest.raises(RuntimeError):
        be.ema_plan([(a.cpu(), b.cpu())])
    plan = be.ema_plan([(a, b)])
    for bad in (1.0, -0.5, float("nan")):
        with pytest.raises(RuntimeError, match="calm_ema_update"):
            be.ema_update(plan, bad, F.EMA_CONSTANT)
    with pytest.raises(RuntimeError, match="calm_ema_update"):
        be.ema_update(plan, 0.9, 2)


# ---- ModelEMA through the training steps -----------------------------------------------------------------------------------
def _batch(name, bs=4):
    cfg = CONFIGS[name]
    g = np.random.default_rng(5)
    x = torch.from_numpy(g.standard_normal((bs, 3, cfg.seq_length, cfg.seq_length)).astype(np.float32))
    a, b = g.integers(0, cfg.out_features, bs), g.integers(0, cfg.out_features, bs)
    y = np.zeros((bs, cfg.out_features), dtype=np.float32)
    y[np.arange(bs), a] += 0.7
    y[np.arange(bs), b] += 0.3
    return x.cuda(), torch.from_numpy(y).cuda()


def _follow(step, ema, m, x, y, decay, steps=3):
    """`steps` training steps; after each, every average against the float64 recurrence from its own previous state and
    the parameters as the optimizer step left them."""
    for n in range(steps):
        before = [_host(s) for s in ema.shadows]
        step(x, y)
        torch.cuda.synchronize()
        assert ema.num_updates == n + 1
        w, skipped = ema._plan.weight_out.tolist()
        assert skipped == 0.0
        F.check_weight(w, decay, F.EMA_WARMUP, n)
        for p, s, e0 in zip(m.parameters(), ema.shadows, before):
            F.check_update(e0, _host(p), _host(s), w)


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_training_steps_keep_the_average_on_the_recurrence(graphed):
    name = "nano48_cls"
    m = build_model(name, load_golden(name), "cuda").train()
    x, y = _batch(name)
    opt = trainer.FusedClipAdamW(m)
    try:
        ema = trainer.ModelEMA(m, decay=0.99, warmup=True)
        start = [_host(p) for p in m.parameters()]
        if graphed:
            step = trainer.GraphedTrainStep(m, opt, x, y, warmup=2, restore_after_warmup=True, ema=ema)
            assert ema.num_updates == 0                    # the warm-up and capture steps are undone: next is update 1
            for p, s, p0 in zip(m.parameters(), ema.shadows, start):
                F.check_bits_equal(_host(p), p0, "parameter restored after the capture")
                F.check_bits_equal(_host(s), p0, "average restored after the capture")
        else:
            step = trainer.TrainStep(m, opt, ema=ema)
        _follow(step, ema, m, x, y, 0.99)
        moved = sum(not torch.equal(p, s) for p, s in zip(m.parameters(), ema.shadows))
        assert moved > 0
    finally:
        opt.close()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch-adamw"])
def test_step_skipped_for_an_inf_gradient_leaves_the_average_alone(fused):
    name = "nano48_cls"
    m = build_model(name, load_golden(name), "cuda").train()
    x, y = _batch(name)
    opt = trainer.FusedClipAdamW(m) if fused else trainer.make_optimizer(m)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    try:
        ema = trainer.ModelEMA(m, decay=0.9, warmup=False)
        step = trainer.TrainStep(m, opt, scaler=scaler, ema=ema)
        victim = dict(m.named_parameters())["autoencoder.ln_final.weight"]
        handle = victim.register_hook(lambda g: torch.full_like(g, float("inf")))
        live = [_host(p) for p in m.parameters()]
        before = [_host(s) for s in ema.shadows]
        step(x, y)
        torch.cuda.synchronize()
        handle.remove()
        assert ema.num_updates == 0 and ema._plan.weight_out.tolist() == [0.0, 1.0]
        assert float(scaler.get_scale()) == 512.0          # the scaler backed off: the optimizer step was skipped
        for p, s, p0, e0 in zip(m.parameters(), ema.shadows, live, before):
            F.check_bits_equal(_host(p), p0, "parameter after the skipped step")
            F.check_bits_equal(_host(s), e0, "average after the skipped step")
        step(x, y)                                         # a clean step is update 1
        torch.cuda.synchronize()
        assert ema.num_updates == 1
        w, skipped = ema._plan.weight_out.tolist()
        assert skipped == 0.0
        F.check_weight(w, 0.9, F.EMA_CONSTANT, 0)
        for p, s, e0 in zip(m.parameters(), ema.shadows, before):
            F.check_update(e0, _host(p), _host(s), w)
    finally:
        if fused:
            opt.close()


# ---- evaluation with the average -------------------------------------------------------------------------------------------
def _model_with_average():
    """A Nano-48 model whose average differs from its weights, and a second instance loaded with the average."""
    name = "nano48_cls"
    g = load_golden(name)
    m = build_model(name, g, "cuda").train()
    ema = trainer.ModelEMA(m, decay=0.5, warmup=False)
    gen = torch.Generator(device="cuda").manual_seed(3)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.randn(p.shape, device="cuda", generator=gen) * 0.02 * p.abs().mean())
    ema.update()
    torch.cuda.synchronize()
    copy = build_model(name, g, "cuda")
    copy.load_state_dict(ema.model_state_dict())
    xs = torch.from_numpy(W.make_input((4, 3, 48, 48), 5)).cuda()
    with torch.no_grad():
        logits = copy.eval()(xs)[0].reshape(4, -1).clone()
    return m, ema, copy, xs, logits


def test_evaluate_with_the_average_equals_a_copy_loaded_with_it():
    m, ema, copy, xs, logits = _model_with_average()
    labels = logits.argmax(dim=1)
    labels[2:] = (labels[2:] + 1) % logits.shape[1]        # two right, two wrong for the averaged model
    batches = [(xs[:2], labels[:2]), (xs[2:], labels[2:])]
    live = [_host(p) for p in m.parameters()]
    avg = [_host(s) for s in ema.shadows]
    with ema.applied(), torch.no_grad():
        m.eval()
        inside = m(xs)[0].reshape(4, -1).clone()
        m.train()
    assert torch.equal(inside, logits)                     # bit-identical logits
    with torch.no_grad():
        m.eval()
        assert not torch.equal(m(xs)[0].reshape(4, -1), logits)     # and they are not the live model's
        m.train()
    acc = trainer.evaluate(m, batches, ema=ema)
    assert acc == trainer.evaluate(copy, batches) == 0.5
    assert m.training and not ema.is_swapped

    def failing():
        yield batches[0]
        raise KeyError("a batch that raises")
    with pytest.raises(KeyError):
        trainer.evaluate(m, failing(), ema=ema)
    torch.cuda.synchronize()
    assert not ema.is_swapped
    for p, s, p0, e0 in zip(m.parameters(), ema.shadows, live, avg):
        F.check_bits_equal(_host(p), p0, "live parameter after evaluate(ema=)")
        F.check_bits_equal(_host(s), e0, "average after evaluate(ema=)")
    m.train()


def test_captured_predictor_sees_the_average_after_a_swap():
    m, ema, copy, xs, logits = _model_with_average()
    pred = trainer.Predictor(m, example_x=xs, graph=True)
    try:
        assert pred.graph is not None
        live_out = pred(xs)[0].reshape(4, -1)
        assert not torch.equal(live_out, logits)
        ema.swap()                                         # no re-capture: the graph reads the parameters where they live
        swapped_out = pred(xs)[0].reshape(4, -1)
        ema.swap()
        assert torch.equal(swapped_out, logits)
        assert torch.equal(pred(xs)[0].reshape(4, -1), live_out)
    finally:
        pred.close()
