"""The gradient tail on the MI355X: calm_reduce_partials_batch and calm_sn_weight_bwd_batch against the single-entry
forms, and a training step with the tail on against the same step with it off.  Every comparison is BITWISE: the batched
kernels run, per entry, the additions of the single ones in the same order (one shared device function), so there is no
tolerance to derive.

The single reduction is reached through calm_colsum: on an input that is not 16-byte aligned it takes the one-element
kernel, whose grid — the number G of partial rows — is ceil(rows / (8 * per)) with per = 1 for cols >= 256 and
256 // cols below (colsum_grid, csrc/norm_act.hip).  That gives every G of the list at every n; the test asserts the G the
library reports.  G in {1, 15, 16, 17, 63, 64, 65, 130} are the boundaries of the 16 row lanes and of their four running
sums, n in {1, 48, 64, 80, 547} those of the 64-column blocks (547 is the CNN tail's partial row)."""
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import weights as W
from helpers import CONFIGS, load_golden
from test_host_logic_cpu import build_model

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")

DEV = "cuda"
GS = (1, 15, 16, 17, 63, 64, 65, 130)
NS = (1, 48, 64, 80, 547)


@pytest.fixture(scope="module")
def hip():
    return calm.backend.get_backend()


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def misaligned(t):
    """Device copy of t that starts 4 bytes into an allocation: not 16-byte aligned."""
    buf = torch.empty(1 + t.numel(), dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    return v


def colsum_rows(G, n):
    per = 1 if n >= 256 else 256 // n
    return G * 8 * per


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def colsum_case(hip, G, n, seed):
    """(x, init, want): the single form's result for an input that makes G rows of n partials."""
    rows = colsum_rows(G, n)
    x = misaligned(rnd(rows, n, seed=seed))
    init = rnd(n, seed=seed + 1).to(DEV)
    want = init.clone()
    hip.colsum(x, want, rows, n)
    return x, init, want


def test_batched_reduce_equals_the_single_reduce_at_every_lane_and_block_boundary(hip):
    """All 40 (G, n) pairs as one call — more entries than one launch takes, so the call also splits."""
    cases, items = [], []
    for i, (G, n) in enumerate((G, n) for G in GS for n in NS):
        x, init, want = colsum_case(hip, G, n, seed=3 * i)
        part, shape = hip.colsum_part(x, x.shape[0], n)
        assert (shape.G, shape.n, shape.stride, shape.nseg) == (G, n, n, 1), (G, n)
        out = init.clone()
        cases.append((G, n, out, want))
        items.append((part, shape, [out]))
    assert len(items) > int(hip.lib.calm_reduce_batch_max())
    hip.reduce_partials_batch(items)
    torch.cuda.synchronize()
    bad = [(G, n) for G, n, out, want in cases if not same_bits(out, want)]
    assert not bad, bad


def test_one_entry_past_the_per_launch_cap(hip):
    cap = int(hip.lib.calm_reduce_batch_max())
    cases, items = [], []
    for i in range(cap + 1):
        G, n = GS[i % len(GS)], (48, 80, 64)[i % 3]
        x, init, want = colsum_case(hip, G, n, seed=100 + 2 * i)
        out = init.clone()
        part, shape = hip.colsum_part(x, x.shape[0], n)
        cases.append((i, out, want))
        items.append((part, shape, [out]))
    hip.reduce_partials_batch(items)
    torch.cuda.synchronize()
    bad = [i for i, out, want in cases if not same_bits(out, want)]
    assert not bad, bad


def test_mixed_producers_in_one_call_with_the_six_segment_cnn_form(hip):
    """LayerNorm dw, RoPE d_inv_freq, a 16-byte-form column sum and the CNN tail's six gradients: each producer's partial
    form + one batched call against the producer's own two-launch form."""
    items, pairs = [], []
    # LayerNorm backward, 300 rows of 48 and (vector kernel) 700 rows of 64
    for rows, D, seed in ((300, 48, 1), (700, 64, 2)):
        dy, x, w = rnd(rows, D, seed=seed).to(DEV), rnd(rows, D, seed=seed + 10).to(DEV), rnd(D, seed=seed + 20).to(DEV)
        mean, rstd = rnd(rows, seed=seed + 30).to(DEV), rnd(rows, seed=seed + 40).abs().add(0.5).to(DEV)
        init = rnd(D, seed=seed + 50).to(DEV)
        dx0, dw0 = torch.empty_like(x), init.clone()
        hip.layernorm_bwd(dy, x, w, mean, rstd, dx0, dw0, rows, D)
        dx1, dw1 = torch.empty_like(x), init.clone()
        part, shape = hip.layernorm_bwd_part(dy, x, w, mean, rstd, dx1, rows, D)
        items.append((part, shape, [dw1]))
        pairs += [("ln dx", dx1, dx0), ("ln dw", dw1, dw0)]
    # RoPE backward
    B, S, H, dr = 2, 16, 4, 8
    xr, inv_freq = rnd(B, S, H * dr, seed=5).to(DEV), rnd(dr // 2, seed=6).abs().to(DEV)
    table, out = torch.empty(2 * S * (dr // 2), device=DEV), torch.empty(B, S, H * dr, device=DEV)
    hip.rope_fwd(None, xr, inv_freq, table, out, B, S, H, 0, dr)
    dout, init = rnd(B, S, H * dr, seed=7).to(DEV), rnd(dr // 2, seed=8).to(DEV)
    dxr0, dif0 = torch.empty_like(xr), init.clone()
    hip.rope_bwd(dout, xr, table, None, dxr0, dif0, B, S, H, 0, dr)
    dxr1, dif1 = torch.empty_like(xr), init.clone()
    part, shape = hip.rope_bwd_part(dout, xr, table, None, dxr1, B, S, H, 0, dr)
    items.append((part, shape, [dif1]))
    pairs += [("rope d_xr", dxr1, dxr0), ("rope d_inv_freq", dif1, dif0)]
    # column sum, 16-byte form (aligned input, rows >= 64)
    x, init = rnd(1000, 80, seed=9).to(DEV), rnd(80, seed=10).to(DEV)
    cs0 = init.clone()
    hip.colsum(x, cs0, 1000, 80)
    cs1 = init.clone()
    part, shape = hip.colsum_part(x, 1000, 80)
    items.append((part, shape, [cs1]))
    pairs.append(("colsum", cs1, cs0))
    # the CNN tail: six outputs side by side in one partial row of 547, rows 560 floats apart
    B, S, Ch = 3, 32, 32
    dy, x = rnd(B, S, 3 * S, seed=11).to(DEV), rnd(B, S, 3 * S, seed=12).to(DEV)
    w0, b0, w2, b2 = (rnd(n, seed=13 + i).mul(0.3).to(DEV) for i, n in enumerate((Ch * 3, Ch, Ch * 9, Ch)))
    w4, b4 = rnd(3 * Ch, seed=17).mul(0.3).to(DEV), rnd(3, seed=18).to(DEV)
    s0, s2, s4 = (torch.tensor([v], device=DEV) for v in (1.3, 0.9, 1.1))
    sizes = [Ch * 3, Ch, Ch * 9, Ch, 3 * Ch, 3]
    init = rnd(sum(sizes), seed=19).to(DEV)
    g0 = init.clone()
    dx0 = torch.empty_like(dy)
    hip.cnn_bwd(dy, x, w0, s0, b0, w2, s2, b2, w4, s4, b4, dx0, *torch.split(g0, sizes), B, S, Ch)
    g1 = init.clone()
    dx1 = torch.empty_like(dy)
    part, shape = hip.cnn_bwd_part(dy, x, w0, s0, b0, w2, s2, b2, w4, s4, b4, dx1, B, S, Ch)
    assert (shape.n, shape.stride, shape.nseg) == (547, 560, 6) and list(shape.begin) == [0, 96, 128, 416, 448, 544, 547]
    items.append((part, shape, list(torch.split(g1, sizes))))
    pairs += [("cnn dx", dx1, dx0), ("cnn weight gradients", g1, g0)]
    hip.reduce_partials_batch(items)
    torch.cuda.synchronize()
    bad = [name for name, got, want in pairs if not same_bits(got, want)]
    assert not bad, bad


SN_SHAPES = ((3, 5), (32, 9), (48, 16), (240, 240))


def test_batched_sn_correction_equals_the_single_one_with_and_without_layerscale(hip):
    """Eight layers (four shapes, with and without ls) in one call against calm_sn_weight_bwd on each."""
    items, pairs = [], []
    for i, ((rows, cols), with_ls) in enumerate((s, l) for s in SN_SHAPES for l in (False, True)):
        G, w = rnd(rows, cols, seed=20 * i).to(DEV), rnd(rows, cols, seed=20 * i + 1).to(DEV)
        u, v = rnd(rows, seed=20 * i + 2).to(DEV), rnd(cols, seed=20 * i + 3).to(DEV)
        sigma = torch.tensor([1.7 + 0.1 * i], device=DEV)
        ls = rnd(rows, seed=20 * i + 4).to(DEV) if with_ls else None
        dW0, dW1 = torch.full_like(w, float("nan")), torch.full_like(w, float("nan"))
        dls0 = torch.full((rows,), float("nan"), device=DEV) if with_ls else None
        dls1 = torch.full((rows,), float("nan"), device=DEV) if with_ls else None
        hip.sn_weight_bwd(G, w, u, v, sigma, ls, dW0, dls0, rows, cols)
        items.append((G, w, u, v, sigma, ls, dW1, dls1, rows, cols))
        pairs.append(((rows, cols, with_ls, "dW"), dW1, dW0))
        if with_ls:
            pairs.append(((rows, cols, with_ls, "d_ls"), dls1, dls0))
    hip.sn_weight_bwd_batch(items)
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(want).any()) for _, _, want in pairs)
    bad = [name for name, got, want in pairs if not same_bits(got, want)]
    assert not bad, bad


def test_one_sn_layer_past_the_per_launch_cap(hip):
    cap = int(hip.lib.calm_sn_bwd_batch_max())
    items, pairs = [], []
    for i in range(cap + 1):
        rows, cols = SN_SHAPES[i % 3]
        G, w = rnd(rows, cols, seed=7 * i).to(DEV), rnd(rows, cols, seed=7 * i + 1).to(DEV)
        u, v, ls = rnd(rows, seed=7 * i + 2).to(DEV), rnd(cols, seed=7 * i + 3).to(DEV), rnd(rows, seed=7 * i + 4).to(DEV)
        sigma = torch.tensor([0.8 + 0.05 * i], device=DEV)
        dW0, dW1, dls0, dls1 = torch.empty_like(w), torch.empty_like(w), torch.empty_like(ls), torch.empty_like(ls)
        hip.sn_weight_bwd(G, w, u, v, sigma, ls, dW0, dls0, rows, cols)
        items.append((G, w, u, v, sigma, ls, dW1, dls1, rows, cols))
        pairs += [(i, dW1, dW0), (i, dls1, dls0)]
    hip.sn_weight_bwd_batch(items)
    torch.cuda.synchronize()
    bad = [i for i, got, want in pairs if not same_bits(got, want)]
    assert not bad, bad


# ---- a training step with the tail on and off ----------------------------------------------------------------------------
def _batch(name, bs=4):
    cfg = CONFIGS[name]
    g = np.random.default_rng(5)
    x = torch.from_numpy(g.standard_normal((bs, 3, cfg.seq_length, cfg.seq_length)).astype(np.float32))
    a, b = g.integers(0, cfg.out_features, bs), g.integers(0, cfg.out_features, bs)
    y = np.zeros((bs, cfg.out_features), dtype=np.float32)
    y[np.arange(bs), a] += 0.7
    y[np.arange(bs), b] += 0.3
    return x.cuda(), torch.from_numpy(y).cuda()


def _train(tail, graphed, monkeypatch):
    """Eager: one backward under the tail (its gradients), then a training step.  Graphed: a captured step (one warm-up
    step in front) replayed twice.  -> (gradients, state, queue lengths (reductions, corrections) at each flush that found
    work)."""
    monkeypatch.setattr(calm.ops, "GRAD_TAIL", tail)
    name = "nano48_cls"
    x, y = _batch(name)
    m = build_model(name, load_golden(name), "cuda").train()
    # the latent noise: injected from the host in the eager run; a capture cannot copy from the host, so the captured run
    # draws it on the device from a generator seeded alike in both runs (the tail draws nothing)
    torch.manual_seed(1234)
    if not graphed:
        calm.ops.set_noise_override(W.NoiseStream(11))
    opt = trainer.FusedClipAdamW(m)
    deferred, grads = [], {}
    real = calm.ops._tail.flush

    def counting_flush():
        deferred.append((len(calm.ops._tail.reduce), len(calm.ops._tail.sn)))
        real()
    monkeypatch.setattr(calm.ops._tail, "flush", counting_flush)
    try:
        if graphed:
            # (no eager backward in front of the capture: the AccumulateGrad nodes it leaves behind belong to the default
            # stream, which a capture must not touch)
            gstep = trainer.GraphedTrainStep(m, opt, x, y, warmup=1)
            for _ in range(2):
                gstep(x, y)
        else:
            step = trainer.TrainStep(m, opt, None)
            y_hat, _ = m(x)
            loss = trainer.soft_target_cross_entropy(y_hat.squeeze(), y)
            with calm.ops.grad_tail(step.params) as on:
                loss.backward()
            assert on == tail
            del loss, y_hat
            grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
            for p in m.parameters():
                p.grad = None
            step(x, y)
        torch.cuda.synchronize()
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        state.update({f"exp_avg.{i}": t.clone() for i, t in enumerate(opt.exp_avg)})
        state.update({f"exp_avg_sq.{i}": t.clone() for i, t in enumerate(opt.exp_avg_sq)})
    finally:
        monkeypatch.setattr(calm.ops._tail, "flush", real)
        opt.close()
        calm.ops.set_noise_override(None)
    return grads, state, [d for d in deferred if d != (0, 0)]


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph_two_replays"])
def test_training_step_is_bit_identical_with_the_tail_on_and_off(hip, graphed, monkeypatch):
    """Nano-48, batch 4, the deterministic k-split.  Eager: every .grad of a backward, and the parameters, buffers and
    optimizer moments after a step, agree in every bit.  Graphed: the same state after a captured step replayed twice (the
    optimizer-side step releases .grad inside the graph).  With the tail on every backward flushed once (eager: two
    backwards; graphed: the warm-up step and the capture) with reductions and spectral-norm corrections in the queue; with
    it off nothing was queued."""
    prev = hip.gemm_set_option(hip.GEMM_OPT_DETERMINISTIC, 1)
    try:
        g_off, s_off, d_off = _train(False, graphed, monkeypatch)
        g_on, s_on, d_on = _train(True, graphed, monkeypatch)
    finally:
        hip.gemm_set_option(hip.GEMM_OPT_DETERMINISTIC, prev)
    assert d_off == []
    assert len(d_on) == 2 and all(r > 10 and n > 0 for r, n in d_on) and d_on[0] == d_on[1], d_on
    assert sorted(g_on) == sorted(g_off) and sorted(s_on) == sorted(s_off)
    assert graphed or len(g_on) > 10
    bad = [k for k in g_off if not torch.equal(g_on[k], g_off[k])]
    assert not bad, bad[:8]
    bad = [k for k in s_off if not torch.equal(s_on[k], s_off[k])]
    assert not bad, bad[:8]
