"""The generative job on a host without a GPU:
  * the three entry points of csrc/recon.hip are declared, exported and bound, the ABI version is still 7, CALM_RED_RECON = 8
    plans what the emulation plans, and every refusal comes before any launch;
  * the fp32 emulation of the kernels (tests/emulated_recon.py) agrees with the float64 checker (tests/recon_f64.py) on the
    shapes the GPU test uses within the measured allowance, the cases meet the condition the allowance needs, and the
    checker catches planted faults;
  * trainer.ReconMetrics, RegTrainStep on row tokens, evaluate(recon=True) alone and on two gloo ranks;
  * train(task="reg") on two gloo ranks: validation, EMA, samples, accumulation, exact resume, equality with a hand-written
    loop, the best checkpoint, the refusals, and train() without task being train(task="cls")."""
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
import recon_f64 as F  # noqa: E402
import emulated_recon as E  # noqa: E402
from emulated_backend import EmulatedBackend  # noqa: E402
from test_host_logic_cpu import build_model  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
HEADER = os.path.join(ROOT, "include", "calm_vit.h")
NEW = ("calm_recon_huber_rows_fwd", "calm_recon_huber_rows_bwd", "calm_recon_metrics")


@pytest.fixture(autouse=True)
def _restore_switch():
    prev = calm.backend.get_loss_kernels()
    yield
    calm.backend.set_loss_kernels(prev)


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_bound_and_the_scratch_plan_answers():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t|const char\*)\s+(calm_\w+)\s*\(", text, flags=re.M))
    lib = binding.load()
    for name in NEW:
        assert name in declared and name in binding.SIGNATURES and hasattr(lib, name), name
    assert [len(binding.SIGNATURES[n][1]) for n in NEW] == [7, 7, 13]
    assert int(re.search(r"#define\s+CALM_ABI_VERSION\s+(\d+)", raw).group(1)) == 7          # additions only
    assert binding.ABI_VERSION == 7 and lib.calm_abi_version() == 7
    assert re.search(r"CALM_RED_RECON\s*=\s*8\b", raw) and binding.RED_RECON == 8
    assert re.search(r"CALM_RED_EVAL\s*=\s*7\b", raw) and binding.RED_EVAL == 7
    assert re.search(r"CALM_RECON_ROWS\s*=\s*0\b", raw) and re.search(r"CALM_RECON_NCHW\s*=\s*1\b", raw)
    assert (binding.RECON_ROWS, binding.RECON_NCHW) == (0, 1)
    for B, S in F.SHAPES + F.EXTRA_SHAPES + [(256, 224), (3, 6), (1, 256), (1, 257), (2, 600), (1, 4096)]:
        assert int(lib.calm_reduce_scratch_floats(binding.RED_RECON, B, S)) == E.scratch_floats(B, S), (B, S)
    assert E.scratch_floats(256, 224) == 8 * 256 * 7 and E.scratch_floats(2, 600) == 8 * 2 * 19 * 3
    assert int(lib.calm_reduce_scratch_floats(binding.RED_RECON, 0, 48)) == 0
    assert int(lib.calm_reduce_scratch_floats(binding.RED_EVAL, 9, 1000)) == 36
    assert int(lib.calm_reduce_scratch_floats(99, 10, 10)) == 0


_P = 0x7f0000010000            # a fake, 16-byte aligned device address: every call below is turned down before any launch


def _metrics_args(**change):
    a = dict(tokens=_P, tokens_type=binding.ST_F32, target=_P, layout=binding.RECON_ROWS,
             mean=(ctypes.c_float * 3)(*F.MEAN), std=(ctypes.c_float * 3)(*F.STD), delta=1.0, want_ssim=1, sums=_P, B=2,
             S=48, partials=_P, stream=None)
    a.update(change)
    return list(a.values())


def test_every_refusal_comes_before_any_launch():
    lib = binding.load()
    call = lib.calm_recon_metrics
    for name in ("tokens", "target", "mean", "std", "sums", "partials"):
        assert call(*_metrics_args(**{name: None})) == binding.E_INVAL, name
    for kw in (dict(B=0), dict(B=-1), dict(S=0), dict(S=-48)):
        assert call(*_metrics_args(**kw)) == binding.E_INVAL, kw
    for st in (binding.ST_FP8_E4M3, binding.ST_FP8_E5M2, 7, -1):
        assert call(*_metrics_args(tokens_type=st)) == binding.E_INVAL, st
    for layout in (2, -1, 7):
        assert call(*_metrics_args(layout=layout)) == binding.E_INVAL, layout
    for S in (1, 6, 10):
        assert call(*_metrics_args(S=S)) == binding.E_UNSUPP, S                 # no 11 x 11 window fits
    assert call(*_metrics_args(S=4097)) == binding.E_UNSUPP
    assert call(*_metrics_args(S=4097, want_ssim=0)) == binding.E_UNSUPP
    assert call(*_metrics_args(S=4096, B=1 << 20)) == binding.E_UNSUPP          # 2^31 workgroups or more
    assert call(*_metrics_args(partials=_P + 4)) == binding.E_LAYOUT
    assert call(*_metrics_args(partials=_P + 8)) == binding.E_LAYOUT
    assert call(*_metrics_args(target=_P + 2)) == binding.E_LAYOUT
    assert call(*_metrics_args(tokens=_P + 2)) == binding.E_LAYOUT              # (fp32 tokens; bf16 tokens may sit there)
    assert call(*_metrics_args(tokens=_P + 1, tokens_type=binding.ST_BF16)) == binding.E_LAYOUT
    assert call(*_metrics_args(sums=_P + 4)) == binding.E_LAYOUT
    fwd, bwd = lib.calm_recon_huber_rows_fwd, lib.calm_recon_huber_rows_bwd
    ok_f, ok_b = [_P, _P, 1.0, _P, 1000, _P, None], [_P, _P, 1.0, _P, _P, 1000, None]
    for fn, ok, ptrs, n_at in ((fwd, ok_f, (0, 1, 3, 5), 4), (bwd, ok_b, (0, 1, 3, 4), 5)):
        for i in ptrs:
            args = list(ok)
            args[i] = None
            assert fn(*args) == binding.E_INVAL, (fn.__name__, i)
        for n, code in ((0, binding.E_INVAL), (-5, binding.E_INVAL), (1 << 31, binding.E_UNSUPP), (1 << 40, binding.E_UNSUPP)):
            args = list(ok)
            args[n_at] = n
            assert fn(*args) == code, (fn.__name__, n)
        args = list(ok)
        args[0] = _P + 2
        assert fn(*args) == binding.E_LAYOUT


# ---- emulation against the checker ----------------------------------------------------------------------------------------
def _emulate(tokens, target, fault=None, ssim=True):
    be = E.EmulatedReconBackend()
    be.recon_fault = fault
    sums = torch.zeros(8, dtype=torch.float64)
    B, S = tokens.shape[0], tokens.shape[1]
    be.recon_metrics(tokens, target, int(target.dim() == 4), F.MEAN, F.STD, 1.0, ssim, sums, B, S)
    return sums


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layout", ["rows", "nchw"])
@pytest.mark.parametrize("B,S", F.SHAPES + F.EXTRA_SHAPES)
def test_emulation_agrees_with_the_checker(B, S, layout, dtype):
    tokens, target = F.make_case(B, S, layout, dtype, nonfinite=B >= 3)
    ref = F.reference(tokens, target)
    bound, yard = F.allowance(tokens, target, ref, trainer.recon_metrics_torch)
    got = _emulate(tokens, target)
    print(f"\nrecon {B}x{S} {layout} {dtype}: yardstick {yard[[2, 3, 4, 6, 7]]}, emulation {F.errors(got, ref)[[2, 3, 4, 6, 7]]}")
    assert F.mismatches(got, ref, bound) == []
    assert np.isfinite(yard).all() and np.isfinite(ref).all()
    assert (ref[0], ref[1]) == (B, 2 if B >= 3 else 0)                    # the inputs hold what they promise
    no_ssim = _emulate(tokens, target, ssim=False)
    assert no_ssim[7] == 0.0 and F.mismatches(no_ssim, ref, bound, ssim=False) == []


def test_the_identical_image_sits_at_the_psnr_cap_with_ssim_one():
    tokens, target = F.make_case(2, 44, "nchw", torch.bfloat16)
    one = F.reference(tokens[1:], target[1:])
    assert one[2] == one[3] == one[4] == 0.0 and one[6] == 100.0 and one[7] == 1.0
    got = _emulate(tokens[1:], target[1:])
    assert got[6] == 100.0 and abs(float(got[7]) - 1.0) <= 1e-6


@pytest.mark.parametrize("S", [44, 48, 100])
def test_the_yardstick_is_finite_and_nonzero_on_the_constant_patch_and_the_clamped_regions(S):
    """The allowance is a multiple of the fp32 torch composition's own error, so that error has to exist where the kernel
    is most likely to differ: each region of make_case, cut out as a case of its own, leaves the composition with a finite,
    nonzero error in at least one real-valued slot (and in the SSIM slot on the constant patch, where E[x^2] - mu^2 cancels)."""
    tokens, target = F.make_case(2, S, "nchw", torch.float32, seed=1)
    tokens, target = tokens[:1], target[:1]                               # (image 1 equals its target)
    for name, (rows, cols) in F.regions(S).items():
        side = rows.stop - rows.start
        tk, tg = F.crop(tokens, target, rows, cols)
        ssim = side >= F.WIN
        ref = F.reference(tk, tg, ssim=ssim)
        _, yard = F.allowance(tk, tg, ref, trainer.recon_metrics_torch, ssim=ssim)
        assert np.isfinite(yard).all(), (name, yard)
        assert yard[[2, 3, 4]].max() > 0.0, (name, yard)
        if name == "constant":
            assert ssim and yard[7] > 0.0, (name, yard)
        else:
            px = np.clip(tg.double().numpy() * np.asarray(F.STD).reshape(1, 3, 1, 1) + np.asarray(F.MEAN).reshape(1, 3, 1, 1),
                         0, 1)
            assert px.min() == px.max() == (1.0 if name == "clamp_hi" else 0.0)          # saturated on this side


@pytest.mark.parametrize("fault,slot", [("unnormalised", "ssim"), ("bessel", "ssim"), ("halo_row", "ssim"),
                                        ("channel_swap", "psnr"), ("nonfinite_leak", "elements")])
def test_the_checker_catches_planted_faults(fault, slot):
    tokens, target = F.make_case(3, 16, "rows", torch.float32, nonfinite=True)
    ref = F.reference(tokens, target)
    bound, _ = F.allowance(tokens, target, ref, trainer.recon_metrics_torch)
    assert F.mismatches(_emulate(tokens, target), ref, bound) == []
    bad = F.mismatches(_emulate(tokens, target, fault=fault), ref, bound)
    assert bad and any(b.startswith(slot) for b in bad), (fault, bad)


@pytest.mark.parametrize("n", F.HUBER_SIZES)
def test_emulated_rows_huber_agrees_with_float64(n):
    a, b = F.huber_case(n)
    want, dwant = F.huber_reference(a, b)
    with calm.backend.use_backend(E.EmulatedReconBackend()):
        x = a.clone().requires_grad_(True)
        loss = calm.ops.HuberRowsFn.apply(x, b, 1.0)
        loss.backward()
    ref32 = torch.nn.functional.huber_loss(a, b)
    assert abs(float(loss.detach()) - want) <= 4 * abs(float(ref32) - want) + 1e-6 * abs(want)
    assert float((x.grad.double() - dwant).abs().max()) <= 1e-6 * float(dwant.abs().max())


# ---- trainer.ReconMetrics ----------------------------------------------------------------------------------------------------
def _means(ref, ssim=True):
    imgs = max(ref[0] - ref[1], 1)
    return {"n": int(ref[0]), "nonfinite": int(ref[1]), "huber": ref[2] / max(ref[5], 1), "mae": ref[3] / max(ref[5], 1),
            "mse": ref[4] / max(ref[5], 1), "psnr": ref[6] / imgs, "ssim": ref[7] / imgs if ssim else None}


def _assert_close(rep, want, what):
    """A report of either fp32 path against the float64 means.  The sums and PSNR are fp32 compositions of a few thousand
    terms: 1e-5 relative is ~100 ulp.  An SSIM value carries the cancellation of E[x^2] - mu^2 — one rounding of a second
    moment of up to 1 (6e-8) against C2 = 9e-4 in the denominator, about 7e-5 of the value per position in the plain torch
    composition — so the mean SSIM gets 2e-5 absolute on top."""
    for k in ("huber", "mae", "mse", "psnr"):
        assert abs(rep[k] - want[k]) <= 1e-5 * abs(want[k]), (what, k, rep[k], want[k])
    assert abs(rep["ssim"] - want["ssim"]) <= 1e-5 * abs(want["ssim"]) + 2e-5, (what, rep["ssim"], want["ssim"])


@pytest.mark.parametrize("layout", ["rows", "nchw"])
def test_recon_metrics_on_cpu_tensors_equals_the_checker_on_both_paths(layout):
    tokens, target = F.make_case(3, 16, layout, torch.bfloat16, nonfinite=True)
    more, more_t = F.make_case(2, 16, layout, torch.bfloat16, seed=5)
    ref = F.reference(tokens, target) + F.reference(more, more_t)
    want = _means(ref)
    be = E.EmulatedReconBackend()
    reports = []
    with calm.backend.use_backend(be):
        for on in (False, True):
            calm.backend.set_loss_kernels(on)
            m = trainer.ReconMetrics(F.MEAN, F.STD)
            address = m.sums.data_ptr()
            m.update(tokens, target)
            m.update(more, more_t)
            assert getattr(be, "recon_calls", 0) == (2 if on else 0)
            rep = m.read()
            reports.append(rep)
            assert set(rep) == {"n", "nonfinite", "huber", "mae", "mse", "psnr", "ssim"}
            assert (rep["n"], rep["nonfinite"]) == (5, 2) and float(m.sums[5]) == 3 * 3 * 16 * 16
            _assert_close(rep, want, on)
            json.dumps(rep)
            m.reset()
            assert m.sums.data_ptr() == address and float(m.sums.abs().sum()) == 0.0
            empty = m.read()
            assert (empty["n"], empty["huber"], empty["psnr"], empty["ssim"]) == (0, 0.0, 0.0, 0.0)
    calm.backend.set_loss_kernels(False)
    small = trainer.ReconMetrics(F.MEAN, F.STD, ssim=False)
    tk, tg = F.make_case(2, 6, layout)
    small.update(tk, tg)                                                    # the 6 x 6 shapes stay servable without SSIM
    rep = small.read()
    assert rep["ssim"] is None and rep["n"] == 2 and abs(rep["huber"] - _means(F.reference(tk, tg, ssim=False))["huber"]) < 1e-6
    with pytest.raises(ValueError, match="SSIM"):
        trainer.ReconMetrics(F.MEAN, F.STD).update(tk, tg)
    with pytest.raises(ValueError, match="tokens"):
        trainer.ReconMetrics(F.MEAN, F.STD).update(torch.zeros(2, 16, 47), torch.zeros(2, 16, 48))
    with pytest.raises(ValueError, match="target"):
        trainer.ReconMetrics(F.MEAN, F.STD).update(torch.zeros(2, 16, 48), torch.zeros(1, 16, 48))
    with pytest.raises(ValueError, match="mean"):
        trainer.ReconMetrics((0.5, 0.5), F.STD)


# ---- RegTrainStep on row tokens ---------------------------------------------------------------------------------------------
def _rows(x):
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], x.shape[2], 3 * x.shape[3]).contiguous()


def test_reg_train_step_takes_row_tokens_and_equals_the_image_step():
    """The row tokens are the channels-last image: the step on them computes what the step on the image computes (the first
    Block skips its tokenisation), through HuberRowsFn when the loss kernels are on and stock torch otherwise."""
    x = torch.randn(2, 3, 48, 48, generator=torch.Generator().manual_seed(4)) * 0.5
    losses = {}
    for kind in ("image", "rows", "rows_kernels"):
        be = E.EmulatedReconBackend()
        with calm.backend.use_backend(be):
            calm.backend.set_loss_kernels(kind == "rows_kernels")
            torch.manual_seed(8)
            m = build_model("nano48_gen", None).train()
            step = trainer.RegTrainStep(m, trainer.make_optimizer(m))
            torch.manual_seed(9)
            loss, img = step(x if kind == "image" else _rows(x))
            assert tuple(img.shape) == (2, 3, 48, 48)
            assert getattr(be, "huber_rows_calls", 0) == (1 if kind == "rows_kernels" else 0)
            losses[kind] = (float(loss), [p.detach().clone() for p in step.params])
    assert losses["rows"][0] == losses["image"][0]
    assert abs(losses["rows_kernels"][0] - losses["rows"][0]) <= 1e-6 * abs(losses["rows"][0])
    assert all(torch.equal(a, b) for a, b in zip(losses["rows"][1], losses["image"][1]))


def test_mixup_with_lam_one_is_the_identity_on_a_uint8_batch():
    """train(task="reg", device_collate=True) hands the collate the decisions (mix-up, lam = 1, no box): the output is the
    normalised, flipped batch whatever the partner sample holds."""
    g = torch.Generator().manual_seed(2)
    u8 = torch.randint(0, 256, (4, 3, 12, 12), dtype=torch.uint8, generator=g)
    flips = torch.tensor([1, 0, 1, 0], dtype=torch.uint8)
    mean, std = trainer.DeviceCollate.MEAN, trainer.DeviceCollate.STD
    outs = []
    for batch in (u8, torch.cat([u8[:1], u8[1:].flip(0)])):               # sample 0 with two different partners
        out = torch.empty(4, 3, 12, 12)
        EmulatedBackend().collate_mix(batch, flips if batch is u8 else torch.cat([flips[:1], flips[1:].flip(0)]), out, 1, 1.0,
                                      None, mean, std)
        outs.append(out)
    plain = (u8.float() / 255.0 - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)
    plain = torch.where(flips.view(4, 1, 1, 1).bool(), plain.flip(-1), plain)
    assert torch.allclose(outs[0], plain, rtol=0, atol=1e-6)
    assert torch.equal(outs[0][0], outs[1][0])


# ---- evaluate(recon=True) -------------------------------------------------------------------------------------------------
class _GenSet(torch.utils.data.Dataset):
    """Images [3,48,48] in normalised space with a label nobody reads."""

    def __init__(self, n=16, seed=7):
        self.x = torch.randn(n, 3, 48, 48, generator=torch.Generator().manual_seed(seed)) * 0.5

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], 0


def _gen_model(seed=3):
    torch.manual_seed(seed)
    return build_model("nano48_gen", None).train()


def _val_batches(data, rank=0, world=1, bs=2, with_labels=True):
    shard = trainer.validation_shard(data, rank, world)
    xs = [torch.stack([shard[i][0] for i in range(j, min(j + bs, len(shard)))]) for j in range(0, len(shard), bs)]
    return [(x, torch.zeros(len(x), dtype=torch.int64)) for x in xs] if with_labels else xs


def test_evaluate_recon_reports_the_models_own_outputs_and_refuses_report():
    with calm.backend.use_backend(E.EmulatedReconBackend()):
        m = _gen_model()
        data = _GenSet(5)
        rep = trainer.evaluate(m, _val_batches(data), recon=True)
        bare = trainer.evaluate(m, _val_batches(data, with_labels=False), recon=True, lean=True)
        rows = trainer.evaluate(m, [_rows(x) for x in _val_batches(data, with_labels=False)], recon=True)
        assert m.training
        with torch.no_grad():
            tokens = m.eval()(data.x)[0]
        m.train()
        want = _means(F.reference(tokens.reshape(5, 48, 144), data.x))
        with pytest.raises(ValueError, match="exclude"):
            trainer.evaluate(m, _val_batches(data), recon=True, report=True)
        with pytest.raises(ValueError, match="at least one batch"):
            trainer.evaluate(m, [], recon=True)
    assert rep == bare == rows                                              # the same numbers whatever the batch form
    assert rep["n"] == 5 and rep["nonfinite"] == 0
    _assert_close(rep, want, "evaluate")


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
    with calm.backend.use_backend(E.EmulatedReconBackend()):
        rep = trainer.evaluate(_gen_model(), _val_batches(_GenSet(5), rank, world), recon=True)
    json.dump(rep, open(os.path.join(outdir, f"rep{rank}.json"), "w"))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_gloo_ranks_produce_the_single_process_report(tmp_path):
    mp.spawn(_evaluate_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    with calm.backend.use_backend(E.EmulatedReconBackend()):
        one = trainer.evaluate(_gen_model(), _val_batches(_GenSet(5)), recon=True)
    for rank in range(2):
        rep = json.load(open(os.path.join(tmp_path, f"rep{rank}.json")))
        assert set(rep) == set(one) and rep["n"] == one["n"] == 5 and rep["nonfinite"] == 0
        for k in ("huber", "mae", "mse", "psnr", "ssim"):                   # (fp32 batch sums, other batch boundaries)
            assert abs(rep[k] - one[k]) <= 1e-6 * abs(one[k]), k


# ---- train(task="reg") on two gloo ranks -----------------------------------------------------------------------------------
EPOCHS = 2
N_TRAIN, N_VAL, BATCH = 16, 5, 2            # 8 samples per rank: 4 steps per epoch


def _reg_run(outdir, tag, seed=50, rank=0, **kw):
    torch.manual_seed(seed + rank)
    m = build_model("nano48_gen", None).train()
    path = os.path.join(outdir, tag, "model_reg.pth")
    with calm.backend.use_backend(E.EmulatedReconBackend()):
        out = trainer.train(m, trainer.make_optimizer(m), None, use_gpu=False, dataset=_GenSet(N_TRAIN), epochs=EPOCHS,
                            batch_size=BATCH, checkpoint_path=path, log_every=1000, task="reg", ema=0.9,
                            val_dataset=_GenSet(N_VAL, seed=9), val_batch_size=2, **kw)
    assert out.training
    return out


def _hand_loop(outdir, rank, world, seed=50):
    """What train(task="reg") has to equal: DistributedSampler(seed 2006) order, default collate, RegTrainStep, the cosine
    schedule per epoch, and a lean recon evaluation of the rank's shard behind every epoch with the RNG put back."""
    from torch.utils.data import DataLoader, DistributedSampler
    torch.manual_seed(seed + rank)
    m = build_model("nano48_gen", None).train()
    lines = []
    with calm.backend.use_backend(E.EmulatedReconBackend()):
        opt = trainer.make_optimizer(m)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=EPOCHS, eta_min=1e-6)
        trainer.sync_module_states(m)
        step = trainer.RegTrainStep(m, opt, trainer.BucketedGradReducer(m), max_norm=1.0, kl_weight=0.1)
        data = _GenSet(N_TRAIN)
        sampler = DistributedSampler(data, num_replicas=world, rank=rank, shuffle=True, seed=2006)
        loader = DataLoader(data, batch_size=BATCH, sampler=sampler, num_workers=0)
        n = 0
        for epoch in range(EPOCHS):
            sampler.set_epoch(epoch)
            for x, _ in loader:
                step(x)
                n += 1
            rng = torch.get_rng_state()
            rep = trainer.evaluate(m, _val_batches(_GenSet(N_VAL, seed=9), rank, world), recon=True, lean=True)
            torch.set_rng_state(rng)
            lines.append({"epoch": epoch + 1, "step": n, **rep})
            sched.step()
    return m, lines


def _train_worker(rank, world, ports, outdir):
    saves = []
    real_save = torch.save
    snap = {n: os.path.join(outdir, f"{n}.snap") for n in "abc"}
    runs = [("a", dict(snapshot_path=snap["a"], samples_dir=os.path.join(outdir, "samples"))),
            ("b", dict(snapshot_path=snap["b"], snapshot_every=3, max_steps=3)),
            ("c", dict(snapshot_path=snap["c"], resume=snap["b"], seed=51)),
            ("acc", dict(accumulate=2))]
    for (tag, kw), port in zip(runs, ports):
        _join(rank, world, port)
        path = os.path.join(outdir, tag, "model_reg.pth")
        if tag == "c":                                                       # the resumed run appends to the cut run's log
            os.makedirs(os.path.dirname(path), exist_ok=True)
            if rank == 0:
                log = os.path.join(outdir, "b", "model_reg_val.jsonl")
                open(os.path.join(outdir, "c", "model_reg_val.jsonl"), "w").write(open(log).read() if os.path.exists(log) else "")
        epoch_of = {}

        def spy(obj, f, *a, **k):
            if isinstance(f, str) and "_best" in f:
                saves.append((tag, os.path.basename(f), epoch_of.get("n", 0)))
            if isinstance(f, str) and f == path:
                epoch_of["n"] = epoch_of.get("n", 0) + 1                      # the per-epoch checkpoint comes first
            return real_save(obj, f, *a, **k)
        torch.save = spy
        try:
            out = _reg_run(outdir, tag, rank=rank, **kw)
        finally:
            torch.save = real_save
        torch.save(out.state_dict(), os.path.join(outdir, f"{tag}_rank{rank}.pt"))
        if tag in ("a", "c"):
            torch.save([s.clone() for s in out._calm_ema.shadows], os.path.join(outdir, f"{tag}_ema_rank{rank}.pt"))
    _join(rank, world, ports[-1])
    torch.distributed.init_process_group(backend="gloo")
    m, lines = _hand_loop(outdir, rank, world)
    torch.distributed.destroy_process_group()
    torch.save(m.state_dict(), os.path.join(outdir, f"hand_rank{rank}.pt"))
    if rank == 0:
        json.dump(saves, open(os.path.join(outdir, "saves.json"), "w"))
        json.dump(lines, open(os.path.join(outdir, "hand_lines.json"), "w"))


def _lines(outdir, tag):
    return [json.loads(x) for x in open(os.path.join(outdir, tag, "model_reg_val.jsonl")) if x.strip()]


@pytest.mark.timeout(900)
def test_train_reg_on_two_gloo_ranks(tmp_path):
    d = str(tmp_path)
    mp.spawn(_train_worker, args=(2, [_free_port() for _ in range(5)], d), nprocs=2, join=True)
    load = lambda name: torch.load(os.path.join(d, name))                   # noqa: E731
    a0 = load("a_rank0.pt")
    for r in range(2):
        a, c, hand = load(f"a_rank{r}.pt"), load(f"c_rank{r}.pt"), load(f"hand_rank{r}.pt")
        assert set(a) == set(c) == set(hand) == set(a0)
        for k in a:
            assert torch.equal(a[k], a0[k]), k                                # the ranks hold one model
            assert torch.equal(a[k], c[k]), f"resumed run differs at {k}"
            assert torch.equal(a[k], hand[k]), f"hand-written loop differs at {k}"
        assert all(torch.equal(x, y) for x, y in zip(load(f"a_ema_rank{r}.pt"), load(f"c_ema_rank{r}.pt")))
    assert trainer.TrainState.read_header(os.path.join(d, "b.snap"))[0]["host"]["progress"] == {"epoch": 0, "batch": 3, "step": 3}
    la, lc, lacc = _lines(d, "a"), _lines(d, "c"), _lines(d, "acc")
    hand_lines = json.load(open(os.path.join(d, "hand_lines.json")))
    assert [x["epoch"] for x in la] == [1, 2] and [x["step"] for x in la] == [4, 8]
    assert [x["step"] for x in lacc] == [2, 4]                               # accumulate = 2: optimizer steps
    lb = _lines(d, "b")                                                      # the cut run validated once, at step 3
    assert [(x["epoch"], x["step"]) for x in lb] == [(1, 3)]
    assert lc == lb + la                                                     # the resumed run appends the uninterrupted lines
    assert [{k: v for k, v in x.items() if k != "ema"} for x in la] == hand_lines
    for x in la + lacc:
        assert set(x) == {"epoch", "step", "n", "nonfinite", "huber", "mae", "mse", "psnr", "ssim", "ema"}
        assert x["n"] == N_VAL and x["nonfinite"] == 0 and x["huber"] > 0 and x["psnr"] > 0 and -1 <= x["ssim"] <= 1
        assert set(x["ema"]) == {"n", "nonfinite", "huber", "mae", "mse", "psnr", "ssim"}
    acc = load("acc_rank0.pt")
    assert any(not torch.equal(acc[k], a0[k]) for k in a0)                   # half as many steps: another model
    saves = [tuple(s) for s in json.load(open(os.path.join(d, "saves.json")))]
    for tag, lines in (("a", la), ("acc", lacc)):
        for name, key in (("model_reg_best.pth", None), ("model_reg_ema_best.pth", "ema")):
            hub = [(x if key is None else x[key])["huber"] for x in lines]
            improved = [e + 1 for e, h in enumerate(hub) if h < min(hub[:e], default=float("inf"))]      # strictly lower
            assert [e for t, n, e in saves if t == tag and n == name] == improved, (tag, name, hub)
            assert os.path.exists(os.path.join(d, tag, name))
    # the resumed run took the best so far from the log it appends to: it saves only what improves on the cut run's values
    for name, key in (("model_reg_best.pth", None), ("model_reg_ema_best.pth", "ema")):
        hub = [(x if key is None else x[key])["huber"] for x in lc]
        improved = [e for e, h in enumerate(hub) if e >= 1 and h < min(hub[:e])]
        assert [e for t, n, e in saves if t == "c" and n == name] == improved, (name, hub)
    for tag in ("a", "acc"):
        assert os.path.exists(os.path.join(d, tag, "model_reg.pth")) and os.path.exists(os.path.join(d, tag, "model_reg_ema.pth"))
    pngs = sorted(os.listdir(os.path.join(d, "samples")))
    assert pngs == [f"sample_{i}.png" for i in range(BATCH)]
    assert open(os.path.join(d, "samples", pngs[0]), "rb").read(8) == b"\x89PNG\r\n\x1a\n"


def test_best_huber_comes_back_from_an_existing_log(tmp_path):
    log = os.path.join(tmp_path, "m_val.jsonl")
    assert trainer._val_best_so_far(log, "huber", True) == {}
    with open(log, "w") as f:
        f.write(json.dumps({"epoch": 1, "step": 2, "huber": 0.5, "ema": {"huber": 0.75}}) + "\n")
        f.write(json.dumps({"epoch": 2, "step": 4, "huber": 0.25, "ema": {"huber": 0.875}}) + "\n\n")
        f.write(json.dumps({"epoch": 3, "step": 6, "huber": 0.375}) + "\n")
    assert trainer._val_best_so_far(log, "huber", True) == {"huber": 0.25, "ema_huber": 0.75}
    assert trainer._val_best_so_far(log) == {}                              # (no top-1 in a generative log)


# ---- refusals, and the default -----------------------------------------------------------------------------------------------
class _Flagged(torch.nn.Linear):
    def __init__(self, generate):
        super().__init__(4, 4)
        self.generate = generate


def test_task_argument_errors_come_before_any_process_group():
    data = _GenSet(4)
    sgd = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    kw = dict(use_gpu=False, dataset=data, epochs=1, batch_size=2)
    plain = torch.nn.Linear(4, 4)                                            # no `generate` attribute: not judged
    for model, bad, match in ((plain, dict(task="gen"), "task"), (plain, dict(task=None), "task"),
                              (plain, dict(task="reg", graph=True), "graph"),
                              (plain, dict(task="reg", device_metrics=True), "device_metrics"),
                              (_Flagged(False), dict(task="reg"), "generate"),
                              (_Flagged(True), dict(task="cls"), "generate"), (_Flagged(True), dict(), "generate")):
        with pytest.raises(ValueError, match=match):
            trainer.train(model, sgd, **kw, **bad)
    assert not torch.distributed.is_initialized()


class _ClsSet(torch.utils.data.Dataset):
    def __init__(self, n=8):
        g = torch.Generator().manual_seed(7)
        self.x = torch.randn(n, 3, 32, 32, generator=g)
        self.y = torch.randint(0, 10, (n,), generator=g)

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return self.x[i], int(self.y[i])


def test_train_without_task_is_the_classification_job(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "1")
    outs = []
    for kw in (dict(), dict(task="cls")):
        torch.manual_seed(50)
        m = build_model("tiny32_cls", None).train()
        with calm.backend.use_backend(E.EmulatedReconBackend()):
            outs.append(trainer.train(m, trainer.make_optimizer(m), None, use_gpu=False, dataset=_ClsSet(), epochs=1,
                                      batch_size=4, num_classes=10, log_every=1000, **kw).state_dict())
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0])
