"""LAMB without a GPU: the float64 checker (tests/lamb_f64.py) on the fp32 emulation of calm_optim_step_lamb
(tests/emulated_lamb.py) and on its planted faults, the C-ABI addition (calm_lamb_hparams, the two entry points, the
refusals), FusedClipAdamW(lamb=) with the torch fallback on CPU parameters against a plain per-tensor LAMB in float64,
train(lamb=) on one and two gloo ranks against a hand-written loop, snapshots, and every refusal."""
import ctypes
import math
import os
import socket
import subprocess
import sys
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import calm_vit_dte_amd as calm  # noqa: E402
import lamb_f64 as lf  # noqa: E402
import optim_groups_f64 as gf  # noqa: E402
import tail_f64 as tf  # noqa: E402
from emulated_backend import EmulatedBackend  # noqa: E402
from emulated_lamb import FAULTS, lamb_step  # noqa: E402
from test_host_logic_cpu import build_model  # noqa: E402
from test_snapshot_cpu import _TinySet  # noqa: E402
from importlib import import_module  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
lamb_step_torch, LambHparams = trainer.lamb_step_torch, binding.LambHparams      # (what this module is about)
TABLE = lf.TABLE


def names(failures):
    return {n for n, _ in failures}


def _emulate(c, fault=None, **kw):
    return lamb_step(c["recs"], c["grads"], c["hp"], c["scale"], c["step"], c["lamb_hp"], lr_dev=c["lr_dev"], groups=c["groups"],
                     group_hp=c["group_hp"], fault=fault, **kw)


# ---- the checker on the emulation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,grouped,mode", lf.RUNS, ids=[f"{n}-{'grouped' if g else 'one'}-{m}" for n, g, m in lf.RUNS])
def test_emulation_inside_every_bound(name, grouped, mode):
    c = lf.case(name, grouped, mode)
    ref, bound = c["ref"], c["bound"]
    got = _emulate(c)
    worst, _ = lf.check(got, ref, bound)
    _, _, checked = lf.check_length(got, ref, bound)
    print(f"lamb {name} {grouped} {mode}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()) + f" lengths={checked}")
    assert ref["found_inf"] == 0.0 and ref["step"] == c["step"] + 1
    # the two overridden records: exact zeros, trust exactly 1 (the clip is above or below 1: min(1, clip))
    always, clipped = lf.MODES[mode]
    one = min(1.0, c["lamb_hp"][0]) if clipped else 1.0
    assert ref["wn"][lf.ZERO_W] == 0.0 and ref["un"][lf.ZERO_W] > 0 and ref["trust"][lf.ZERO_W] == one
    assert ref["un"][lf.ZERO_ALL] == 0.0 and ref["trust"][lf.ZERO_ALL] == one
    adapted = [x for x in ref["ratio"] if x is not None]
    if grouped or always or c["sc"]["wd"] != 0.0:
        assert len(adapted) > 100
    else:
        assert not adapted                                   # wd = 0 without always_adapt: plain Adam everywhere
    if grouped and not always:                               # GROUP_HP's wd = 0 group does not adapt, its lr = 0 group does
        assert all(ref["ratio"][t] is None for t, g in enumerate(c["groups"]) if g == 1)
        assert sum(ref["ratio"][t] is not None for t, g in enumerate(c["groups"]) if g == 2) > 50
    if clipped and adapted:                                  # the clip clips some tensors and leaves others
        hit, free = lf.clipped_kinds(ref, bound, c["lamb_hp"][0])
        assert hit > 10 and free > 10, (hit, free)
    assert checked == sum(1 for x, tr in zip(ref["ratio"], ref["trust"]) if x is not None and x == tr)


@pytest.mark.parametrize("grouped", [False, True], ids=["one", "grouped"])
@pytest.mark.parametrize("nonfinite", [c[0] for c in tf.optim_nonfinite_cases(TABLE)])
def test_emulation_with_a_non_finite_gradient(nonfinite, grouped):
    c = lf.case("clip_t1000", grouped, "always_clip", nonfinite)
    assert c["ref"]["found_inf"] == 1.0
    before = torch.rand(len(TABLE), 3)
    got = _emulate(c, trust_before=before)
    lf.check_skipped(got, tf.optim_flat(c["recs"]), c["step"], before)


# the run each fault shows in — (scenario, grouped, mode, non-finite case) — and the fields the checker must name
PLANTED = {"norm_without_decay": (("clip_t1000", False, "plain", None), {"un", "trust", "p"}),
           "trust_per_chunk": (("clip_t1000", False, "plain", None), {"p"}),
           "adapt_without_decay": (("clip_t1000", True, "plain", None), {"trust", "p"}),
           "no_bc1": (("below_t2", False, "plain", None), {"un", "trust"}),
           "no_bc2": (("below_t2", False, "plain", None), {"un", "trust"}),
           "w_norm_after_update": (("clip_t1000", False, "plain", None), {"wn", "trust"}),
           "clip_ignored": (("clip_t1000", False, "clip", None), {"trust", "p"}),
           "u_from_old_m": (("clip_t1000", False, "plain", None), {"p"}),
           "neighbour_trust": (("clip_t1000", False, "plain", None), {"p"}),
           "squared_norms": (("clip_t1000", False, "plain", None), {"wn", "un", "trust", "p"}),
           "write_on_found_inf": (("clip_t1000", False, "plain", "nan_sn"), {"p", "m", "v", "trust"})}


@pytest.mark.parametrize("fault", FAULTS)
def test_checker_rejects_the_planted_fault(fault):
    run, must = PLANTED[fault]
    c = lf.case(*run)
    if run[3] is None:
        failures = lf.check(_emulate(c, fault), c["ref"], c["bound"], strict=False)[1]
        failures += lf.check_length(_emulate(c, fault), c["ref"], c["bound"], strict=False)[1]
        lf.check(_emulate(c), c["ref"], c["bound"])          # the clean emulation on the same inputs: strict
    else:
        before = torch.tensor([[0.0, 0.0, 1.0]] * len(TABLE))
        failures = lf.check_skipped(_emulate(c, fault), tf.optim_flat(c["recs"]), c["step"], before, strict=False)[1]
        lf.check_skipped(_emulate(c), tf.optim_flat(c["recs"]), c["step"], before)
    assert must <= names(failures), (fault, failures)


def test_planted_faults_cover_the_list():
    assert set(PLANTED) == set(FAULTS) and len(FAULTS) == 11
    assert any(e["numel"] > tf.OPT_CHUNK for e in TABLE)                            # trust_per_chunk has tensors to hit
    assert any(w == 0.0 for _, w in gf.GROUP_HP) and any(lr == 0.0 for lr, _ in gf.GROUP_HP)


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------
def test_lamb_hparams_match_the_header():
    fields = [n for n, _ in LambHparams._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "calm_vit.h"\nint main(void){printf("%zu", sizeof(calm_lamb_hparams));\n' + \
          "".join(f'printf(" %zu", offsetof(calm_lamb_hparams, {f}));\n' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert fields == ["trust_clip", "always_adapt"]
    assert got == [8, 0, 4]
    assert got == [ctypes.sizeof(LambHparams)] + [getattr(LambHparams, f).offset for f in fields]


def test_abi_version_stays_and_the_scratch_query_needs_no_gpu():
    lib = binding.load()
    assert lib.calm_abi_version() == binding.ABI_VERSION == 7
    assert {"calm_optim_step_lamb", "calm_optim_lamb_scratch_floats"} <= set(binding.SIGNATURES)
    _, n_chunks = tf.optim_chunks(TABLE)
    # calm_optim_step's 6 per tensor, 4 globals and 3 per chunk, then sum w^2 and sum u^2 per chunk
    assert lib.calm_optim_lamb_scratch_floats(len(TABLE), n_chunks) == 6 * len(TABLE) + 4 + 5 * n_chunks
    assert lib.calm_optim_lamb_scratch_floats(521, 2700) == 6 * 521 + 4 + 5 * 2700
    assert lib.calm_optim_lamb_scratch_floats(0, 5) < 0 and lib.calm_optim_lamb_scratch_floats(5, 0) < 0


_P = 0x7f0000010000          # a fake, 16-byte aligned device address: every call below is refused before any launch
NAN = float("nan")
# positions: 0 tensors_dev, 1 n_tensors, 2 chunk_tensor_dev, 3 n_chunks, 4 scratch, 5 hparams, 6 lamb_hparams, 7 groups_dev,
# 8 n_groups, 9 grad_scale, 10 stats_out, 11 trust_out, 12 step_dev, 13 lr_dev, 14 stream
REFUSED = [({0: None}, "null tensors_dev"), ({2: None}, "null chunk_tensor_dev"), ({4: None}, "null scratch"),
           ({5: None}, "null hparams"), ({6: None}, "null lamb_hparams"), ({10: None}, "null stats_out"),
           ({1: 0}, "n_tensors 0"), ({1: -3}, "n_tensors negative"), ({3: 0}, "n_chunks 0"),
           ({12: None, "step": 0}, "no step_dev and step 0"), ({"beta1": 1.0}, "beta1 1"), ({"beta1": -0.1}, "beta1 negative"),
           ({"beta2": 1.0}, "beta2 1"), ({"beta2": -0.1}, "beta2 negative"), ({"lr": -1e-3}, "lr negative without groups"),
           ({"trust_clip": -1.0}, "trust_clip negative"), ({"trust_clip": NAN}, "trust_clip NaN"),
           ({"always_adapt": 2}, "always_adapt 2"), ({"always_adapt": -1}, "always_adapt -1"),
           ({7: _P, 8: 0}, "groups_dev with n_groups 0"), ({7: _P, 8: -2}, "groups_dev with n_groups negative")]


@pytest.mark.parametrize("change,what", REFUSED, ids=[w for _, w in REFUSED])
def test_calm_optim_step_lamb_refuses_before_any_launch(change, what):
    lib, change = binding.load(), dict(change)
    h = binding.OptimHparams(change.pop("lr", 1e-3), change.pop("beta1", 0.9), change.pop("beta2", 0.999), 1e-8, 0.05, 1.0,
                             change.pop("step", 1))
    lh = LambHparams(change.pop("trust_clip", 10.0), change.pop("always_adapt", 0))
    args = [_P, 3, _P, 5, _P, ctypes.byref(h), ctypes.byref(lh), None, 0, None, _P, None, _P, None, None]
    for i, v in change.items():
        args[i] = v
    assert lib.calm_optim_step_lamb(*args) == binding.E_INVAL, what


# ---- the torch fallback and FusedClipAdamW(lamb=) on CPU parameters ----------------------------------------------------------
@pytest.mark.parametrize("name,grouped,mode", [("clip_t1000", False, "clip"), ("scaled_t100000", True, "always"),
                                               ("lr_dev", False, "always_clip"), ("below_t2", True, "plain")])
def test_fallback_on_the_table_inside_every_bound(name, grouped, mode):
    """lamb_step_torch on tail_f64's table.  It has no lr_dev: the rate arrives in hp, as FusedClipAdamW hands it over."""
    c = lf.case(name, grouped, mode)
    recs = [dict(r, param=r["param"].clone(), exp_avg=r["exp_avg"].clone(), exp_avg_sq=r["exp_avg_sq"].clone()) for r in c["recs"]]
    if grouped:
        recs = gf.with_groups(recs, c["groups"])
    hp = c["hp"] if c["lr_dev"] is None else (c["lr_dev"],) + tuple(c["hp"][1:])
    step_dev, stats, trust = torch.tensor([c["step"]], dtype=torch.int32), torch.zeros(2), torch.zeros(len(TABLE), 3)
    lamb_step_torch(recs, step_dev, c["grads"], hp, c["lamb_hp"], c["group_hp"],
                            torch.tensor([c["scale"]]) if c["scale"] else None, stats, trust)
    got = dict(tf.optim_flat(recs), norm=float(stats[0]), found_inf=float(stats[1]), step=int(step_dev), trust=trust)
    lf.check(got, c["ref"], c["bound"])
    lf.check_length(got, c["ref"], c["bound"])


def test_fallback_skips_a_non_finite_step():
    c = lf.case("clip_t1000", True, "always_clip", "inf_last")
    recs = gf.with_groups([dict(r, param=r["param"].clone(), exp_avg=r["exp_avg"].clone(), exp_avg_sq=r["exp_avg_sq"].clone())
                           for r in c["recs"]], c["groups"])
    step_dev, stats, trust = torch.tensor([c["step"]], dtype=torch.int32), torch.zeros(2), torch.rand(len(TABLE), 3)
    before = trust.clone()
    lamb_step_torch(recs, step_dev, c["grads"], c["hp"], c["lamb_hp"], c["group_hp"], None, stats, trust)
    got = dict(tf.optim_flat(recs), norm=float(stats[0]), found_inf=float(stats[1]), step=int(step_dev), trust=trust)
    lf.check_skipped(got, tf.optim_flat(c["recs"]), c["step"], before)


def _batch(seed=0, B=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 32, 32, generator=g), torch.softmax(torch.randn(B, 10, generator=g), 1)


def _bits(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors]).clone().view(torch.int32)


def _flat_records(opt):
    flat = lambda t: t.detach().clone().reshape(-1)                                # noqa: E731  (tail_f64's records are flat)
    return [dict(param=flat(r["param"]), exp_avg=flat(r["exp_avg"]), exp_avg_sq=flat(r["exp_avg_sq"]), sn=None if r["sn"] is None else
                 tuple(t.detach().clone().reshape(-1) if torch.is_tensor(t) else t for t in r["sn"])) for r in opt._records]


def plain_lamb64(recs, gcorr, lr, wd_of, b1, b2, eps, t, clip_coef, trust_clip, always):
    """An independent LAMB in float64, tensor by tensor, from the corrected gradients: the textbook rule (You et al. 2020,
    timm's choice of which tensors adapt), written without looking at the header's order of operations."""
    out = []
    for k, (r, g) in enumerate(zip(recs, gcorr)):
        w, m, v = (r[n].double().reshape(-1) for n in ("param", "exp_avg", "exp_avg_sq"))
        g = g * clip_coef
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        update = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps) + wd_of(k) * w
        trust = 1.0
        if (always or wd_of(k) != 0.0) and float(w.norm()) > 0 and float(update.norm()) > 0:
            trust = float(w.norm() / update.norm())
        if trust_clip:
            trust = min(trust, trust_clip)
        out.append((w - lr * trust * update, trust))
    return out


@pytest.mark.parametrize("lamb", [True, {"trust_clip": 0.5, "always_adapt": True}], ids=["default", "clip_always"])
def test_fused_optimizer_with_lamb_on_cpu_parameters_against_a_plain_lamb_in_float64(lamb):
    with calm.backend.use_backend(EmulatedBackend()):
        torch.manual_seed(4)
        m = build_model("tiny32_cls", None).train()
        opt = trainer.FusedClipAdamW(m, lr=2e-3, weight_decay=0.05, lamb=lamb)
        try:
            want = {"trust_clip": None, "always_adapt": False} if lamb is True else lamb
            assert opt.lamb == want and opt.state_dict()["hparams"]["lamb"] == want
            assert all(v == (0.0, 0.0, 1.0) for v in opt.trust_ratios().values())
            for k in range(2):
                x, y = _batch(k)
                trainer.soft_target_cross_entropy(m(x)[0].squeeze(), y).backward()
                assert any(r["sn"] is not None for r in opt._records)       # deferred layers: their .grad is not the gradient
                recs, grads = _flat_records(opt), [p.grad.detach().clone().reshape(-1) for p in opt.params]
                hp = (2e-3, 0.9, 0.98, 1e-8, 0.05, 1.0, 0)
                ref, bound = lf.reference(recs, grads, hp, None, k, (want["trust_clip"], want["always_adapt"]))
                # (a deferred layer whose gradient cancels to its rounding error has r = +-1 of undecided sign at the first
                # steps: the reference says so with an infinite bound; it must still decide nearly every tensor)
                assert sum(not math.isfinite(e) for e in bound["trust"]) <= len(recs) // 50
                stats = opt.step()
                ratios = opt.trust_ratios()
                assert list(ratios) == [n for n, p in m.named_parameters() if p.requires_grad]
                got = dict(tf.optim_flat(_flat_records(opt)), norm=float(stats[0]), found_inf=float(stats[1]), step=opt.step_count,
                           trust=torch.tensor(list(ratios.values()), dtype=torch.float32))
                worst, _ = lf.check(got, ref, bound)
                print(f"FusedClipAdamW(lamb={lamb}) step {k}: " + " ".join(f"{a}={b:.3f}" for a, b in worst.items()))
                # the independent rule, from the reference's corrected gradient and clip coefficient alone
                o_ref = tf.optim_reference(recs, grads, hp, None, k)[0]
                plain = plain_lamb64(recs, o_ref["gcorr"], tf.f32(2e-3), lambda _: tf.f32(0.05), tf.f32(0.9), tf.f32(0.98),
                                     tf.f32(1e-8), k + 1, o_ref["clip"], want["trust_clip"], want["always_adapt"])
                for t, ((lo, hi), (p64, trust)) in enumerate(zip(ref["spans"], plain)):
                    # two float64 evaluations of the same rule in different orders: equal far inside the fp32 bounds
                    assert float((p64 - ref["p"][lo:hi]).abs().max()) <= 1e-12 + 0.01 * float(bound["p"][lo:hi].min()), t
                    assert abs(trust - ref["trust"][t]) <= 1e-9 * trust
                    assert abs(ratios[list(ratios)[t]][2] - trust) <= bound["trust"][t] + 1e-9 * trust
            assert opt.step_count == 2
        finally:
            opt.close()


def test_constructor_and_state_refusals():
    lin = torch.nn.Linear(4, 4)
    with calm.backend.use_backend(EmulatedBackend()):
        for bad, match in (({"clip": 1.0}, '"trust_clip", "always_adapt"'), ({"trust_clip": 0.0}, "trust_clip"),
                           ({"trust_clip": -2.0}, "trust_clip"), ({"trust_clip": NAN}, "trust_clip"),
                           ({"trust_clip": math.inf}, "trust_clip"), ({"trust_clip": True}, "trust_clip"),
                           ({"always_adapt": 2}, "always_adapt"), ({"always_adapt": "yes"}, "always_adapt"), (0.5, "None, True or a dict")):
            with pytest.raises(ValueError, match=match):
                trainer.FusedClipAdamW(lin, lamb=bad)
        plain, lamb = trainer.FusedClipAdamW(lin), trainer.FusedClipAdamW(lin, lamb=True)
        try:
            assert plain.lamb is None and "lamb" not in plain.state_dict()["hparams"]
            assert trainer.FusedClipAdamW(lin, lamb=False).lamb is None
            with pytest.raises(RuntimeError, match="without lamb="):
                plain.trust_ratios()
            with pytest.raises(ValueError, match="written with LAMB"):
                plain.load_state_dict(lamb.state_dict())
            with pytest.raises(ValueError, match="written without LAMB"):
                lamb.load_state_dict(plain.state_dict())
            lamb.load_state_dict(lamb.state_dict())
            window = trainer.FusedClipAdamWindow(lin, lamb={"trust_clip": 4})
            assert window.lamb == {"trust_clip": 4.0, "always_adapt": False}
        finally:
            plain.close(), lamb.close()


# ---- train(lamb=) ----------------------------------------------------------------------------------------------------------
class HandLambStep(trainer.TrainStep):
    """train()'s step with the optimizer-side half written out: the reducer's exchange, then lamb_step_torch on the
    optimizer's own records, step counter and trust table — nothing of FusedClipAdamW.step / _launch runs."""

    def _optimizer_step(self, m=1):
        opt = self.opt
        grads = opt._contiguous_grads(keep=True)
        group_hp = opt.group_hparams() if len(opt.param_groups) > 1 else None
        lamb_step_torch(opt._records, opt._plan.step_dev, grads, opt._hparams(),
                                (opt.lamb["trust_clip"], opt.lamb["always_adapt"]), group_hp, None, opt.stats, opt._trust_host)
        for p in opt.params:
            p.grad = None


def _train(seed=50, n=8, epochs=2, hand=False, optimizer="fused", **kw):
    torch.manual_seed(seed)
    m = build_model("tiny32_cls", None).train()
    real = trainer._STEP_CLASSES["cls", False]
    if hand:
        trainer._STEP_CLASSES["cls", False] = HandLambStep
    try:
        with calm.backend.use_backend(EmulatedBackend()):
            if callable(optimizer):
                optimizer = optimizer(m)
            return trainer.train(m, optimizer, None, use_gpu=False, dataset=_TinySet(n), epochs=epochs, batch_size=4,
                                 num_classes=10, collate_fn="mix", num_workers=0, log_every=1000, **kw)
    finally:
        trainer._STEP_CLASSES["cls", False] = real


def _same_bits(a, b, what):
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{what}: differs at {k}"


def _differ(a, b):
    return any(not torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))


@pytest.mark.timeout(600)
def test_train_with_lamb_equals_the_hand_written_loop_and_moves_the_run(capsys):
    out = _train(lamb=True)
    assert "LAMB: per-tensor trust ratios on, trust_clip None, always_adapt False" in capsys.readouterr().out
    opt = out._calm_lamb
    assert isinstance(opt, trainer.FusedClipAdamW) and opt.lamb == {"trust_clip": None, "always_adapt": False}
    ratios = opt.trust_ratios()
    assert all(math.isfinite(tr) and tr > 0 for _, _, tr in ratios.values()) and any(tr != 1.0 for _, _, tr in ratios.values())
    _same_bits(out, _train(lamb=True, hand=True), "train(lamb=True) against the hand-written loop")
    plain = _train()
    assert _differ(out, plain) and not hasattr(plain, "_calm_lamb")
    _same_bits(plain, _train(lamb=None), "lamb=None against a run that never mentions the argument")
    # an optimizer object built with lamb=, with and without the matching argument
    built = lambda m: trainer.FusedClipAdamW(m, lamb=True)                         # noqa: E731
    _same_bits(out, _train(optimizer=built), "a FusedClipAdamW built with lamb=")
    _same_bits(out, _train(optimizer=built, lamb=True), "a FusedClipAdamW built with lamb=, and the same argument")
    # parameter groups, a clip, a monitor and an EMA
    kw = dict(lamb={"trust_clip": 1.0}, param_groups="no_decay")
    grouped = _train(monitor={"every": 1, "top": 3}, ema=0.99, **kw)
    _same_bits(grouped, _train(hand=True, **kw), "train(lamb=, param_groups=) against the hand-written loop")
    opt = grouped._calm_lamb
    decays = {n: g["weight_decay"] for g in opt.param_groups for n, p in zip(opt.param_names, opt.params) if any(p is q for q in g["params"])}
    ratios = opt.trust_ratios()
    assert any(wd == 0.0 for wd in decays.values()) and any(wd != 0.0 for wd in decays.values())
    assert all(ratios[n][2] == 1.0 for n, wd in decays.items() if wd == 0.0)       # no decay: plain Adam, exactly
    assert all(ratios[n][2] <= 1.0 for n, wd in decays.items() if wd != 0.0)
    assert any(ratios[n][2] < 1.0 for n, wd in decays.items() if wd != 0.0)
    text = capsys.readouterr().out
    assert "Trust ratio min / median / max:" in text and "LAMB: per-tensor trust ratios on, trust_clip 1.0" in text


@pytest.mark.timeout(600)
def test_monitor_file_carries_the_trust_summary(tmp_path):
    import json
    ck = str(tmp_path / "m.pth")
    out = _train(epochs=1, lamb={"always_adapt": True}, monitor={"every": 1, "top": 2}, checkpoint_path=ck)
    lines = [json.loads(s) for s in open(str(tmp_path / "m_grad.jsonl"))]
    assert len(lines) == 3                                   # two steps and the epoch's end
    ratios = out._calm_lamb.trust_ratios()
    last = lines[-1]
    vals = sorted(v[2] for v in ratios.values())
    assert last["trust"] == {"min": vals[0], "median": vals[len(vals) // 2], "max": vals[-1]}
    assert [e["trust"] for e in last["top_small_trust"]] == vals[:2] and set(last["top_small_trust"][0]) == {
        "name", "trust", "weight_norm", "update_norm"}
    assert "top_update_ratio" in last                        # the AdamW-direction fields keep their place
    plain = _train(epochs=1, monitor={"every": 1, "top": 2}, checkpoint_path=str(tmp_path / "p.pth"))
    assert all("trust" not in json.loads(s) for s in open(str(tmp_path / "p_grad.jsonl"))) and not hasattr(plain, "_calm_lamb")


@pytest.mark.timeout(600)
def test_a_snapshot_at_step_2_resumed_to_step_4_equals_the_uninterrupted_run(tmp_path):
    fa, fb, fc, fd = (str(tmp_path / f"{n}.snap") for n in "abcd")
    a = _train(lamb=True, snapshot_path=fa)
    _train(lamb=True, snapshot_path=fb, max_steps=2)
    head = trainer.TrainState.read_header(fb)[0]["host"]
    assert head["progress"]["step"] == 2 and head["lamb"] == {"trust_clip": None, "always_adapt": False}
    c = _train(seed=51, lamb=True, snapshot_path=fc, resume=fb)
    _same_bits(a, c, "the resumed run")
    with pytest.raises(ValueError, match="written with LAMB"):
        _train(snapshot_path=fc, resume=fb)
    _train(snapshot_path=fd, max_steps=2)
    assert "lamb" not in trainer.TrainState.read_header(fd)[0]["host"]
    with pytest.raises(ValueError, match="written without LAMB"):
        _train(lamb=True, snapshot_path=fc, resume=fd)


@pytest.mark.timeout(600)
def test_train_with_lamb_under_a_window_sam_and_the_generative_task():
    plain = _train(epochs=1, n=16, accumulate=2)
    acc = _train(epochs=1, n=16, accumulate=2, lamb=True)
    assert isinstance(acc._calm_lamb, trainer.FusedClipAdamWindow) and acc._calm_lamb.step_count == 2 and _differ(acc, plain)
    sam = _train(epochs=1, lamb=True, sam=0.05)
    assert isinstance(sam._calm_lamb, trainer.FusedClipAdamWindow) and sam._calm_sam.optimizer is sam._calm_lamb
    assert _differ(sam, _train(epochs=1, sam=0.05))
    for out in (acc, sam):
        assert all(bool(torch.isfinite(p).all()) for p in out.parameters())
        assert any(tr != 1.0 for _, _, tr in out._calm_lamb.trust_ratios().values())
    torch.manual_seed(3)
    m = build_model("nano48_gen", None).train()
    data = torch.utils.data.TensorDataset(torch.randn(8, 3, 48, 48), torch.zeros(8, dtype=torch.long))
    with calm.backend.use_backend(EmulatedBackend()):
        gen = trainer.train(m, "fused", None, use_gpu=False, dataset=data, epochs=1, batch_size=4, num_classes=10, task="reg",
                            num_workers=0, log_every=1000, lamb={"trust_clip": 10.0}, ema=0.9)
    assert gen._calm_lamb.step_count == 2 and all(bool(torch.isfinite(p).all()) for p in gen.parameters())


def test_train_refusals_come_before_any_process_group():
    data = torch.utils.data.TensorDataset(torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,)))
    lin = torch.nn.Linear(4, 4)
    sgd = torch.optim.SGD(lin.parameters(), lr=0.1)
    kw = dict(use_gpu=False, dataset=data, epochs=1, batch_size=2, num_classes=10)
    with pytest.raises(ValueError, match='lamb= needs optimizer="fused"'):
        trainer.train(lin, sgd, lamb=True, **kw)
    with pytest.raises(ValueError, match='"trust_clip", "always_adapt"'):
        trainer.train(lin, "fused", lamb={"clip": 1.0}, **kw)
    for clip in (0.0, -1.0, NAN):
        with pytest.raises(ValueError, match=r'lamb\["trust_clip"\]'):
            trainer.train(lin, "fused", lamb={"trust_clip": clip}, **kw)
    with pytest.raises(ValueError, match="None, True or a dict"):
        trainer.train(lin, "fused", lamb=0.5, **kw)
    with calm.backend.use_backend(EmulatedBackend()):
        plain, lamb = trainer.FusedClipAdamW(lin), trainer.FusedClipAdamW(lin, lamb={"trust_clip": 2.0})
        try:
            with pytest.raises(ValueError, match="contradicts the optimizer"):
                trainer.train(lin, plain, lamb=True, **kw)
            with pytest.raises(ValueError, match="contradicts the optimizer"):
                trainer.train(lin, lamb, lamb=True, **kw)
            with pytest.raises(ValueError, match="contradicts the optimizer"):
                trainer.train(lin, lamb, lamb={"trust_clip": 2.0, "always_adapt": True}, **kw)
        finally:
            plain.close(), lamb.close()
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
    kw = dict(n=16, lamb={"trust_clip": 1.0}, param_groups="no_decay", destroy_process_group=False)
    run = _train(**kw)
    hand = _train(hand=True, **kw)
    torch.save(dict(run=run.state_dict(), hand=hand.state_dict(), trust=run._calm_lamb.trust_ratios()),
               os.path.join(outdir, f"rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_train_with_lamb_on_two_gloo_ranks(tmp_path):
    mp.spawn(_two_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(2))
    for k in r0["run"]:
        assert torch.equal(r0["run"][k], r0["hand"][k]), f"train(lamb=) differs from the hand-written loop at {k}"
        assert torch.equal(r0["run"][k], r1["run"][k]), f"the ranks diverged at {k}"
    assert r0["trust"] == r1["trust"] and any(v[2] != 1.0 for v in r0["trust"].values())
