"""Parameter groups of the fused optimizer without a GPU: the C-ABI addition (calm_optim_group, the group field of
calm_optim_tensor, calm_optim_step_groups's refusals), the per-group float64 checker (tests/optim_groups_f64.py) on the
torch fallback and on planted faults, FusedClipAdamW(groups=) / FusedClipAdamWindow(groups=) against torch AdamW with the
same groups, `param_groups()`, and train(param_groups=, scheduler_step=) on one and two gloo ranks."""
import copy
import ctypes
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
import optim_groups_f64 as gf  # noqa: E402
import tail_f64 as tf  # noqa: E402
from emulated_backend import EmulatedBackend  # noqa: E402
from test_host_logic_cpu import build_model  # noqa: E402
from test_snapshot_cpu import _TinySet, _assert_same_run  # noqa: E402
from importlib import import_module  # noqa: E402

trainer = import_module("calm_vit_dte_amd.trainer")
binding = import_module("calm_vit_dte_amd._lib")
TABLE = tf.optim_table()
GROUPS = gf.table_groups(TABLE)
RULES = [("*ls_*", {"lr_scale": 0.1}), (lambda name, p: p.ndim <= 1, {"weight_decay": 0.0})]     # three groups with the base


def names(failures):
    return {n for n, _ in failures}


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------
def test_group_record_and_group_field_match_the_header():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "calm_vit.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", ' \
          'sizeof(calm_optim_group), offsetof(calm_optim_group, weight_decay), sizeof(calm_optim_tensor), ' \
          'offsetof(calm_optim_tensor, group), offsetof(calm_optim_tensor, chunk0));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    G, T = binding.OptimGroup, binding.OptimTensor
    assert got == [8, 4, 80, 76, 72]
    assert got == [ctypes.sizeof(G), G.weight_decay.offset, ctypes.sizeof(T), T.group.offset, T.chunk0.offset]
    assert np.dtype(G).itemsize == 8 and np.dtype(T).itemsize == 80


_P = 0x7f0000010000          # a fake, 16-byte aligned device address: every call below is refused before any launch


def _hp(beta1=0.9):
    return binding.OptimHparams(1e-3, beta1, 0.999, 1e-8, 0.0, 1.0, 1)


@pytest.mark.parametrize("change,what", [({0: None}, "null tensors_dev"), ({2: None}, "null chunk_tensor_dev"),
                                         ({4: None}, "null scratch"), ({5: None}, "null hparams"),
                                         ({6: None}, "null groups_dev"), ({9: None}, "null stats_out"),
                                         ({7: 0}, "n_groups 0"), ({7: -1}, "n_groups negative"), ({1: 0}, "n_tensors 0"),
                                         ({3: 0}, "n_chunks 0"), ({"beta1": 1.0}, "beta1 1")], ids=lambda v: v if isinstance(v, str) else "")
def test_calm_optim_step_groups_refuses_before_any_launch(change, what):
    lib = binding.load()
    assert "calm_optim_step_groups" in binding.SIGNATURES and lib.calm_abi_version() == binding.ABI_VERSION == 7
    h = _hp(change.pop("beta1", 0.9))
    args = [_P, 3, _P, 5, _P, ctypes.byref(h), _P, 2, None, _P, _P, None]
    for i, v in change.items():
        args[i] = v
    assert lib.calm_optim_step_groups(*args) == binding.E_INVAL, what


# ---- the checker on the torch fallback ------------------------------------------------------------------------------------
def _fallback(recs, grads, sc, group_hp, step):
    """the torch fallback on a copy of the records -> what check_optim reads, and the records after the call"""
    recs = gf.with_groups(copy.deepcopy(recs), GROUPS)
    step_dev, stats = torch.tensor([step], dtype=torch.int32), torch.zeros(2)
    scale = torch.tensor([sc["grad_scale"]]) if sc["grad_scale"] else None
    trainer.optim_step_groups_torch(recs, step_dev, grads, gf.hp_of(sc), group_hp, scale, stats)
    return dict(tf.optim_flat(recs), norm=float(stats[0]), found_inf=float(stats[1]), step=int(step_dev)), recs


@pytest.mark.parametrize("name", gf.SCENARIOS)
def test_torch_fallback_inside_every_bound_of_the_per_group_reference(name):
    """Two consecutive calls; the second reference starts from the state the first call left.  Then the planted faults."""
    sc = gf.scenario(name)
    recs, step = tf.optim_state(TABLE), sc["t_prev"]
    assert {g for g in GROUPS} == {0, 1, 2} and len(gf.GROUP_HP) == 4          # the fourth group is empty
    for call in (1, 2):
        grads = tf.optim_grads(TABLE, recs, seed=call, scale=sc["grad_scale"] or 1.0)
        ref, bound = gf.grouped_reference(recs, grads, sc, gf.GROUP_HP, GROUPS, step)
        got, after = _fallback(recs, grads, sc, gf.GROUP_HP, step)
        worst, _ = tf.check_optim(got, ref, bound)                             # strict
        print(f"grouped optim {name} call {call}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
        if call == 1:
            frozen = gf.element_groups(recs, GROUPS) == 2                      # lr = 0: the bits stay, the moments move
            before = tf.optim_flat(recs)
            assert torch.equal(got["p"][frozen].view(torch.int32), before["p"][frozen].view(torch.int32))
            assert not torch.equal(got["m"][frozen], before["m"][frozen])
            # planted: group 0's weight decay for every tensor; the rates of groups 0 and 1 exchanged
            (lr0, wd0), (lr1, wd1) = gf.GROUP_HP[:2]
            one_wd = [(lr, wd0) for lr, _ in gf.GROUP_HP]
            swapped = [(lr1, wd0), (lr0, wd1)] + gf.GROUP_HP[2:]
            for fault in (one_wd, swapped):
                _, failures = tf.check_optim(_fallback(recs, grads, sc, fault, step)[0], ref, bound, strict=False)
                assert "p" in names(failures), failures
        recs = [{k: v for k, v in r.items() if k != "group"} for r in after]
        step = got["step"]
    assert step == sc["t_prev"] + 2


def test_assignment_reaches_what_it_claims():
    by = {(e["kind"], e["numel"]): g for e, g in zip(TABLE, GROUPS)}
    assert by[("plain", 3 * tf.OPT_CHUNK + 5)] == 1 and by[("sn", 144 * 288)] == 1
    assert by[("sn", 300 * 260)] == 2 and by[("cancel", 64 * 48)] == 2
    assert [GROUPS.count(g) > 50 for g in range(3)] == [True] * 3 and 3 not in GROUPS


# ---- the optimizer classes on tiny32_cls ------------------------------------------------------------------------------------
def _batch(seed=0, B=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 32, 32, generator=g), torch.softmax(torch.randn(B, 10, generator=g), 1)


def _pair(seed):
    torch.manual_seed(seed)
    m_ref = build_model("tiny32_cls", None).train()
    m = build_model("tiny32_cls", None).train()
    m.load_state_dict(m_ref.state_dict())
    return m_ref, m


def _worst(m, m_ref):
    sd, sd_ref = m.state_dict(), m_ref.state_dict()
    return max(float((sd[k] - sd_ref[k]).abs().max()) for k in sd)


def test_grouped_fused_optimizer_steps_like_torch_adamw_with_the_same_groups_under_a_schedule():
    """The "no_decay" preset plus a reduced rate on the layer scales: three groups, CosineAnnealingLR stepping between
    four steps, against make_optimizer(groups=) + clip_grad_norm_ on a model whose backward corrects the spectral-norm
    gradients itself (the construction and the bar of test_second_optimizer_takes_the_deferral_over_and_steps_like_torch)."""
    with calm.backend.use_backend(EmulatedBackend()):
        m_ref, m = _pair(2)
        opt_ref = trainer.make_optimizer(m_ref, groups=trainer.param_groups(m_ref, RULES)[0])
        opt = trainer.FusedClipAdamW(m, groups=trainer.param_groups(m, RULES)[0])
        assert len(opt.param_groups) == len(opt_ref.param_groups) == 3 and opt.grouped
        assert [len(g["params"]) for g in opt.param_groups] == [len(g["params"]) for g in opt_ref.param_groups]
        assert [id(p) for p in opt.params] == [id(p) for p in m.parameters() if p.requires_grad]     # model order
        s_ref = torch.optim.lr_scheduler.CosineAnnealingLR(opt_ref, T_max=5, eta_min=1e-6)
        s = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=5, eta_min=1e-6)
        step_ref, step = trainer.TrainStep(m_ref, opt_ref), trainer.TrainStep(m, opt)
        try:
            for k in range(4):
                l_ref, _ = step_ref(*_batch(k))
                l, _ = step(*_batch(k))
                assert abs(float(l) - float(l_ref)) < 1e-5
                s_ref.step()
                s.step()
                assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in opt_ref.param_groups]
            assert opt.param_groups[1]["lr"] != opt.param_groups[0]["lr"] == opt.lr
            assert _worst(m, m_ref) < 2e-5, _worst(m, m_ref)
            hp = opt.state_dict()["hparams"]
            assert hp["groups"] == [[g["lr"], g["weight_decay"]] for g in opt.param_groups]
            assert [wd for _, wd in hp["groups"]] == [0.02, 0.02, 0.0]
        finally:
            opt.close()


def test_state_dict_round_trip_restores_every_group_and_refuses_another_count():
    with calm.backend.use_backend(EmulatedBackend()):
        _, m = _pair(3)
        opt = trainer.FusedClipAdamW(m, groups=trainer.param_groups(m, RULES)[0])
        plain = trainer.FusedClipAdamW(m)
        try:
            assert "groups" not in plain.state_dict()["hparams"] and len(plain.param_groups) == 1
            sd = copy.deepcopy(opt.state_dict())
            sd["hparams"]["groups"] = [[1e-4, 0.5], [2e-4, 0.25], [3e-4, 0.0]]
            opt.load_state_dict(sd)
            assert opt.group_hparams() == [(1e-4, 0.5), (2e-4, 0.25), (3e-4, 0.0)]
            with pytest.raises(ValueError, match="parameter group"):
                plain.load_state_dict(sd)
            with pytest.raises(ValueError, match="parameter group"):
                opt.load_state_dict(plain.state_dict())
        finally:
            plain.close()
            opt.close()


def test_group_refusals():
    with calm.backend.use_backend(EmulatedBackend()):
        m = build_model("tiny32_cls", None).train()
        other = torch.nn.Parameter(torch.zeros(3))
        ps = list(m.parameters())
        bad = [([{"params": ps[:1], "betas": (0.9, 0.9)}], "betas"), ([{"params": ps[:1], "eps": 1e-6}], "eps"),
               ([{"params": ps[:2]}, {"params": ps[1:3]}], "another group"), ([{"params": [ps[0], ps[0]]}], "another group"),
               ([{"params": [other]}], "not a parameter of the model"), ([{"params": ps[:1], "lr": -1e-3}], "negative")]
        for groups, match in bad:
            with pytest.raises(ValueError, match=match):
                trainer.FusedClipAdamW(m, groups=groups)
            with pytest.raises(ValueError, match=match):
                trainer.make_optimizer(m, groups=groups)
        ps[0].requires_grad_(False)
        with pytest.raises(ValueError, match="requires_grad=False"):
            trainer.FusedClipAdamW(m, groups=[{"params": ps[:1]}])
        ps[0].requires_grad_(True)
        # nothing above left a deferral mark behind; an empty base group is fine
        opt = trainer.FusedClipAdamW(m, groups=[{"params": ps, "lr": 1e-3}])
        assert len(opt.param_groups) == 2 and opt.param_groups[0]["params"] == [] and opt.lr == 3.1e-3
        opt.close()


def test_param_groups_rules():
    m = build_model("tiny32_cls", None).train()
    named = dict(m.named_parameters())
    small = [n for n, p in named.items() if p.ndim <= 1]
    # the preset: every tensor with ndim <= 1 and nothing else
    groups, frozen = trainer.param_groups(m, "no_decay")
    assert frozen == [] and len(groups) == 1 and groups[0]["weight_decay"] == 0.0 and groups[0]["lr"] == 3.1e-3
    assert groups[0]["names"] == small and [id(p) for p in groups[0]["params"]] == [id(named[n]) for n in small]
    assert any(n.endswith("inv_freq") for n in small) and any("ls_att" in n for n in small) and any(n.endswith(".bias") for n in small)
    assert not any(n.endswith("weight_orig") for n in small) and any(n.endswith("weight_orig") for n in named)
    # the first match wins: the layer scales take rule 0 although rule 1 matches them too
    groups, _ = trainer.param_groups(m, RULES)
    assert [(g["lr"], g["weight_decay"]) for g in groups] == [(3.1e-3 * 0.1, 0.02), (3.1e-3, 0.0)]
    assert all("ls_" in n for n in groups[0]["names"]) and not any("ls_" in n for n in groups[1]["names"])
    assert sorted(groups[0]["names"] + groups[1]["names"]) == sorted(small)
    # rules that end at the same pair share a group; a pair equal to the base one stays in the base group
    same, _ = trainer.param_groups(m, [("*ls_att", {"lr": 1e-4, "weight_decay": 0.0}), ("*ls_mlp", {"lr": 1e-4, "weight_decay": 0.0})])
    assert len(same) == 1 and any("ls_att" in n for n in same[0]["names"]) and any("ls_mlp" in n for n in same[0]["names"])
    # frozen parameters are handed back, in no group
    groups, frozen = trainer.param_groups(m, [("*inv_freq", {"frozen": True}), ("*ls_*", {"lr_scale": 0.5})])
    assert {id(p) for p in frozen} == {id(p) for n, p in named.items() if n.endswith("inv_freq")} and len(groups) == 1
    with pytest.raises(ValueError, match="matches no parameter"):
        trainer.param_groups(m, [("*ls_*", {"lr_scale": 0.1}), ("*no_such_layer*", {"weight_decay": 0.0})])
    with pytest.raises(ValueError, match="lr_scale"):
        trainer.param_groups(m, [("*ls_*", {"lr_scale": 0.1, "lr": 1e-3})])
    with pytest.raises(ValueError, match="takes"):
        trainer.param_groups(m, [("*ls_*", {"momentum": 0.1})])
    with pytest.raises(ValueError, match="preset"):
        trainer.param_groups(m, "decay_nothing")


def test_grouped_window_of_two_equals_the_torch_loop():
    """FusedClipAdamWindow(groups=), window of 2, against "2 x (forward, backward), mean, clip, grouped AdamW"."""
    with calm.backend.use_backend(EmulatedBackend()):
        m_ref, m = _pair(5)
        opt_ref = trainer.make_optimizer(m_ref, groups=trainer.param_groups(m_ref, RULES)[0])
        params = [p for p in m_ref.parameters() if p.requires_grad]
        opt = trainer.FusedClipAdamWindow(m, groups=trainer.param_groups(m, RULES)[0])
        step = trainer.AccumTrainStep(m, opt, accumulate=2)
        try:
            for w in range(2):
                for k in range(2):
                    x, y = _batch(2 * w + k)
                    torch.nn.functional.cross_entropy(m_ref(x)[0].squeeze(), y).backward()      # autograd sums into .grad
                    step(x, y)
                    assert step.boundary == (k == 1)
                torch._foreach_mul_([p.grad for p in params], 0.5)
                torch.nn.utils.clip_grad_norm_(params, max_norm=1.0)
                opt_ref.step()
                opt_ref.zero_grad()
            assert opt.step_count == 2 and [r["group"] for r in opt._acc_records] == [r["group"] for r in opt._records]
            assert _worst(m, m_ref) < 2e-5, _worst(m, m_ref)
        finally:
            opt.close()


# ---- train() ------------------------------------------------------------------------------------------------------------------
FROZEN_RULES = [("*inv_freq", {"frozen": True})] + RULES


def _train(seed=50, n=8, epochs=2, **kw):
    """train("fused") on the CPU model: `epochs` epochs of n / 4 batches (per rank), SoftMixCollate in the main process"""
    torch.manual_seed(seed)
    m = build_model("tiny32_cls", None).train()
    with calm.backend.use_backend(EmulatedBackend()):
        return trainer.train(m, "fused", None, use_gpu=False, dataset=_TinySet(n), epochs=epochs, batch_size=4,
                             num_classes=10, collate_fn="mix", num_workers=0, log_every=1000, **kw)


def _hand_loop(rules, seed=50, n=8, epochs=2, rank=0, world=1):
    """What train(param_groups=rules) means, written out by hand: the groups read off named_parameters() with plain string
    tests (not through trainer.param_groups / make_optimizer(groups=)) into torch's AdamW, the sampler, the collate, the
    per-epoch cosine schedule, and TrainStep's backward / exchange / clip / step."""
    from torch.utils.data import DataLoader, DistributedSampler
    torch.manual_seed(seed)
    m = build_model("tiny32_cls", None).train()
    with calm.backend.use_backend(EmulatedBackend()):
        base, scales, no_decay = [], [], []
        for name, p in m.named_parameters():
            if rules is FROZEN_RULES and name.endswith("inv_freq"):
                p.requires_grad_(False)                   # frozen: in no group
            elif rules is FROZEN_RULES and "ls_" in name:
                scales.append(p)                          # a tenth of the rate, the base decay
            elif p.ndim <= 1:
                no_decay.append(p)
            else:
                base.append(p)
        assert rules is FROZEN_RULES or rules == "no_decay"
        hand = [{"params": base}] + ([{"params": scales, "lr": 3.1e-3 * 0.1}] if scales else []) + \
            [{"params": no_decay, "weight_decay": 0.0}]
        opt = torch.optim.AdamW(hand, lr=3.1e-3, weight_decay=0.02, betas=(0.9, 0.98))
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs, eta_min=1e-6)
        trainer.sync_module_states(m)
        reducer = trainer.BucketedGradReducer(m) if world > 1 else None
        data = _TinySet(n)
        sampler = DistributedSampler(data, num_replicas=world, rank=rank, shuffle=True, seed=2006)
        loader = DataLoader(data, batch_size=4, sampler=sampler, collate_fn=trainer.SoftMixCollate(num_classes=10, seed=2006 + rank))
        step = trainer.TrainStep(m, opt, reducer)
        for epoch in range(epochs):
            sampler.set_epoch(epoch)
            for x, y in loader:
                step(x, y)
            sched.step()
    return m


def _check_frozen(out, seed=50):
    torch.manual_seed(seed)
    first = build_model("tiny32_cls", None).state_dict()
    sd = out.state_dict()
    frozen = [k for k in sd if k.endswith("inv_freq")]
    assert frozen and all(torch.equal(sd[k].view(torch.int32), first[k].view(torch.int32)) for k in frozen)
    for n, p in out.named_parameters():
        if n.endswith("inv_freq"):
            assert p.grad is None and not p.requires_grad
    assert any(not torch.equal(sd[k], first[k]) for k in sd if k.endswith("weight_orig"))


@pytest.mark.timeout(600)
def test_train_with_the_no_decay_preset_and_with_a_frozen_rule_equals_the_hand_written_loop(capsys):
    out = _train(param_groups="no_decay")
    printed = capsys.readouterr().out
    assert printed.count("Parameter group") == 2 and "weight decay 0.0" in printed
    assert _worst(out, _hand_loop("no_decay")) < 2e-5
    out = _train(param_groups=FROZEN_RULES)
    _check_frozen(out)
    assert _worst(out, _hand_loop(FROZEN_RULES)) < 2e-5


@pytest.mark.timeout(600)
def test_per_step_schedule_moves_once_per_optimizer_step_also_behind_the_flushed_window(monkeypatch):
    """20 samples, batches of 4, windows of 2: optimizer steps behind batches 2, 4 and the flushed 5 of both epochs.  Every
    step must use the rate CosineAnnealingLR(T_max = 2 * 3) holds after as many scheduler steps as optimizer steps taken."""
    used, real = [], trainer.optim_step_groups_torch

    def spy(records, step_dev, grads, hp, group_hp, *a):
        used.append([lr for lr, _ in group_hp])
        return real(records, step_dev, grads, hp, group_hp, *a)

    monkeypatch.setattr(trainer, "optim_step_groups_torch", spy)
    _train(n=20, accumulate=2, param_groups=RULES, scheduler_step="step")
    ref = torch.optim.AdamW([{"params": [torch.nn.Parameter(torch.zeros(1))], "lr": lr} for lr in (3.1e-3, 3.1e-4, 3.1e-3)])
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(ref, T_max=6, eta_min=1e-6)
    want = []
    for _ in range(6):
        want.append([g["lr"] for g in ref.param_groups])
        ref.step()
        sched.step()
    assert len(used) == 6 and used == want
    assert want[0] == [3.1e-3, 3.1e-3 * 0.1, 3.1e-3] and want[5][0] < want[1][0]


@pytest.mark.timeout(600)
def test_snapshot_with_three_groups_and_a_per_step_schedule_resumes_exactly_and_is_refused_by_one_group(tmp_path):
    fa, fb, fc = (str(tmp_path / f"{n}.snap") for n in "abc")
    kw = dict(param_groups=RULES, scheduler_step="step")
    a = _train(snapshot_path=fa, **kw)
    _train(snapshot_path=fb, snapshot_every=3, max_steps=3, **kw)
    host = trainer.TrainState.read_header(fb)[0]["host"]
    assert host["progress"] == {"epoch": 1, "batch": 1, "step": 3}
    assert len(host["lrs"]) == 3 and host["lrs"][0] == host["lr"] and host["scheduler"]["last_epoch"] == 3
    c = _train(seed=51, snapshot_path=fc, resume=fb, **kw)
    _assert_same_run(a, c, fa, fc)
    with pytest.raises(ValueError, match="parameter group"):
        _train(seed=51, resume=fb)                                  # one group
    # a one-group file is what it was: no new key
    fd = str(tmp_path / "d.snap")
    _train(snapshot_path=fd, epochs=1)
    assert "lrs" not in trainer.TrainState.read_header(fd)[0]["host"]
    with pytest.raises(ValueError, match="parameter group"):
        _train(seed=51, resume=fd, **kw)


@pytest.mark.timeout(600)
def test_torch_optimizer_with_several_groups_keeps_its_snapshot_format(tmp_path):
    """A torch optimizer's groups travel in its own state dict: no "lrs" key, and a file without one resumes."""
    path = str(tmp_path / "t.snap")

    def run(**kw):
        torch.manual_seed(50)
        m = build_model("tiny32_cls", None).train()
        with calm.backend.use_backend(EmulatedBackend()):
            opt = trainer.make_optimizer(m, groups=trainer.param_groups(m, RULES)[0])
            trainer.train(m, opt, None, use_gpu=False, dataset=_TinySet(8), epochs=1, batch_size=4, num_classes=10,
                          collate_fn="mix", num_workers=0, log_every=1000, **kw)
        return opt

    assert len(run(snapshot_path=path, max_steps=1).param_groups) == 3
    host = trainer.TrainState.read_header(path)[0]["host"]
    assert "lrs" not in host and len(host["optimizer"]["param_groups"]) == 3 and host["progress"]["step"] == 1
    run(resume=path)


def test_argument_refusals_come_before_any_process_group():
    data = torch.utils.data.TensorDataset(torch.randn(4, 3, 32, 32), torch.randint(0, 10, (4,)))
    lin = torch.nn.Linear(4, 4)
    sgd = torch.optim.SGD(lin.parameters(), lr=0.1)
    with pytest.raises(ValueError, match="build the groups into the optimizer you hand in"):
        trainer.train(lin, sgd, use_gpu=False, dataset=data, epochs=1, batch_size=2, num_classes=10, param_groups="no_decay")
    with pytest.raises(ValueError, match="scheduler_step"):
        trainer.train(lin, sgd, use_gpu=False, dataset=data, epochs=1, batch_size=2, num_classes=10, scheduler_step="batch")
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
    out = _train(n=16, param_groups=FROZEN_RULES, destroy_process_group=False)
    _check_frozen(out)
    ref = _hand_loop(FROZEN_RULES, n=16, rank=rank, world=world)
    torch.save({"train": out.state_dict(), "loop": ref.state_dict()}, os.path.join(outdir, f"rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_train_with_groups_and_a_frozen_rule_on_two_gloo_ranks(tmp_path):
    mp.spawn(_two_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(2))
    for k in r0["train"]:
        assert torch.equal(r0["train"][k], r1["train"][k]), f"ranks diverged at {k}"
    worst = max(float((r0["train"][k] - r0["loop"][k]).abs().max()) for k in r0["train"])
    assert worst < 2e-5, worst
