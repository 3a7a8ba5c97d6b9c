"""The k-NN probe's kernels on the MI355X: the checker of tests/knn_f64.py on HipBackend — every exact case, hand-built row and
realistic case, fp32 and bf16 into calm_knn_normalize, aligned and unaligned strides and bases, with guard elements around
every output —, two identical runs bit for bit, KnnProbe on CUDA against the emulation, and knn_evaluate(lean=True, graph=True)
on the nano-48 generative model with golden weights against tests/eval_f64.py and float64 similarities."""
from importlib import import_module

import numpy as np
import pytest
import torch

import calm_vit_dte_amd as calm
import emulated_knn as E
import eval_f64
import knn_f64 as F
import weights as W
from helpers import load_golden
from test_host_logic_cpu import build_model

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")


@pytest.fixture(autouse=True)
def _restore():
    yield
    calm.backend.set_loss_kernels(False)


def _strided(t, pad, lead, fill, tail=8):
    """`t` [R, C] on the device with row stride C + pad, its base `lead` elements behind a 16-byte boundary; the padding, the
    lead and `tail` guard elements hold `fill`.  Returns (buffer, view)."""
    R, Cn = t.shape
    ld = Cn + pad
    buf = torch.full((lead + R * ld + tail,), fill, dtype=t.dtype, device="cuda")
    view = torch.as_strided(buf, (R, Cn), (ld, 1), lead)
    view.copy_(t)
    assert view.data_ptr() % 16 == (t.element_size() * lead) % 16
    return buf, view


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 16,), fill, dtype=dtype, device="cuda")
    return buf, buf[:n].view(shape)


class HipImpl:
    """The kernels behind the checker's interface; every call also checks that nothing was written outside its output."""

    def __init__(self):
        self.be = calm.backend.get_backend()

    def normalize(self, x, pad, lead):
        N, D = x.shape
        _, xs = _strided(x, pad, lead, float("nan"))
        buf, out = _guarded((N, D), torch.float32, 7.0)
        bad = torch.tensor([100, 9], dtype=torch.int64, device="cuda")
        self.be.knn_normalize(xs, out, bad[:1], N, D)
        assert bool((buf[N * D:] == 7.0).all()) and int(bad[1]) == 9
        return out.cpu(), int(bad[0]) - 100

    def similarities(self, q, rows):
        q, rows = q.cuda().contiguous(), rows.cuda().contiguous()
        (Nq, D), n = q.shape, rows.shape[0]
        out = torch.empty(Nq, n, device="cuda")
        with calm.backend.fp32_matmul():
            self.be.gemm(q, rows, out, Nq, n, D, (D, 1, 0, 0), (D, 1, 0, 0), (n, 0, 0))
        return out.cpu()

    def merge(self, sims, base, best_sim, best_idx, pad, lead):
        Nq, n = sims.shape
        k = best_sim.shape[1]
        _, s = _strided(sims, pad, lead, 3.0e38)                      # (a pad element read as data would win every compare)
        sbuf, bs = _guarded((Nq, k), torch.float32, 7.0)
        ibuf, bi = _guarded((Nq, k), torch.int64, 7)
        bs.copy_(best_sim)
        bi.copy_(best_idx)
        self.be.knn_merge(s, base, bs, bi, Nq, n, k)
        assert bool((sbuf[Nq * k:] == 7.0).all()) and bool((ibuf[Nq * k:] == 7).all())
        return bs.cpu(), bi.cpu()

    def vote(self, best_sim, best_idx, labels, inv_T, C):
        Nq, k = best_sim.shape
        buf = torch.full((Nq * (C + 3) + 16,), 7.0, device="cuda")
        scores = torch.as_strided(buf, (Nq, C), (C + 3, 1), 0)        # a row stride that is not C
        self.be.knn_vote(best_sim.cuda(), best_idx.cuda(), labels.cuda(), inv_T, scores, Nq, k, C)
        assert bool((torch.as_strided(buf, (Nq, 3), (C + 3, 1), C) == 7.0).all()) and bool((buf[Nq * (C + 3):] == 7.0).all())
        return scores.cpu()


@pytest.mark.parametrize("case", F.EXACT_CASES, ids=lambda c: "Nq{}_Nb{}_D{}_k{}_chunk{}".format(*c))
def test_exact_cases_are_bit_exact_under_every_chunking(case):
    assert F.check_exact(HipImpl(), [case]) == []


def test_hand_built_rows():
    assert F.check_rows(HipImpl()) == []


def test_realistic_cases_within_the_derived_bound():
    assert F.check_realistic(HipImpl()) == []


def test_normalize_fp32_and_bf16_aligned_and_unaligned():
    assert F.check_normalize(HipImpl()) == []


def test_vote_against_float64_on_its_own_state():
    assert F.check_vote(HipImpl()) == []


def test_two_identical_runs_are_bit_equal():
    impl = HipImpl()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(300, 144, generator=g)
    sims = [torch.randint(-40, 41, (64, 6000), generator=g).float() / 32 for _ in range(3)]
    labels = torch.arange(18000) % 10
    runs = []
    for _ in range(2):
        xn = impl.normalize(x, 0, 0)[0]
        state = F.run_chunks(impl, [(6000 * i, s) for i, s in enumerate(sims)], 64, 50)
        runs.append((xn, state[0], state[1], impl.vote(state[0], state[1], labels, 1.0 / 0.07, 10)))
    for a, b in zip(*runs):
        assert torch.equal(a, b) if a.dtype == torch.int64 else torch.equal(F.bits(a), F.bits(b))


def _unit_grid(Nq, Nb, D, seed=0):
    """Rows of +-1 / sqrt(D), D a power of four: the squared norm is exactly 1, so the normalisation changes no bit and
    every similarity is an exact multiple of 1 / D with many ties."""
    g = torch.Generator().manual_seed(31 * Nb + D + seed)
    a = 1.0 / float(np.sqrt(D))
    q = (torch.randint(0, 2, (Nq, D), generator=g).float() * 2 - 1) * a
    bank = (torch.randint(0, 2, (Nb, D), generator=g).float() * 2 - 1) * a
    return q, bank


@pytest.mark.parametrize("case", [(1, 1, 1, 1, 1), (3, 5, 16, 8, 2), (2, 64, 16, 1, 64), (5, 257, 64, 20, 64), (4, 1000, 64, 200, 333),
                                  (2, 4099, 256, 256, 4099), (1, 16387, 64, 20, 16384)],
                         ids=lambda c: "Nq{}_Nb{}_D{}_k{}_chunk{}".format(*c))
def test_probe_on_cuda_equals_the_emulation(case):
    """The exact cases' shapes with D moved to a power of four and entries +-1 / sqrt(D): KnnProbe normalises what it is
    given, and only unit rows come through calm_knn_normalize bit for bit, which the exact comparison needs."""
    Nq, Nb, D, k, chunk = case
    q, bank = _unit_grid(Nq, Nb, D)
    C = 7
    bl, ql = torch.arange(Nb) % C, torch.arange(Nq) % C
    got = trainer.KnnProbe(C, k=k, chunk=chunk, confusion=True, device="cuda")
    got.add_bank(bank.cuda(), bl.cuda())
    gs, gi = got.neighbours(q.cuda())
    got.query(q.cuda(), ql.cuda())
    with calm.backend.use_backend(E.EmulatedKnnBackend()):
        want = trainer.KnnProbe(C, k=k, chunk=max(1, chunk // 2 + 1), confusion=True)
        want.add_bank(bank, bl)
        ws, wi = want.neighbours(q)
        want.query(q, ql)
        rw = want.read()
    rg = got.read()
    assert torch.equal(gi.cpu(), wi) and torch.equal(F.bits(gs.cpu()), F.bits(ws))
    assert F.state_diff((gs.cpu(), gi.cpu()), F.ref_topk((q.double() @ bank.double().T).float().numpy(), np.arange(Nb), k), "probe") == []
    assert set(rg) == set(rw)
    for key in rg:
        if isinstance(rg[key], torch.Tensor):
            assert torch.equal(rg[key].cpu().double().nan_to_num(nan=-1.0), rw[key].double().nan_to_num(nan=-1.0)), key
        else:
            assert rg[key] == rw[key], key


def test_knn_evaluate_lean_graph_on_the_generative_model(monkeypatch):
    name, D, k = "nano48_gen", 144, 5
    m = build_model(name, load_golden(name), "cuda").train()
    bank_x = torch.from_numpy(W.make_input((40, 3, 48, 48), 11)).cuda()
    query_x = torch.from_numpy(W.make_input((10, 3, 48, 48), 12)).cuda()
    bank_y, query_y = torch.arange(40, device="cuda") % 4, torch.arange(10, device="cuda") % 4
    seen = {"bank": [], "query": [], "scores": [], "state": []}
    add_bank, query, neighbours = trainer.KnnProbe.add_bank, trainer.KnnProbe.query, trainer.KnnProbe._neighbours
    replays = []
    replay = torch.cuda.CUDAGraph.replay

    def spy_bank(self, f, y):
        seen["bank"].append(f.float().cpu())
        return add_bank(self, f, y)

    def spy_query(self, f, y):
        seen["query"].append(f.float().cpu())
        seen["scores"].append(query(self, f, y).cpu())

    def spy_neighbours(self, q):
        out = neighbours(self, q)
        seen["state"].append((out[0].cpu(), out[1].cpu()))
        return out

    def spy_replay(self):
        replays.append(1)
        return replay(self)
    monkeypatch.setattr(trainer.KnnProbe, "add_bank", spy_bank)
    monkeypatch.setattr(trainer.KnnProbe, "query", spy_query)
    monkeypatch.setattr(trainer.KnnProbe, "_neighbours", spy_neighbours)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", spy_replay)
    batches = lambda x, y: [(x[i:i + 16], y[i:i + 16]) for i in range(0, len(x), 16)]
    rep = trainer.knn_evaluate(m, batches(bank_x, bank_y), batches(query_x, query_y), 4, k=k, topk=(1, 2), lean=True, graph=True,
                               confusion=True)
    assert m.training and len(replays) == 2                        # bank batches of 16, 16 (replayed) and 8, queries 10 (eager)
    scores, feats, q = torch.cat(seen["scores"]), torch.cat(seen["bank"]), torch.cat(seen["query"])
    ref = eval_f64.reference(scores, query_y.cpu(), (1, 2))
    assert rep["n"] == 10 and rep["bank"] == 40 and rep["bank_zeroed"] == 0 and rep["query_zeroed"] == 0
    assert rep["top1"] == int(ref["counts"][3]) / 10 and rep["top2"] == int(ref["counts"][4]) / 10
    assert torch.equal(rep["confusion"], torch.from_numpy(ref["confusion"]))
    s64 = (F.unit64(q) @ F.unit64(feats).T).numpy()
    gs, gi = torch.cat([s for s, _ in seen["state"]]), torch.cat([i for _, i in seen["state"]])
    bad, worst = F.tolerant_diff(gs, gi, s64, k, D * 2.0 ** -23, "knn_evaluate")
    print(f"knn_evaluate: worst |sim - float64| / eps = {worst:.4f}")
    assert bad == []
