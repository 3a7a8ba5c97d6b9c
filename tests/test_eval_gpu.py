"""calm_eval_metrics on the MI355X, through the C-ABI (HipBackend) and trainer.EvalMetrics / evaluate(report=True): every
integer against the float64 checker (tests/eval_f64.py) — exactly — on fp32 and bf16 logits with an aligned row stride
(16-byte loads) and one with ld % 4 == 1 (element loads), the loss sum against float64, calm_top1_count's total, split
updates, bit-reproducibility, a captured update and the evaluation loop of the nano48 model.

The loss bound is not a constant: `soft_ce_error` measures calm_soft_ce_fwd against float64 on the same rows with one-hot
targets — the counted rows of every case below that hold no NaN and no infinity, as fp32: with a -inf logit the soft-target
formula multiplies a zero target by an infinity and is NaN, in torch as in the kernel — and the new loss sum, over all
finite rows, may be off by twice the largest of those errors: per row the two kernels compute the same (max - z_l) +
log(sum exp(z - max)), only the order of the sums differs, and a -inf entry adds an exact zero to the sum.  The largest
error over all cases is the bound for every case: on a case of one to five rows either kernel lands on the float64 value
or one ulp beside it by chance, which says nothing about the other.
Measured on MI355X: see DESIGN.md, "Validation metrics"."""
from importlib import import_module

import pytest
import torch

import calm_vit_dte_amd as calm
import eval_f64 as F
import weights as W
from helpers import CONFIGS, load_golden
from test_eval_cpu import LOSS_TOL
from test_host_logic_cpu import build_model

pytestmark = pytest.mark.gpu
trainer = import_module("calm_vit_dte_amd.trainer")
KS = (1, 5)
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(autouse=True)
def _restore_switch():
    prev = calm.backend.get_loss_kernels()
    yield
    calm.backend.set_loss_kernels(prev)


def _with_stride(z, aligned):
    """The values of z on the device in rows of stride ld: the next multiple of 8 (16-byte loads in both storage types),
    or the next ld >= C with ld % 4 == 1 (element loads)."""
    B, C = z.shape
    ld = (C + 7) // 8 * 8 if aligned else C + (1 - C) % 4
    buf = torch.zeros(B, ld, dtype=z.dtype, device="cuda")
    buf[:, :C] = z
    view = buf[:, :C]
    assert view.stride() == (ld, 1) and (ld % 8 == 0 if aligned else ld % 4 == 1)
    return view


def _kernel(z, labels, ks=KS, confusion=True):
    be = calm.backend.get_backend()
    B, C = z.shape
    counts = torch.zeros(7 + 2 * C, dtype=torch.int64, device="cuda")
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    conf = torch.zeros(C, C, dtype=torch.int64, device="cuda") if confusion else None
    be.eval_metrics(z, labels.cuda(), ks, counts, loss, conf, B, C)
    return counts, float(loss), conf


@pytest.fixture(scope="module")
def soft_ce_error():
    """Largest relative error of calm_soft_ce_fwd's loss against float64 over the finite rows of every case (one-hot
    targets): what the new loss sum is measured against."""
    be = calm.backend.get_backend()
    worst = 0.0
    for B, C in F.SHAPES:
        for dtype in DTYPES:
            z, labels = F.make_case(B, C, dtype, inf_row=False)
            keep = (labels >= 0) & (labels < C) & torch.isfinite(z.float()).all(dim=1)
            zf, lf = z.float()[keep].contiguous().cuda(), labels[keep]
            n = zf.shape[0]
            assert n > 0
            y = torch.zeros(n, C)
            y[torch.arange(n), lf] = 1.0
            row_stats, loss = torch.empty(n, 2, device="cuda"), torch.zeros((), device="cuda")
            be.soft_ce_fwd(zf, y.cuda(), row_stats, loss, None, n, C)
            err = F.loss_error(float(loss) * n, F.reference(z[keep], lf, KS)["loss_sum"])
            print(f"\ncalm_soft_ce_fwd {B}x{C} {dtype}: rel err {err:.3e}")
            worst = max(worst, err)
    print(f"\ncalm_soft_ce_fwd: largest rel err against float64 {worst:.3e}")
    assert 0.0 < worst < float("inf")
    return worst


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C", F.SHAPES)
def test_kernel_against_the_float64_checker(B, C, dtype, aligned, soft_ce_error):
    for inf_row in (True, False):
        z, labels = F.make_case(B, C, dtype, inf_row=inf_row)
        ref = F.reference(z, labels, KS)
        counts, loss, conf = _kernel(_with_stride(z.cuda(), aligned), labels)
        assert F.mismatches(counts, conf, ref, len(KS)) == []
        err = F.loss_error(loss, ref["loss_sum"])
        print(f"\ncalm_eval_metrics {B}x{C} {dtype} aligned={aligned} inf_row={inf_row}: loss sum {loss!r} vs "
              f"{ref['loss_sum']!r}, rel err {err:.3e} (bound {2 * soft_ce_error:.3e})")
        assert err <= 2 * soft_ce_error
    counts2, loss2, _ = _kernel(_with_stride(z.cuda(), aligned), labels, ks=(2, 1, 7, 3), confusion=False)
    assert F.mismatches(counts2, None, F.reference(z, labels, (2, 1, 7, 3)), 4) == [] and loss2 == loss


@pytest.mark.parametrize("B,C", F.SHAPES)
def test_top1_total_equals_calm_top1_count(B, C):
    z, labels = F.make_case(B, C)
    counts, _, _ = _kernel(z.cuda(), labels, ks=(1,), confusion=False)
    m = trainer.StepMetrics(torch.device("cuda"))
    calm.backend.get_backend().top1_count(z.cuda(), labels.cuda(), m.buf, B, C)
    _, hits, rows, _ = m.read()
    assert hits == int(counts[3]) and rows == B == int(counts[0] + counts[1])


def test_split_updates_repeat_runs_and_a_captured_update():
    calm.backend.set_loss_kernels(True)
    C = 257
    z, labels = F.make_case(130, C, torch.bfloat16, inf_row=False)
    z, labels = z.cuda(), labels.cuda()

    def run(parts):
        m = trainer.EvalMetrics(C, confusion=True, device="cuda")
        for p in parts:
            m.update(z[p], labels[p])
        return m
    one, again = run([slice(0, 130)]), run([slice(0, 130)])
    three = run([slice(0, 7), slice(7, 64), slice(64, 130)])
    assert F.mismatches(one.counts, one.confusion, F.reference(z, labels, KS), 2) == []
    assert torch.equal(three.counts, one.counts) and torch.equal(three.confusion, one.confusion)
    for a, b in zip(one.tensors(), again.tensors()):
        assert torch.equal(a, b)                                          # bit for bit, the loss sum included
    # captured: warmed up on a side stream (the records are allocated there), zeroed, captured, replayed three times
    m = trainer.EvalMetrics(C, confusion=True, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.update(z, labels)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    m.reset()
    records = m._records.data_ptr()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.update(z, labels)
    assert m._records.data_ptr() == records
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(m.counts, 3 * one.counts) and torch.equal(m.confusion, 3 * one.confusion)
    assert torch.equal(m.loss_sum, 3 * one.loss_sum)                      # (three exact additions of one fp32 value)
    rep = m.read()
    assert rep["n"] == 3 * 128 and rep["top1"] == one.read()["top1"]


def test_evaluate_report_lean_graph_on_the_nano48_model_equals_the_report_from_its_logits():
    name = "nano48_cls"
    cfg = CONFIGS[name]
    m = build_model(name, load_golden(name), "cuda").train()
    xs = torch.from_numpy(W.make_input((10, 3, cfg.seq_length, cfg.seq_length), 5)).cuda()
    with torch.no_grad():
        logits = trainer.Predictor(m)(xs)[0].reshape(10, -1).float()
    C = logits.shape[1]
    labels = logits.argmax(dim=1)
    labels[::3] = (labels[::3] + 1) % C
    labels[4] = -100
    batches = [(xs[0:4], labels[0:4]), (xs[4:8], labels[4:8]), (xs[8:10], labels[8:10])]   # two replays, one ragged batch
    ref = F.reference(logits, labels, KS)
    for on in (True, False):
        calm.backend.set_loss_kernels(on)
        rep = trainer.evaluate(m, batches, lean=True, graph=True, report=True, confusion=True)
        assert m.training
        n = int(ref["counts"][0])
        assert (rep["n"], rep["skipped"], rep["nonfinite"]) == (n, 1, 0) and n == 9
        assert rep["top1"] == int(ref["counts"][3]) / n == 5 / 9 and rep["top5"] == int(ref["counts"][4]) / n
        assert abs(rep["loss"] - ref["loss_sum"] / n) <= LOSS_TOL * abs(ref["loss_sum"] / n)
        assert torch.equal(rep["confusion"], torch.from_numpy(ref["confusion"]))
        support, hits1 = torch.from_numpy(ref["counts"][7:7 + C]).double(), torch.from_numpy(ref["counts"][7 + C:]).double()
        want = torch.where(support > 0, hits1 / support.clamp(min=1), torch.full_like(support, -1.0))
        assert torch.equal(rep["per_class_accuracy"].nan_to_num(nan=-1.0), want)
    assert trainer.evaluate(m, batches[:2], lean=True, graph=True) == pytest.approx(
        int((logits[:8].argmax(1) == labels[:8]).sum()) / 8)
