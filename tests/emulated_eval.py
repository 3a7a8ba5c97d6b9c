"""CPU emulation of calm_eval_metrics on top of tests/emulated_backend.py — used by tests/test_eval_*.py only.  It is never
imported by the package.

It mirrors the two launches in fp32: one record per row {nll = (max - z_l) + log(sum exp(z - max)), beaten, pred, flags}
(csrc/loss.hip: eval_rows_kernel), then the fold of the records into counts / loss_sum / confusion (eval_fold_kernel; the
batch's fp32 loss sum is added to the float64 accumulator).  `eval_fault` plants a defect for the tests that check the
checker (tests/eval_f64.py):
    "tie_high"         a tie at the label's value counts against the label when the other index is HIGHER
    "le_k"             hit when beaten <= k
    "nan_hit"          a row holding a NaN is treated as finite (NaN compares false: nothing beats its label)
    "skipped_in_rows"  a skipped row is counted in rows as well
    "confusion_T"      confusion[pred, label]"""
import numpy as np
import torch

from emulated_ema import EmaMixin
from emulated_infer import EmulatedInferBackend

SKIPPED, NONFINITE = 1, 2


def emu_records(logits, labels, fault=None):
    """(nll fp32 [B], beaten, pred, flags int32 [B]) as launch 1 writes them."""
    z = logits.detach().float().cpu().numpy()
    lab = labels.detach().cpu().numpy().astype(np.int64)
    B, C = z.shape
    nll = np.zeros(B, np.float32)
    beaten, pred, flags = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    cls = np.arange(C)
    with np.errstate(all="ignore"):
        for b in range(B):
            l = int(lab[b])
            if not 0 <= l < C:
                flags[b] = SKIPPED
                continue
            row = z[b]
            zl = row[l]
            nan = bool(np.isnan(row).any())
            if nan and fault != "nan_hit":
                flags[b] = NONFINITE
            zm = np.float32(np.nanmax(row)) if not np.isnan(row).all() else np.float32(-np.inf)
            pred[b] = int(np.flatnonzero(row == zm)[0]) if (row == zm).any() else 0
            tie_side = cls > l if fault == "tie_high" else cls < l
            beaten[b] = int(((row > zl) | ((row == zl) & tie_side)).sum())
            se = np.float32(np.exp(row - zm, dtype=np.float32).sum(dtype=np.float32))
            nll[b] = np.float32(zm - zl) + np.log(se, dtype=np.float32)
    return nll, beaten, pred, flags


def emu_fold(records, labels, ks, counts, loss_sum, confusion, C, fault=None):
    nll, beaten, pred, flags = records
    lab = labels.detach().cpu().numpy().astype(np.int64)
    cnt = counts.numpy()
    s = np.float32(0.0)
    for b in range(len(lab)):
        if flags[b] & SKIPPED:
            cnt[1] += 1
            if fault == "skipped_in_rows":
                cnt[0] += 1
            continue
        l = int(lab[b])
        cnt[0] += 1
        cnt[7 + l] += 1
        if flags[b] & NONFINITE:
            cnt[2] += 1
            continue
        with np.errstate(all="ignore"):
            s = np.float32(s + nll[b])
        for i, k in enumerate(ks):
            cnt[3 + i] += (beaten[b] <= k) if fault == "le_k" else (beaten[b] < k)
        cnt[7 + C + l] += pred[b] == l
        if confusion is not None:
            if fault == "confusion_T":
                confusion[int(pred[b]), l] += 1
            else:
                confusion[l, int(pred[b])] += 1
    loss_sum += float(s)


class EvalMixin:
    """eval_metrics with HipBackend's signature (and its refusals) over CPU tensors."""
    eval_fault = None

    def eval_metrics(self, logits, labels, ks, counts, loss_sum, confusion, B, C, partials=None):
        if not 1 <= len(ks) <= 4 or any(k < 1 for k in ks) or logits.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError("calm_eval_metrics failed: code -1 (invalid argument/unsupported shape)")
        if C > 65536:
            raise RuntimeError("calm_eval_metrics failed: code -3 (invalid argument/unsupported shape)")
        if counts.dtype != torch.int64 or loss_sum.dtype != torch.float64 or counts.numel() < 7 + 2 * C:
            raise TypeError("eval_metrics: int64 counts [7 + 2C] and float64 loss_sum expected")
        if partials is not None and partials.numel() < 4 * B:
            raise ValueError("eval_metrics: partials holds one 16-byte record per row")
        self.eval_calls = getattr(self, "eval_calls", 0) + 1
        emu_fold(emu_records(logits, labels, self.eval_fault), labels, list(ks), counts, loss_sum, confusion, C,
                 self.eval_fault)


class EmulatedEvalBackend(EvalMixin, EmaMixin, EmulatedInferBackend):
    """The emulated C-ABI with the validation metrics, the weight EMA and the lean inference entry points: what
    train(val_dataset=..., ema=...) needs on a host without a GPU."""
    name = "emulated+eval"

