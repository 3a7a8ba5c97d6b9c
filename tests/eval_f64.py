"""float64 checker of the validation metrics (calm_eval_metrics, trainer.EvalMetrics) — used by tests/test_eval_*.py only.

`reference` recomputes every integer and the loss sum from the given logits and labels with the definitions of
include/calm_vit.h, row by row in numpy: class c BEATS label l when z_c > z_l, or z_c == z_l and c < l; the label is in
the top k exactly when fewer than k classes beat it; the prediction is the lowest index among the maximal values; a row
whose label is outside [0, C) is skipped (counted in `skipped` and in nothing else); a row holding a NaN is counted in
rows, nonfinite and its class's support, never as a hit, and adds to neither the loss sum nor the confusion matrix.  The
integers come from comparisons of the stored values (bf16 and fp32 convert to float64 exactly), so they are exact; the
loss sum is torch's float64 cross_entropy over the finite rows.

`make_case` builds the seeded inputs both test files share and `mismatches` lists what differs between a result and the
reference."""
import numpy as np
import torch
import torch.nn.functional as F

HEAD = 7                 # counts: rows, skipped, nonfinite, hits@ks[0..3], then support[C], hits1[C]
# (B, C): smallest; C < every k and a partial workgroup; fewer classes than lanes with a scalar tail; the 1000-class row;
# C % 4 != 0; more rows than one chunk of the fold; a fold thread owning two classes
SHAPES = [(1, 1), (3, 3), (5, 63), (7, 1000), (130, 257), (1030, 10), (9, 1030)]


def reference(logits, labels, ks):
    """{"counts": int64 [7 + 2C], "loss_sum": float, "confusion": int64 [C,C]} of one batch, from zeroed accumulators."""
    z = logits.detach().cpu().double().numpy()
    lab = labels.detach().cpu().numpy().astype(np.int64)
    B, C = z.shape
    counts = np.zeros(HEAD + 2 * C, dtype=np.int64)
    confusion = np.zeros((C, C), dtype=np.int64)
    finite_rows = []
    for b in range(B):
        l = int(lab[b])
        if not 0 <= l < C:
            counts[1] += 1
            continue
        counts[0] += 1
        counts[HEAD + l] += 1
        row = z[b]
        if np.isnan(row).any():
            counts[2] += 1
            continue
        finite_rows.append(b)
        beaten = int((row > row[l]).sum() + (row[:l] == row[l]).sum())
        pred = int(np.flatnonzero(row == row.max())[0])
        for i, k in enumerate(ks):
            counts[3 + i] += beaten < k
        counts[HEAD + C + l] += pred == l
        confusion[l, pred] += 1
    loss_sum = 0.0
    if finite_rows:
        idx = torch.tensor(finite_rows)
        loss_sum = float(F.cross_entropy(logits.detach().cpu().double()[idx], labels.detach().cpu().long()[idx],
                                         reduction="sum"))
    return {"counts": counts, "loss_sum": loss_sum, "confusion": confusion}


def mismatches(counts, confusion, ref, nk):
    """Names of the integer results that differ from the reference ([] when all are equal).  confusion may be None."""
    counts = np.asarray(counts.detach().cpu() if isinstance(counts, torch.Tensor) else counts)
    C = (len(counts) - HEAD) // 2
    bad = []
    names = ["rows", "skipped", "nonfinite"] + [f"hits@k[{i}]" for i in range(nk)]
    for i, n in enumerate(names):
        if counts[i] != ref["counts"][i]:
            bad.append(f"{n}: {int(counts[i])} != {int(ref['counts'][i])}")
    if any(counts[3 + nk:HEAD] != 0):
        bad.append("unused hit slots written")
    if not np.array_equal(counts[HEAD:HEAD + C], ref["counts"][HEAD:HEAD + C]):
        bad.append("support")
    if not np.array_equal(counts[HEAD + C:], ref["counts"][HEAD + C:]):
        bad.append("hits1")
    if confusion is not None:
        got = np.asarray(confusion.detach().cpu() if isinstance(confusion, torch.Tensor) else confusion)
        if not np.array_equal(got.reshape(C, C), ref["confusion"]):
            bad.append("confusion")
    return bad


def loss_error(got, want):
    """Relative error of a loss sum; 0 when both are the same non-finite value or both NaN."""
    if not np.isfinite(want) or not np.isfinite(got):
        return 0.0 if (np.isnan(want) and np.isnan(got)) or got == want else float("inf")
    return abs(got - want) / max(abs(want), 1e-30)


def make_case(B, C, dtype=torch.float32, seed=0, inf_row=True):
    """(logits [B,C] of `dtype`, labels [B] int64), seeded.  Where B allows: row 1 has label -100, row 2 label C, row 3
    holds a NaN, row 4 is all -inf (inf_row=True; its loss is NaN, so loss checks use inf_row=False).  Every third other
    row has exact ties at the label's value on both sides of its index, every third some -inf entries away from the
    label, and every second row's label logit is raised so that top-1 / top-5 hits and misses both occur."""
    g = torch.Generator().manual_seed(1000 * B + C + seed)
    z = (torch.randn(B, C, generator=g) * 3.0).to(dtype).float()           # (values the storage type holds exactly)
    labels = torch.randint(0, C, (B,), generator=g)
    for b in range(B):
        l = int(labels[b])
        if b % 2 == 0:
            z[b, l] = (z[b, l] + 4.0).to(dtype).float()
        if b % 3 == 0:
            for c in (l - 1, l + 1, l + 3):                     # one below, two above: the side of the tie rule shows
                if 0 <= c < C:
                    z[b, c] = z[b, l]
        if b % 3 == 1:
            for c in torch.randint(0, C, (max(C // 8, 1),), generator=g).tolist():
                if c != l:
                    z[b, c] = float("-inf")
    if B > 1:
        labels[1] = -100
    if B > 2:
        labels[2] = C
    if B > 3:
        z[3, int(torch.randint(0, C, (1,), generator=g))] = float("nan")
    if B > 4 and inf_row:
        z[4, :] = float("-inf")
    return z.to(dtype), labels
