"""CPU emulation of the three entry points of csrc/knn.hip — used by tests/test_knn_*.py only.  It is never imported by the
package.

The selection is a numpy lexsort on the kernel's own order-preserving uint32 key (the checker, tests/knn_f64.py, sorts
float64 values over the whole bank; trainer.knn_merge_torch does two stable torch sorts); normalisation and vote are fp32
torch expressions.  `knn_fault` plants a defect for the tests that check the checker:
    "tie_high"           equal similarities: the HIGHER bank index first
    "k_plus_one"         the state holds ranks 1 .. k instead of 0 .. k - 1
    "base_ignored"       a chunk's indices start at 0 whatever base is
    "state_dropped"      the old state is not merged in
    "unsorted"           the best k, in reversed order
    "neg_zero_low"       -0.0 ranks below +0.0
    "nan_high"           a NaN ranks above everything
    "empty_beats_inf"    an empty slot ranks above a real -inf
    "t_multiplied"       the vote multiplies by T instead of dividing
    "no_shift"           the vote does not subtract the row's largest similarity
    "label_oob_clamped"  a label outside [0, C) votes for the nearest class
    "empty_reads_label"  an empty slot (index -1) reads bank_labels[-1] and votes
    "bad_row_kept"       a zero or non-finite row is counted but divided anyway
    "bad_uncounted"      a zero or non-finite row is zeroed but not counted"""
import numpy as np
import torch

from emulated_mim import EmulatedMimBackend

MERGE_FAULTS = ("tie_high", "k_plus_one", "base_ignored", "state_dropped", "unsorted", "neg_zero_low", "nan_high",
                "empty_beats_inf")
VOTE_FAULTS = ("t_multiplied", "no_shift", "label_oob_clamped", "empty_reads_label")
NORMALIZE_FAULTS = ("bad_row_kept", "bad_uncounted")
FAULTS = MERGE_FAULTS + VOTE_FAULTS + NORMALIZE_FAULTS
# the checks of knn_f64.CHECKS a fault may show in (the realistic cases normalise, select and never vote)
CONCERNS = {**{f: {"exact", "rows", "realistic"} for f in MERGE_FAULTS}, **{f: {"vote"} for f in VOTE_FAULTS},
            **{f: {"normalize"} for f in NORMALIZE_FAULTS}}


def normalize(x, fault=None):
    xf = x.float()
    nrm = (xf * xf).sum(dim=1).sqrt()
    ok = torch.isfinite(xf).all(dim=1) & (nrm > 0) & torch.isfinite(nrm)
    out = xf / nrm[:, None]
    if fault != "bad_row_kept":
        out = torch.where(ok[:, None], out, torch.zeros_like(out))
    return out, 0 if fault == "bad_uncounted" else int((~ok).sum())


def keys(bits, fault=None):
    """int64 numpy: the order-preserving key of stored fp32 bits (uint32 numpy)."""
    u = bits.astype(np.uint32)
    if fault != "neg_zero_low":
        u = np.where(u == np.uint32(0x80000000), np.uint32(0), u)
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.int64)


def merge(sims, base, best_sim, best_idx, fault=None):
    """The new (best_sim, best_idx) numpy pair."""
    s = np.array(sims, dtype=np.float32)
    Nq, n = s.shape
    k = best_sim.shape[1]
    nan = np.isnan(s)
    s[nan] = -np.inf
    idx = np.broadcast_to((0 if fault == "base_ignored" else int(base)) + np.arange(n, dtype=np.int64), (Nq, n))
    top = nan
    if fault != "state_dropped":
        s = np.concatenate([np.asarray(best_sim, dtype=np.float32), s], axis=1)
        idx = np.concatenate([np.asarray(best_idx, dtype=np.int64), idx], axis=1)
        top = np.concatenate([np.zeros((Nq, k), dtype=bool), nan], axis=1)
    key = keys(s.view(np.uint32), fault)
    key[idx < 0] = 0x00800000 if fault == "empty_beats_inf" else 0
    if fault == "nan_high":
        key[top] = 1 << 33
    out_s = np.full((Nq, k), -np.inf, dtype=np.float32)
    out_i = np.full((Nq, k), -1, dtype=np.int64)
    for q in range(Nq):
        order = np.lexsort((-idx[q] if fault == "tie_high" else idx[q], -key[q]))
        order = order[1:k + 1] if fault == "k_plus_one" else order[:k]
        if fault == "unsorted":
            order = order[::-1]
        out_s[q, :len(order)] = s[q, order]
        out_i[q, :len(order)] = idx[q, order]
    out_s[out_i < 0] = -np.inf
    return out_s, out_i


def vote(best_sim, best_idx, labels, inv_T, C, fault=None):
    Nq, k = best_sim.shape
    Nb = labels.numel()
    scale = np.float32(1.0 / inv_T if fault == "t_multiplied" else inv_T)
    scores = torch.zeros(Nq, C, dtype=torch.float32)
    rows = torch.arange(Nq)
    s0 = best_sim[:, 0]
    for j in range(k):
        i, s = best_idx[:, j], best_sim[:, j]
        inside = (i >= 0) & (i < Nb)
        if fault == "empty_reads_label":
            inside = (i >= -1) & (i < Nb)
        lab = labels[torch.where(i < 0, i + Nb, i).clamp(0, Nb - 1)]
        if fault == "label_oob_clamped":
            lab = lab.clamp(0, C - 1)
        votes = inside & (lab >= 0) & (lab < C)
        d = s if fault == "no_shift" else torch.where(s == s0, torch.zeros_like(s), s - s0)
        w = torch.exp(d * float(scale))
        scores[rows[votes], lab[votes]] += w[votes]
    return scores


def _fail(name, code):
    raise RuntimeError(f"{name} failed: code {code} (invalid argument/unsupported shape)")


class KnnMixin:
    """knn_normalize / knn_merge / knn_vote with HipBackend's signatures (and the library's refusals) over CPU tensors."""
    knn_fault = None

    def knn_normalize(self, x, out, bad, N, D):
        if N < 0 or D < 1 or x.dtype not in (torch.float32, torch.bfloat16):
            _fail("calm_knn_normalize", -1)
        if D > 4096:
            _fail("calm_knn_normalize", -3)
        self.knn_calls = getattr(self, "knn_calls", 0) + 1
        o, n = normalize(x, self.knn_fault)
        out.copy_(o)
        bad[0] += n

    def knn_merge(self, sims, base, best_sim, best_idx, Nq, n, k):
        if k < 1 or n < 1 or Nq < 0 or base < 0 or sims.dtype != torch.float32:
            _fail("calm_knn_merge", -1)
        if k > 256:
            _fail("calm_knn_merge", -3)
        self.knn_calls = getattr(self, "knn_calls", 0) + 1
        s, i = merge(sims.numpy(), base, best_sim.numpy(), best_idx.numpy(), self.knn_fault)
        best_sim.copy_(torch.from_numpy(s))
        best_idx.copy_(torch.from_numpy(i))

    def knn_vote(self, best_sim, best_idx, bank_labels, inv_T, scores, Nq, k, C):
        if k < 1 or C < 1 or Nq < 0 or not 0 < inv_T < float("inf"):
            _fail("calm_knn_vote", -1)
        if k > 256:
            _fail("calm_knn_vote", -3)
        self.knn_calls = getattr(self, "knn_calls", 0) + 1
        scores.copy_(vote(best_sim, best_idx, bank_labels, inv_T, C, self.knn_fault))


class EmulatedKnnBackend(KnnMixin, EmulatedMimBackend):
    """The emulated C-ABI with the k-NN probe's entry points: what KnnProbe and train(knn=) need on a host without a GPU."""
    name = "emulated+knn"
