"""CPU emulation of the four entry points of csrc/mim.hip on top of tests/emulated_dropout.py (the numpy Philox) and
tests/emulated_recon.py — used by tests/test_mim_*.py only.  It is never imported by the package.

The mask comes from a stable argsort of the words (the checker, tests/mim_f64.py, counts compares instead); apply and the
loss pair are fp32 torch expressions over the per-element mask.  `mim_fault` plants a defect for the tests that check the
checker:
    "tie_high"        equal words: the HIGHER patch index ranks first
    "rank_le"         rank <= k instead of rank < k
    "transposed"      the patch of pixel (r, x) is (x / p) * G + r / p
    "stride_P"        the words of sample s start at element s * P instead of s * 1024
    "sample0"         sample0 is ignored
    "fill_swapped"    fill channels 0 and 2 are exchanged
    "inverted"        the loss pair looks where the mask is NOT set
    "divisor"         the loss pair divides by 3 B S^2
    "grad_leak"       dtokens holds the unmasked gradient outside the mask
    "clamp_one"       the backward clamps to [-1, 1] whatever delta is
    "multiply"        value * mask instead of a select (a NaN outside the mask leaks)"""
import numpy as np
import torch

from emulated_dropout import philox4x32_10
from emulated_recon import EmulatedReconBackend

FAULTS = ("tie_high", "rank_le", "transposed", "stride_P", "sample0", "fill_swapped", "inverted", "divisor", "grad_leak",
          "clamp_one", "multiply")


def words(key, sample0, B, P, stride=1024):
    """uint32 [B, P]: w(b, i) = word((sample0 + b) * stride + i) of the dropout generator under key = (seed, offset)."""
    seed, offset = (int(v) & (2 ** 64 - 1) for v in key)              # int64 bit patterns read as uint64
    e = ((np.uint64(sample0) + np.arange(B, dtype=np.uint64)) * np.uint64(stride))[:, None] + np.arange(P, dtype=np.uint64)[None, :]
    g, z = e >> np.uint64(2), np.zeros_like(e)
    w = philox4x32_10((g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), z + np.uint64(offset & 0xFFFFFFFF), z + np.uint64(offset >> 32)),
                      (seed & 0xFFFFFFFF, seed >> 32))
    return np.take_along_axis(np.stack(w, axis=-1), (e & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0]


def draw(key, sample0, B, G, k, fault=None):
    """uint8 numpy [B, G * G]: the k lowest-ranked patches of every sample."""
    P = G * G
    if B == 0:
        return np.zeros((0, P), np.uint8)
    w = words(key, 0 if fault == "sample0" else sample0, B, P, P if fault == "stride_P" else 1024)
    if fault == "tie_high":                                           # among equals the higher index first
        order = np.stack([np.lexsort((-np.arange(P), w[b])) for b in range(B)])
    else:
        order = np.argsort(w, axis=1, kind="stable")                  # by (word, index)
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(P), order.shape), axis=1)
    return (rank <= k if fault == "rank_le" else rank < k).astype(np.uint8)


def element_mask(mask, S, p, fault=None):
    """bool torch [B, S, 3S]: the decision of every element."""
    mask = torch.as_tensor(mask)
    B, G = mask.shape[0], S // p
    grid = mask.reshape(B, G, G) != 0
    if fault == "transposed":
        grid = grid.transpose(1, 2)
    return grid.reshape(B, G, 1, G, 1).expand(B, G, p, G, 3 * p).reshape(B, S, 3 * S)


def apply(x, mask, fill, p, fault=None):
    B, S, _ = x.shape
    f = torch.tensor([float(v) for v in fill], dtype=torch.float32)
    if fault == "fill_swapped":
        f = f.flip(0)
    m = element_mask(mask.cpu(), S, p, fault).to(x.device)
    return torch.where(m, f.to(x.device).repeat(S).expand(B, S, 3 * S), x)


def _count(B, S, p, masked, fault):
    return np.float32(3.0 * B * S * S if fault == "divisor" else 3.0 * p * p * masked)


def huber_fwd(tokens, target, mask, delta, p, masked, fault=None):
    B, S, _ = tokens.shape
    m = element_mask(mask.cpu(), S, p, fault).to(tokens.device)
    if fault == "inverted":
        m = ~m
    d = tokens.detach().float() - target.detach().float()
    ad = d.abs()
    h = torch.where(ad <= delta, 0.5 * d * d, delta * (ad - 0.5 * delta))
    h = h * m if fault == "multiply" else torch.where(m, h, torch.zeros(()))
    return (h.sum(dtype=torch.float32) / float(_count(B, S, p, masked, fault))).reshape(())


def huber_bwd(tokens, target, mask, delta, dloss, p, masked, fault=None):
    B, S, _ = tokens.shape
    m = element_mask(mask.cpu(), S, p, fault).to(tokens.device)
    if fault == "inverted":
        m = ~m
    d = tokens.detach().float() - target.detach().float()
    lim = 1.0 if fault == "clamp_one" else delta
    g = (dloss.reshape(()).float() / float(_count(B, S, p, masked, fault))) * torch.where(d != d, d, d.clamp(-lim, lim))
    if fault == "grad_leak":
        return g
    return g * m if fault == "multiply" else torch.where(m, g, torch.zeros(()))


def _fail(name, code):
    raise RuntimeError(f"{name} failed: code {code} (invalid argument/unsupported shape)")


class MimMixin:
    """mim_draw / mim_apply / mim_huber_fwd / mim_huber_bwd with HipBackend's signatures (and the library's refusals) over CPU
    tensors."""
    mim_fault = None

    @staticmethod
    def _geom(name, B, S, p):
        if S <= 0 or p <= 0 or S % p:
            _fail(name, -1)
        if S // p > 32 or 3 * B * S * S >= 1 << 31:
            _fail(name, -3)

    def mim_draw(self, mask, B, G, k, key, sample0=0):
        if key is None or key.dtype != torch.int64 or key.numel() != 2:
            raise TypeError("mim_draw expects its key as a contiguous int64 tensor of two elements (seed, offset)")
        if B < 0 or G < 1 or k < 0 or k > G * G or sample0 < 0 or sample0 + B > 1 << 53:
            _fail("calm_mim_draw", -1)
        if G > 32:
            _fail("calm_mim_draw", -3)
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (B, G * G):
            raise TypeError("mim_draw expects its mask as a contiguous uint8 tensor [B, P]")
        self.mim_draw_calls = getattr(self, "mim_draw_calls", 0) + 1
        mask.copy_(torch.from_numpy(draw([int(v) for v in key], sample0, B, G, k, self.mim_fault)))

    def mim_apply(self, x, y, mask, fill, B, S, p):
        if B < 0:
            _fail("calm_mim_apply", -1)
        self._geom("calm_mim_apply", B, S, p)
        y.copy_(apply(x.reshape(B, S, 3 * S), mask, fill, p, self.mim_fault).reshape(y.shape))

    def mim_huber_fwd(self, tokens, target, mask, delta, loss, B, S, p, masked):
        if B <= 0 or not 0 < delta < float("inf") or masked <= 0 or tokens.dtype != torch.float32:
            _fail("calm_mim_huber_fwd", -1)
        self._geom("calm_mim_huber_fwd", B, S, p)
        if masked > B * (S // p) ** 2:
            _fail("calm_mim_huber_fwd", -1)
        self.mim_huber_calls = getattr(self, "mim_huber_calls", 0) + 1
        loss.copy_(huber_fwd(tokens.reshape(B, S, 3 * S), target.reshape(B, S, 3 * S), mask, delta, p, masked, self.mim_fault))

    def mim_huber_bwd(self, tokens, target, mask, delta, dloss, dtokens, B, S, p, masked):
        if B <= 0 or not 0 < delta < float("inf") or masked <= 0 or masked > B * (S // p) ** 2:
            _fail("calm_mim_huber_bwd", -1)
        self._geom("calm_mim_huber_bwd", B, S, p)
        dtokens.copy_(huber_bwd(tokens.reshape(B, S, 3 * S), target.reshape(B, S, 3 * S), mask, delta, dloss, p, masked,
                                self.mim_fault).reshape(dtokens.shape))


class EmulatedMimBackend(MimMixin, EmulatedReconBackend):
    """The emulated C-ABI with the masked-image-modelling entry points: what train(task="reg", mim=...) needs on a host
    without a GPU."""
    name = "emulated+mim"
