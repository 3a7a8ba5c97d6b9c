"""CPU emulation of calm_dropout (csrc/dropout.hip) on top of tests/emulated_backend.py: a numpy Philox4x32-10, the
threshold / scale of the entry point and its two separately rounded fp32 operations — used by tests/test_dropout_*.py and
tests/golden/make_golden_dropout.py only.  It is never imported by the package."""
import numpy as np
import torch

from emulated_backend import EmulatedBackend

M0, M1 = 0xD2511F53, 0xCD9E8D57                    # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85                    # key increments
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two integers -> four uint32 arrays (Salmon et al., SC'11)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _LO for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def dropout_words(seed, offset, e0, n):
    """word(e) for e = e0 .. e0 + n - 1 as a uint32 array: output word e & 3 of the call with counter
    (lo32(e >> 2), hi32(e >> 2), lo32(offset), hi32(offset)) and key (lo32(seed), hi32(seed))."""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)           # int64 bit patterns read as uint64
    g = np.arange(e0 >> 2, ((e0 + n + 3) >> 2) + 1, dtype=np.uint64)
    z = np.zeros_like(g)
    w = philox4x32_10((g & _LO, g >> _S32, z + np.uint64(offset & 0xFFFFFFFF), z + np.uint64(offset >> 32)),
                      (seed & 0xFFFFFFFF, seed >> 32))
    first = e0 & 3
    return np.stack(w, axis=1).reshape(-1)[first:first + n]


def threshold_and_scale(p):
    """What the entry point computes on the host from its fp32 argument p."""
    p32 = np.float32(p)
    return int(float(p32) * 4294967296.0), np.float32(1.0) / (np.float32(1.0) - p32)


def keep_mask(seed, offset, e0, n, p):
    """Boolean numpy array: element e0 + j is kept."""
    return dropout_words(seed, offset, e0, n) >= np.uint32(threshold_and_scale(p)[0])


def multiplier(key, e0, n, p):
    """fp32 torch tensor [n]: scale where kept, 0 where dropped; key: the (seed, offset) tensor or pair."""
    seed, offset = (int(k) for k in key)
    scale = threshold_and_scale(p)[1]
    return torch.from_numpy(np.where(keep_mask(seed, offset, e0, n, p), scale, np.float32(0.0)).astype(np.float32))


class EmulatedDropoutBackend(EmulatedBackend):
    def dropout(self, x, residual, y, n, p, key, e0=0):
        if not 0.0 <= float(np.float32(p)) < 1.0 or e0 < 0 or e0 % 4:
            raise RuntimeError("calm_dropout failed: code -1 (invalid argument/unsupported shape)")
        if n == 0:
            return
        v = x.reshape(-1)[:n].float() * multiplier(key, e0, n, p).to(x.device)      # one fp32 rounding (bf16 widens exactly)
        if residual is not None:
            v = v + residual.reshape(-1)[:n].float()                                # a second one
        y.view(-1)[:n].copy_(v)                                                     # bf16 output: round to nearest even


class KeyStream:
    """Stand-in for ops.draw_dropout_key: the i-th call returns (seed, i)."""

    def __init__(self, seed):
        self.seed = seed
        self.n = 0

    def __call__(self, device):
        key = torch.tensor([self.seed, self.n], dtype=torch.int64, device=device)
        self.n += 1
        return key
