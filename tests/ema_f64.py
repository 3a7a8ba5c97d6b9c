"""TEST INFRASTRUCTURE: float64 reference and element-wise checker of the weight EMA (calm_ema_update / calm_ema_swap,
csrc/ema.hip; trainer.ModelEMA on CPU parameters).  Nothing here depends on what the code under test returns.

Update.  For fp32 inputs e (the average), x (the parameter) and the weight w the device reports in weight_out[0], the
reference is r = e + w * (x - e) in float64 and EVERY element has to satisfy
    |e' - r| <= 4 * 2^-24 * max(|e|, |x|)
The bound is the arithmetic's own: fp32 rounds x - e (an error of at most 2^-24 |x - e| <= 2^-24 * 2 max, scaled by
w < 1), the product w * (x - e) (|w (x - e)| <= |x| + |e| <= 2 max) and the sum (the result lies between e and x) — or
product and sum in one fused rounding.  Both forms, and torch's Tensor.lerp_ (which for w >= 0.5 evaluates
x - (x - e) * (1 - w), 1 - w exact), stay below 4 units of 2^-24 * max.  Inputs are exactly 0 or have magnitudes in
[1e-6, 1e4], so no result is subnormal and the relative rounding model holds for every element.

Weight.  The reported w has to be within 2 * 2^-24 of 1 - d evaluated in float64 from the fp32 decay, d = decay
(constant) or min(decay, (1 + n) / (10 + n)) (warm-up, n = updates applied before this one): one rounding for the
division and one for the subtraction, both of values <= 1.

Swap, skip.  Bit equality on the int32 view (NaN payloads included)."""
import numpy as np

EMA_CONSTANT, EMA_WARMUP = 0, 1
U = 2.0 ** -24


def make_values(numel, seed, zero_fraction=0.125):
    """Seeded fp32 values: exactly 0, or +/- a magnitude drawn log-uniformly from [1e-6, 1e4]."""
    g = np.random.default_rng(seed)
    mag = np.exp(g.uniform(np.log(1e-6), np.log(1e4), numel))
    v = (mag * g.choice((-1.0, 1.0), numel)).astype(np.float32)
    v = np.clip(np.abs(v), np.float32(1e-6), np.float32(1e4)) * np.sign(v)          # the cast cannot leave the range
    v[g.random(numel) < zero_fraction] = 0.0
    return v.astype(np.float32)


def reference_weight(decay, schedule, n):
    """1 - d in float64 from the fp32 decay."""
    d = float(np.float32(decay))
    if schedule == EMA_WARMUP:
        d = min(d, (1.0 + n) / (10.0 + n))
    return 1.0 - d


def check_weight(w_reported, decay, schedule, n):
    ref = reference_weight(decay, schedule, n)
    err = abs(float(w_reported) - ref)
    assert err <= 2 * U, f"w = {float(w_reported)!r} for n = {n}: {err:.3e} from the float64 value {ref!r} (bound {2 * U:.3e})"
    return err


def check_update(e_before, x, e_after, w):
    """Every element of e_after against the float64 recurrence from e_before, x and the reported w.  Returns the worst
    error in units of the bound; raises AssertionError naming the first offending element."""
    e0 = np.asarray(e_before, dtype=np.float32).reshape(-1)
    xs = np.asarray(x, dtype=np.float32).reshape(-1)
    e1 = np.asarray(e_after, dtype=np.float32).reshape(-1)
    assert e0.shape == xs.shape == e1.shape, (e0.shape, xs.shape, e1.shape)
    assert np.isfinite(e1).all(), "non-finite average"
    r = e0.astype(np.float64) + float(w) * (xs.astype(np.float64) - e0.astype(np.float64))
    bound = 4 * U * np.maximum(np.abs(e0), np.abs(xs)).astype(np.float64)
    err = np.abs(e1.astype(np.float64) - r)
    bad = np.flatnonzero(err > bound)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{bad.size} of {err.size} elements outside the bound; first at {i}: e {e0[i]!r} x {xs[i]!r} "
                             f"-> {e1[i]!r}, float64 {r[i]!r}, error {err[i]:.3e} > {bound[i]:.3e}")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).reshape(-1).view(np.int32)


def check_bits_equal(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert not bad.size, f"{what}: {bad.size} of {g.size} words differ, first at {int(bad[0])}"


def check_swap(src_before, ema_before, src_after, ema_after):
    """An exchange: the parameter holds the average's bits and the average the parameter's."""
    check_bits_equal(src_after, ema_before, "parameter after the swap vs average before")
    check_bits_equal(ema_after, src_before, "average after the swap vs parameter before")


def table_numels(chunk):
    """The sizes at which the kernels can go wrong: below / at / above one 16-byte vector, partial and whole 256-thread
    sweeps, one element short of / exactly / one past a chunk, several chunks with a tail."""
    return [1, 3, 4, 5, 255, 256, 1023, chunk - 1, chunk, chunk + 1, 2 * chunk + 7]


def make_table(chunk, device, seed=0):
    """[(src, ema)] fp32 pairs on `device` with seeded values (make_values): the sizes of table_numels, a 0-d tensor, one
    pair whose average starts one float into a larger buffer (mixed alignment: the scalar path), one pair with both
    tensors one float in (equally misaligned: scalar as well), and a pair without elements (left out of the plan)."""
    import torch

    def tensor(n, s, offset=0, shape=None):
        buf = torch.zeros(n + 8, dtype=torch.float32, device=device)
        t = buf[offset:offset + n]
        t.copy_(torch.from_numpy(make_values(n, s)))
        assert t.data_ptr() % 16 == 4 * offset % 16
        return t.reshape(shape) if shape is not None else t

    pairs = [(tensor(n, seed + 2 * i), tensor(n, seed + 2 * i + 1)) for i, n in enumerate(table_numels(chunk))]
    pairs.append((tensor(1, seed + 100, shape=()), tensor(1, seed + 101, shape=())))
    pairs.append((tensor(chunk + 37, seed + 102), tensor(chunk + 37, seed + 103, offset=1)))
    pairs.append((tensor(chunk + 37, seed + 104, offset=1), tensor(chunk + 37, seed + 105, offset=1)))
    pairs.append((torch.zeros(0, 3, device=device), torch.zeros(0, 3, device=device)))
    return pairs
