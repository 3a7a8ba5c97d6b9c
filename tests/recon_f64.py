"""float64 checker of the reconstruction metrics (calm_recon_metrics, trainer.ReconMetrics) and of the rows Huber pair — used
by tests/test_recon_*.py only.

`reference` recomputes the eight accumulator slots of one batch from the definitions of include/calm_vit.h in numpy
float64, independently of the kernel's formulation: the SSIM statistics are taken over EXPLICIT 11 x 11 windows
(numpy.lib.stride_tricks.sliding_window_view) with the two-dimensional Gaussian weights, the variances and the covariance as
weighted sums of centred products (no E[x^2] - mu^2, no separable filter), PSNR from the pixel-space mean square error with
the 1e-10 floor.  bf16 and fp32 convert to float64 exactly, so the integer-valued slots are exact.

`make_case` builds the seeded inputs both test files share, `allowance` turns the error of the fp32 torch composition
(trainer.recon_metrics_torch, the yardstick) into the per-slot bound "4 x yardstick + 1e-6 x magnitude", and `mismatches`
lists the slots outside it."""
import numpy as np
import torch
from numpy.lib.stride_tricks import sliding_window_view

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
WIN, SIGMA, C1, C2 = 11, 1.5, 0.01 ** 2, 0.03 ** 2
SLOTS = ["images", "nonfinite", "huber", "abs", "sq", "elements", "psnr", "ssim"]
EXACT = (0, 1, 5)
# (B, S): one valid position; a 2 x 2 valid area; a band that does not divide the valid rows (4 + 2); 9 bands; the nano-48
# image; S % 4 != 0 and a 16-row band that does not divide (90 = 5 * 16 + 10); the 32-row band (130 = 4 * 32 + 2)
SHAPES = [(1, 11), (2, 12), (3, 16), (2, 44), (1, 48), (2, 100)]
EXTRA_SHAPES = [(1, 140)]


def window2d():
    k = np.arange(WIN, dtype=np.float64) - (WIN - 1) / 2
    w = np.exp(-k * k / (2.0 * SIGMA ** 2))
    w2 = np.outer(w, w)
    return w2 / w2.sum()


def _images(tokens, target):
    """(generated, target) as float64 [B,3,S,S]."""
    g = tokens.detach().cpu().double().numpy()
    B, S = g.shape[0], g.shape[1]
    gi = g.reshape(B, S, S, 3).transpose(0, 3, 1, 2)
    t = target.detach().cpu().double().numpy()
    ti = t if t.ndim == 4 else t.reshape(B, S, S, 3).transpose(0, 3, 1, 2)
    return gi, ti


def ssim_image(px, py):
    """Mean SSIM of one image pair in pixel space, [3,S,S] float64, over explicit windows."""
    w = window2d()
    vals = []
    for c in range(3):
        wx = sliding_window_view(px[c], (WIN, WIN))                  # [S-10, S-10, 11, 11]
        wy = sliding_window_view(py[c], (WIN, WIN))
        ux = (wx * w).sum(axis=(2, 3))
        uy = (wy * w).sum(axis=(2, 3))
        dx, dy = wx - ux[:, :, None, None], wy - uy[:, :, None, None]
        sxx = (w * dx * dx).sum(axis=(2, 3))
        syy = (w * dy * dy).sum(axis=(2, 3))
        sxy = (w * dx * dy).sum(axis=(2, 3))
        vals.append(((2 * ux * uy + C1) * (2 * sxy + C2)) / ((ux * ux + uy * uy + C1) * (sxx + syy + C2)))
    return float(np.mean(np.stack(vals)))


def reference(tokens, target, mean=MEAN, std=STD, delta=1.0, ssim=True):
    """float64 [8]: what one batch adds to zeroed accumulators (slot 7 stays 0 without ssim)."""
    gi, ti = _images(tokens, target)
    B, _, S, _ = gi.shape
    m = np.asarray(mean, dtype=np.float64).reshape(3, 1, 1)
    sd = np.asarray(std, dtype=np.float64).reshape(3, 1, 1)
    out = np.zeros(8)
    for b in range(B):
        out[0] += 1
        if not np.isfinite(gi[b]).all():
            out[1] += 1
            continue
        d = gi[b] - ti[b]
        ad = np.abs(d)
        out[2] += np.where(ad <= delta, 0.5 * d * d, delta * (ad - 0.5 * delta)).sum()
        out[3] += ad.sum()
        out[4] += (d * d).sum()
        out[5] += d.size
        px, py = np.clip(gi[b] * sd + m, 0.0, 1.0), np.clip(ti[b] * sd + m, 0.0, 1.0)
        mse = float(((px - py) ** 2).mean())
        out[6] += 10.0 * np.log10(1.0 / max(mse, 1e-10))
        if ssim:
            out[7] += ssim_image(px, py)
    return out


def allowance(tokens, target, ref, torch_fn, ssim=True, mean=MEAN, std=STD, delta=1.0):
    """(bound, yardstick) per slot: the yardstick is |torch_fn in fp32 - ref| on the same inputs, the bound 4 x that plus
    1e-6 of the slot's magnitude."""
    sums = torch.zeros(8, dtype=torch.float64)
    torch_fn(tokens.detach().cpu(), target.detach().cpu(), mean, std, delta, ssim, sums)
    yard = np.abs(sums.numpy() - ref)
    return 4.0 * yard + 1e-6 * np.abs(ref), yard


def errors(got, ref):
    got = np.asarray(got.detach().cpu() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    return np.abs(got - ref)


def mismatches(got, ref, bound, ssim=True):
    """Names of the slots that differ from the reference ([] when all agree): the integer-valued slots must be equal, the
    others within `bound`; a NaN never agrees."""
    err = errors(got, ref)
    bad = []
    for s, name in enumerate(SLOTS):
        if s == 7 and not ssim:
            continue
        ok = err[s] == 0.0 if s in EXACT else err[s] <= bound[s]
        if not ok:
            bad.append(f"{name}: error {err[s]:.3e} (bound {0.0 if s in EXACT else bound[s]:.3e}, value {ref[s]!r})")
    return bad


def regions(S):
    """(row slice, column slice) of the constant patch (top left, S // 2 wide) and of the two clamped regions (bottom
    left: above 1; bottom right: below 0; S // 4 wide) of every image of make_case."""
    h, q = max(S // 2, 1), max(S // 4, 1)
    return {"constant": (slice(0, h), slice(0, h)), "clamp_hi": (slice(S - q, S), slice(0, q)),
            "clamp_lo": (slice(S - q, S), slice(S - q, S))}


def crop(tokens, target, rows, cols):
    """The same region of both tensors as a case of its own: (tokens [B,h,3w], target [B,3,h,w]); square regions only."""
    gi = tokens.float().reshape(tokens.shape[0], tokens.shape[1], tokens.shape[1], 3)[:, rows, cols, :]
    ti = target if target.dim() == 4 else target.reshape(gi.shape[0], tokens.shape[1], tokens.shape[1], 3).permute(0, 3, 1, 2)
    return gi.reshape(gi.shape[0], gi.shape[1], -1).contiguous().to(tokens.dtype), ti[:, :, rows, cols].contiguous()


def make_case(B, S, layout="rows", dtype=torch.float32, seed=0, nonfinite=False):
    """(tokens [B,S,3S] of `dtype`, target fp32 in `layout` "rows" [B,S,3S] or "nchw" [B,3,S,S]), seeded, in normalised
    space.  The target is a smooth random field (a few low-frequency waves per channel) plus noise; the generated image
    is the target plus a smooth error and finer noise.  Every image holds a constant patch in both tensors (two different
    constants, neither a dyadic fraction: windows inside it have zero variance — the cancellation regime) and two regions
    far outside the pixel range (values around 4 / 5 and -4 / -3.5 with a little noise: both tensors clamp at 1, and at 0,
    there); `regions(S)` names the three.  Where B > 1, image 1 equals its target exactly (PSNR at its 100 dB cap, SSIM
    1) — except with nonfinite=True (B >= 3), where image 0 holds a NaN, image 2 an inf and image 1 stays ordinary."""
    rng = np.random.default_rng(7919 * B + 31 * S + seed)
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")

    def field(amp, waves, noise):
        f = np.zeros((B, 3, S, S))
        for b in range(B):
            for c in range(3):
                for _ in range(waves):
                    fy, fx = rng.uniform(0.02, 0.2, 2)
                    f[b, c] += amp * rng.uniform(0.3, 1.0) * np.sin(fy * yy + fx * xx + rng.uniform(0, 2 * np.pi))
        return f + noise * rng.standard_normal(f.shape)

    t = field(1.0, 3, 0.15)
    g = t + field(0.25, 2, 0.08)
    reg = regions(S)
    t[(..., *reg["constant"])], g[(..., *reg["constant"])] = 0.3, 0.41
    for name, tv, gv in (("clamp_hi", 4.0, 5.0), ("clamp_lo", -4.0, -3.5)):
        shape = t[(..., *reg[name])].shape
        t[(..., *reg[name])] = tv + 0.05 * rng.standard_normal(shape)
        g[(..., *reg[name])] = gv + 0.05 * rng.standard_normal(shape)
    tokens = torch.from_numpy(g.transpose(0, 2, 3, 1).reshape(B, S, 3 * S).copy()).to(torch.float32).to(dtype)
    ti = torch.from_numpy(t).to(torch.float32)
    if B > 1 and not nonfinite:
        ti[1] = tokens[1].float().reshape(S, S, 3).permute(2, 0, 1)  # (values the storage type holds exactly)
    if nonfinite:
        assert B >= 3
        tokens[0, S // 2, 5] = float("nan")
        tokens[2, 0, 0] = float("inf")
    target = ti.contiguous() if layout == "nchw" else ti.permute(0, 2, 3, 1).reshape(B, S, 3 * S).contiguous()
    return tokens, target


# ---- the rows Huber pair ----------------------------------------------------------------------------------------------------
HUBER_SIZES = [1, 3, 5, 4 * 48 * 144, 4 * 48 * 144 + 1]


def huber_case(n, seed=0):
    """(tokens, target) fp32 [n]: differences on both sides of delta = 1, some exactly 0."""
    g = torch.Generator().manual_seed(100 + n + seed)
    a = torch.randn(n, generator=g) * 1.5
    b = torch.randn(n, generator=g) * 0.5
    b[::7] = a[::7]
    return a, b


def huber_reference(a, b, delta=1.0):
    """(loss, dtokens for dloss = 1) in float64."""
    d = a.double() - b.double()
    ad = d.abs()
    loss = torch.where(ad <= delta, 0.5 * d * d, delta * (ad - 0.5 * delta)).mean()
    return float(loss), d.clamp(-delta, delta) / d.numel()
