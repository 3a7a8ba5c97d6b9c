"""CPU emulation of the three entry points of csrc/recon.hip on top of tests/emulated_eval.py — used by tests/test_recon_*.py
only.  It is never imported by the package.

It mirrors the kernels' formulation in fp32 numpy: the rows Huber pair element by element; calm_recon_metrics band by band
(recon_band_rows output rows per band, ten halo rows, the last band owning the rows to S), pixel space shifted by 1/2, the
separable window — vertical, then horizontal — over the five fields x, y, x^2, y^2, xy, E[a^2] - E[a]^2 moments, one fp32
record per band, and the fold of the records in float64 in image order.  `recon_fault` plants a defect for the tests that
check the checker (tests/recon_f64.py):
    "unnormalised"   the window weights are not divided by their sum
    "bessel"         variances and covariance carry an n / (n - 1) factor with n = 121
    "halo_row"       a band stops one row short of its halo: its last output row is lost
    "channel_swap"   mean / std of channels 0 and 2 are exchanged
    "nonfinite_leak" a non-finite image is added to the sums like any other"""
import numpy as np
import torch

from emulated_eval import EmulatedEvalBackend
from emulated_loss import EmulatedLossBackend

WIN = 11
f32 = np.float32


def band_rows(S):
    v = S - (WIN - 1) if S > WIN - 1 else 1
    return 32 if v >= 128 else 16 if v >= 48 else 4


def bands(S):
    v = S - (WIN - 1) if S > WIN - 1 else 1
    return (v + band_rows(S) - 1) // band_rows(S)


def strips(S):
    v = S - (WIN - 1) if S > WIN - 1 else 1
    return (v + 245) // 246


def scratch_floats(B, S):
    return 8 * B * bands(S) * strips(S)


def window1d(fault=None):
    k = np.arange(WIN, dtype=np.float64) - (WIN - 1) / 2
    w = np.exp(-k * k / (2.0 * 1.5 ** 2))
    return (w if fault == "unnormalised" else w / w.sum()).astype(f32)


def huber_value(d, delta):
    ad = np.abs(d)
    return np.where(ad <= delta, f32(0.5) * d * d, f32(delta) * (ad - f32(0.5 * delta))).astype(f32)


def emu_records(tokens, target, mean, std, delta, want_ssim, fault=None):
    """float32 [B, bands, 8]: {huber, abs, sq, pixel sq, ssim, non-finite flag, 0, 0} per band (one strip: S <= 256)."""
    g = tokens.detach().float().cpu().numpy()
    B, S = g.shape[0], g.shape[1]
    assert S <= 256, "the emulation keeps one strip per band"
    gi = g.reshape(B, S, S, 3)                                        # channels last, as the kernel walks it
    t = target.detach().float().cpu().numpy()
    ti = t.transpose(0, 2, 3, 1) if t.ndim == 4 else t.reshape(B, S, S, 3)
    m, sd = np.asarray(mean, f32), np.asarray(std, f32)
    if fault == "channel_swap":
        m, sd = m[::-1].copy(), sd[::-1].copy()
    w = window1d(fault)
    R, nb = band_rows(S), bands(S)
    rec = np.zeros((B, nb, 8), f32)
    with np.errstate(all="ignore"):
        for b in range(B):
            xp = np.clip(gi[b] * sd + m, f32(0), f32(1)).astype(f32)
            yp = np.clip(ti[b] * sd + m, f32(0), f32(1)).astype(f32)
            for k in range(nb):
                r0 = k * R
                own_end = S if k == nb - 1 else r0 + R
                d = gi[b, r0:own_end] - ti[b, r0:own_end]
                pd = xp[r0:own_end] - yp[r0:own_end]
                rec[b, k, 0] = huber_value(d, delta).sum(dtype=f32)
                rec[b, k, 1] = np.abs(d).sum(dtype=f32)
                rec[b, k, 2] = (d * d).sum(dtype=f32)
                rec[b, k, 3] = (pd * pd).sum(dtype=f32)
                rec[b, k, 5] = f32(np.count_nonzero(~np.isfinite(gi[b, r0:own_end])))
                if not want_ssim:
                    continue
                row_end = min(r0 + R + WIN - 1, S) - (1 if fault == "halo_row" else 0)
                a, y = xp[r0:row_end] - f32(0.5), yp[r0:row_end] - f32(0.5)
                n_out = a.shape[0] - (WIN - 1)
                if n_out <= 0:
                    continue
                fields = [a, y, a * a, y * y, a * y]
                vert = [sum(w[j] * f[j:j + n_out] for j in range(WIN)).astype(f32) for f in fields]      # [n_out, S, 3]
                mom = [sum(w[j] * v[:, j:j + S - (WIN - 1)] for j in range(WIN)).astype(f32) for v in vert]
                mx, my = mom[0], mom[1]
                sxx, syy, sxy = mom[2] - mx * mx, mom[3] - my * my, mom[4] - mx * my
                if fault == "bessel":
                    sxx, syy, sxy = (v * f32(121.0 / 120.0) for v in (sxx, syy, sxy))
                ux, uy = mx + f32(0.5), my + f32(0.5)
                C1, C2 = f32(0.01) * f32(0.01), f32(0.03) * f32(0.03)
                smap = ((2 * ux * uy + C1) * (2 * sxy + C2)) / ((ux * ux + uy * uy + C1) * (sxx + syy + C2))
                rec[b, k, 4] = smap.sum(dtype=f32)
    return rec


def emu_fold(rec, sums, S, want_ssim, fault=None):
    B = rec.shape[0]
    elems = 3.0 * S * S
    valid = float(S - (WIN - 1) if S > WIN - 1 else 1)
    out = sums.numpy()
    with np.errstate(all="ignore"):
        for b in range(B):
            tot = rec[b].astype(np.float64).sum(axis=0)
            out[0] += 1
            finite = tot[5] == 0.0
            if not finite:
                out[1] += 1
                if fault != "nonfinite_leak":
                    continue
            mse = tot[3] / elems
            out[2] += tot[0]
            out[3] += tot[1]
            out[4] += tot[2]
            out[5] += elems
            out[6] += 10.0 * np.log10(1.0 / (mse if mse > 1e-10 or mse != mse else 1e-10))
            if want_ssim:
                out[7] += tot[4] / (3.0 * valid * valid)


def _fail(name, code):
    raise RuntimeError(f"{name} failed: code {code} (invalid argument/unsupported shape)")


class ReconMixin:
    """huber_rows_fwd / _bwd, recon_metrics and recon_scratch_floats with HipBackend's signatures (and the library's
    refusals) over CPU tensors."""
    recon_fault = None

    def huber_rows_fwd(self, tokens, target, delta, loss, n):
        if n <= 0 or tokens.numel() != n or target.numel() != n or tokens.dtype != torch.float32:
            _fail("calm_recon_huber_rows_fwd", -1)
        if n >= 1 << 31:
            _fail("calm_recon_huber_rows_fwd", -3)
        self.huber_rows_calls = getattr(self, "huber_rows_calls", 0) + 1
        d = tokens.detach().reshape(-1).numpy() - target.detach().reshape(-1).numpy()
        loss.copy_(torch.tensor(float(huber_value(d, delta).sum(dtype=f32) * f32(1.0 / n))))

    def huber_rows_bwd(self, tokens, target, delta, dloss, dtokens, n):
        if n <= 0 or tokens.numel() != n or target.numel() != n or dtokens.numel() != n:
            _fail("calm_recon_huber_rows_bwd", -1)
        d = tokens.detach() - target.detach()
        dtokens.copy_((dloss.reshape(()) / float(n)) * d.clamp(-delta, delta))

    def recon_scratch_floats(self, B, S):
        return scratch_floats(B, S)

    def recon_metrics(self, tokens, target, layout, mean, std, delta, want_ssim, sums, B, S, partials=None):
        if tokens.dtype not in (torch.float32, torch.bfloat16) or layout not in (0, 1) or B <= 0 or S <= 0:
            _fail("calm_recon_metrics", -1)
        if S > 4096 or (want_ssim and S < WIN):
            _fail("calm_recon_metrics", -3)
        if sums.dtype != torch.float64 or sums.numel() < 8:
            raise TypeError("recon_metrics expects a contiguous float64 tensor of 8 values for sums")
        if tuple(tokens.shape) != (B, S, 3 * S) or tuple(target.shape) != ((B, 3, S, S) if layout == 1 else (B, S, 3 * S)):
            raise ValueError("recon_metrics: contiguous tokens [B,S,3S] and a target of as many elements expected")
        if partials is not None and partials.numel() < scratch_floats(B, S):
            raise ValueError("recon_metrics: partials is smaller than calm_reduce_scratch_floats(CALM_RED_RECON, B, S)")
        self.recon_calls = getattr(self, "recon_calls", 0) + 1
        emu_fold(emu_records(tokens, target, mean, std, delta, want_ssim, self.recon_fault), sums, S, want_ssim,
                 self.recon_fault)


class EmulatedReconBackend(ReconMixin, EmulatedEvalBackend):
    """The emulated C-ABI with the reconstruction entry points: what train(task="reg", val_dataset=..., ema=...) needs on a
    host without a GPU."""
    name = "emulated+recon"
    _diff = staticmethod(EmulatedLossBackend._diff)                  # the image-layout Huber pair of the 4-d path
    huber_tokens_fwd = EmulatedLossBackend.huber_tokens_fwd
    huber_tokens_bwd = EmulatedLossBackend.huber_tokens_bwd
