"""TEST INFRASTRUCTURE: calm_sam_perturb / calm_sam_restore (csrc/sam.hip) emulated in fp32 torch in the header's operation
and summation order, over tail_f64's records — <G, W_orig> per chunk in the single-word dealing and then in chunk order,
the elements' s in the header's order of operations, s^2 summed by a thread's serial run, the wave butterfly, the four wave
sums left to right, the tensor's chunks in chunk order, then the tensors dealt to 256 running sums (tensor k, k + 256, ...)
and the block sum — and the planted faults the float64 checker (sam_f64.py) must reject, each one changed line.  Products
and sums are separate fp32 operations here; where the compiler contracts them into an fma the kernel's error is the smaller.

The dealing of a chunk's elements (single words or 16-byte vectors) is emulated_grad_stats' convention: the 16-byte one
when the tensor's gradient offset (tail_f64's `goff`) is a multiple of 4.  It does not mirror the path the device takes."""
import torch

import tail_f64 as tf
from emulated_grad_stats import EmulatedGradStats, _block_sum, _serial

NT, CHUNK = tf.OPT_NT, tf.OPT_CHUNK
FAULTS = ("no_correction", "uv_transposed", "norm_per_tensor", "scale_in_norm_only", "adaptive_without_eta", "adaptive_t_once",
          "last_partial_chunk", "applied_despite_nonfinite", "restore_by_subtraction")
FMAX = 3.402823466e38


def _f(x):
    return torch.tensor(float(x), dtype=torch.float32)


class EmulatedSam:
    def __init__(self, table, fault=None):
        assert fault is None or fault in FAULTS
        self.table, self.fault = table, fault
        self.first, self.n_chunks = tf.optim_chunks(table)
        self._layout = EmulatedGradStats(table)._layout
        self._step = None

    def _per_tensor(self, chunk_values):
        """a tensor's chunk values added in chunk order -> [n_tensors]"""
        out = torch.zeros(len(self.table), dtype=torch.float32)
        for t, e in enumerate(self.table):
            acc = torch.zeros((), dtype=torch.float32)
            for k in range(tf.cdiv(e["numel"], CHUNK)):
                acc = acc + chunk_values[self.first[t] + k]
            out[t] = acc
        return out

    def perturb(self, recs, grads, hp, grad_scale):
        """One calm_sam_perturb call; hp = (rho, eps, eta, adaptive).  -> dict(norm, found_inf, scale: floats; backup,
        p_after: one flat fp32 tensor per record).  recs are not modified."""
        fault = self.fault
        rho, eps, eta, adaptive = _f(hp[0]), _f(hp[1]), _f(hp[2]), bool(hp[3])
        inv = _f(1.0) / _f(grad_scale) if grad_scale is not None else _f(1.0)
        n = len(self.table)
        G = [g.float().reshape(-1) for g in grads]
        P = [r["param"].reshape(-1) for r in recs]
        # pass 1: <G, W_orig> per chunk in the single-word order, then c per tensor in chunk order
        gw = self._per_tensor(_block_sum(_serial(self._layout(G, False) * self._layout(P, False))))
        S, T = [], []
        for t, (r, g, p) in enumerate(zip(recs, G, P)):
            x = g
            if r["sn"] is not None:
                u, v, sigma, rows, cols = r["sn"]
                sg = sigma.reshape(())
                c, inv_sg = gw[t] / sg, 1.0 / sg
                uu, vv = u.repeat_interleave(cols), v.repeat(rows)
                if fault == "uv_transposed":
                    i = torch.arange(rows * cols)
                    uu, vv = u[i % rows], v[i // rows]
                x = (g - c * uu * vv) * inv_sg
                if fault == "no_correction":
                    x = g * inv_sg
            x = x * inv
            tt = p.abs() + (eta if fault != "adaptive_without_eta" else 0.0) if adaptive else torch.ones(())
            S.append(tt * x if adaptive else x)
            T.append(tt)
        # pass 2 and 3: s^2 per chunk, per tensor in chunk order, the tensors in 256 running sums, the block sum
        n2 = self._per_tensor(_block_sum(_serial(self._layout([s * s for s in S], True))))
        run = torch.zeros(1, NT, dtype=torch.float32)
        for t in range(n):
            run[0, t % NT] = run[0, t % NT] + n2[t]
        norm = torch.sqrt(_block_sum(run)[0])
        bad = any(not bool((g.abs() <= FMAX).all()) for g in G) or not bool(norm.abs() <= FMAX)
        scale = _f(0.0) if bad else rho / (norm + eps)
        apply_scale = rho / (norm + eps) if fault == "applied_despite_nonfinite" else scale
        after, self._step = [], []
        for t, (p, s, tt) in enumerate(zip(P, S, T)):
            sc = rho / (torch.sqrt(n2[t]) + eps) if fault == "norm_per_tensor" else apply_scale
            if fault == "scale_in_norm_only":
                s = s / inv
            step = (sc * tt) * s if adaptive and fault != "adaptive_t_once" else sc * s
            if fault == "last_partial_chunk" and p.numel() > CHUNK and p.numel() % CHUNK:
                step = step.clone()
                step[p.numel() - p.numel() % CHUNK:] = 0.0
            untouched = bad and fault != "applied_despite_nonfinite"          # found_inf: no parameter is written
            after.append(p.clone() if untouched else p + step)
            self._step.append(step)
        return dict(norm=float(norm), found_inf=float(bad), scale=float(scale), backup=[p.clone() for p in P], p_after=after)

    def restore(self, p_after, backup):
        """calm_sam_restore -> the parameters after it (one flat tensor per record)"""
        if self.fault == "restore_by_subtraction":
            return [w - e for w, e in zip(p_after, self._step)]
        return [b.clone() for b in backup]
