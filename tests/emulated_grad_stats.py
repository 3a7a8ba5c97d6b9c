"""TEST INFRASTRUCTURE: calm_grad_stats (csrc/grad_stats.hip) emulated in fp32 torch in the kernel's own order — the
elements of a chunk dealt to 256 threads the way the single-word and the 16-byte paths deal them, a thread's serial sum,
the wave butterfly, the four wave sums added left to right, the tensor's chunks in chunk order, the single workgroup's
sticky update — and the planted faults the float64 checker (grad_stats_f64.py) must reject.  Products and sums are
separate fp32 operations here; where the compiler contracts them into an fma the kernel's error is the smaller one.

Which dealing a tensor gets here is a convention of the emulation alone — the 16-byte one when its gradient offset
(tail_f64's `goff`, in floats) is a multiple of 4 — so that both orders are emulated.  It does NOT mirror the path the
device takes for that tensor: the GPU tests' arenas put a tensor wherever the running sizes leave it, and the kernel
decides by the addresses.  The checker's bounds depend on the summation depth, which the two dealings share."""
import numpy as np
import torch

import tail_f64 as tf

NT, CHUNK = tf.OPT_NT, tf.OPT_CHUNK
SLOTS = CHUNK // NT + 1                    # a thread's 64 elements, and the one tail element of the 16-byte path
FAULTS = ("no_correction", "no_unscale", "expanded_norm", "span_off_by_one", "no_bias_correction", "nonfinite_to_neighbour",
          "not_sticky")
FMAX = 3.402823466e38


def _wave_sum(x):
    """x: [..., 64] -> the butterfly of wave_sum (every lane ends with the same value; lane 0 is taken)"""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lane ^ o]
    return x[..., 0]


def _block_sum(x):
    """x: [chunks, 256] -> block_sum_256"""
    w = _wave_sum(x.view(-1, 4, 64))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _serial(x):
    """x: [chunks, SLOTS, 256]: every thread adds its elements in slot order, starting from 0"""
    acc = torch.zeros(x.shape[0], NT, dtype=torch.float32)
    for k in range(x.shape[1]):
        acc = acc + x[:, k]
    return acc


def _deal(n, vector):
    """(slot, thread) of the elements 0 .. n-1 of a chunk"""
    j = np.arange(n)
    if not vector:
        return j // NT, j % NT
    v1 = n & ~3
    q = j // 4
    slot, thread = (q // NT) * 4 + j % 4, q % NT
    tail = j >= v1
    slot[tail], thread[tail] = SLOTS - 1, (j - v1)[tail]
    return slot, thread


class EmulatedGradStats:
    def __init__(self, table, fault=None):
        assert fault is None or fault in FAULTS
        self.table, self.fault = table, fault
        self.first, self.n_chunks = tf.optim_chunks(table)

    def _layout(self, per_tensor, vector_ok, short=0):
        """per_tensor: one flat fp32 tensor per table entry -> [n_chunks, SLOTS, 256], zero where no element sits"""
        out = torch.zeros(self.n_chunks, SLOTS, NT, dtype=torch.float32)
        for e, c0, x in zip(self.table, self.first, per_tensor):
            for k in range(tf.cdiv(e["numel"], CHUNK)):
                i0 = k * CHUNK
                i1 = min(i0 + CHUNK, e["numel"]) - short
                if i1 <= i0:
                    continue
                slot, thread = _deal(i1 - i0, vector_ok and e["goff"] % 4 == 0)
                out[c0 + k, slot, thread] = x[i0:i1]
        return out

    def call(self, recs, grads, hp, grad_scale, step, out, summary):
        """One calm_grad_stats call: `out` (numpy record array) and `summary` (four ints) are updated in place."""
        fault = self.fault
        f = lambda x: torch.tensor(float(x), dtype=torch.float32)            # noqa: E731
        b1, b2, eps = f(hp[1]), f(hp[2]), f(hp[3])
        inv = f(1.0) / f(grad_scale) if grad_scale is not None and fault != "no_unscale" else f(1.0)
        short = 1 if fault == "span_off_by_one" else 0
        n = len(self.table)
        sn = [r["sn"] is not None for r in recs]
        ones = lambda e: torch.ones(e["numel"])                               # noqa: E731
        G = [g.float().reshape(-1) for g in grads]
        P = [r["param"].reshape(-1) for r in recs]
        Uu = [r["sn"][0].repeat_interleave(r["sn"][4]) if s else ones(e) for r, s, e in zip(recs, sn, self.table)]
        Vv = [r["sn"][1].repeat(r["sn"][3]) if s else ones(e) for r, s, e in zip(recs, sn, self.table)]
        # pass 1: <G, W_orig> per chunk in the single-word order, then c per tensor in chunk order
        gw = _block_sum(_serial(self._layout(G, False) * self._layout(P, False)))
        c, inv_sg = torch.zeros(n), torch.ones(n)
        for t, r in enumerate(recs):
            if sn[t]:
                acc = torch.zeros(())
                for k in range(tf.cdiv(self.table[t]["numel"], CHUNK)):
                    acc = acc + gw[self.first[t] + k]
                sg = r["sn"][2].reshape(())
                c[t], inv_sg[t] = acc / sg, 1.0 / sg
        chunk_t = torch.tensor([t for t, e in enumerate(self.table) for _ in range(tf.cdiv(e["numel"], CHUNK))])
        cc, isg, is_sn = c[chunk_t][:, None, None], inv_sg[chunk_t][:, None, None], torch.tensor(sn)[chunk_t][:, None, None]
        # pass 2
        g, p = self._layout(G, True, short), self._layout(P, True, short)
        here = self._layout([ones(e) for e in self.table], True, short) > 0
        corr = (g - cc * self._layout(Uu, True, short) * self._layout(Vv, True, short)) * isg
        if fault == "no_correction":
            corr = g * isg
        x = torch.where(is_sn, corr, g) * inv
        ok = here & (x.abs() <= FMAX)
        x = torch.where(ok, x, torch.zeros(()))
        g2 = _block_sum(_serial(x * x))
        gmax = x.abs().amax(dim=(1, 2))
        p2 = _block_sum(_serial(p * p))
        pmax = p.abs().amax(dim=(1, 2))
        bad = (here & ~(g.abs() <= FMAX)).sum(dim=(1, 2))
        d2 = torch.zeros(self.n_chunks)
        if step >= 1:
            bc1, bc2 = 1.0 - torch.pow(b1, float(step)), 1.0 - torch.pow(b2, float(step))
            if fault == "no_bias_correction":
                bc1, bc2 = f(1.0), f(1.0)
            m = self._layout([r["exp_avg"].reshape(-1) for r in recs], True, short)
            v = self._layout([r["exp_avg_sq"].reshape(-1) for r in recs], True, short)
            d = (1.0 / bc1) * (m / (v.sqrt() * (1.0 / bc2.sqrt()) + eps))
            d2 = _block_sum(_serial(d * d))
        if fault == "expanded_norm":
            # optim_finalize's form for the spectral-norm tensors: (|G|^2 - 2 c u^T G v + c^2 |u|^2 |v|^2) / sigma^2
            gr, ur, vr = self._layout(G, False), self._layout(Uu, False), self._layout(Vv, False)
            s2, guv = _block_sum(_serial(gr * gr)), _block_sum(_serial(gr * ur * vr))
        # pass 3
        call = int(summary[0])
        first = -1
        for t, e in enumerate(self.table):
            acc = dict(g2=torch.zeros(()), p2=torch.zeros(()), d2=torch.zeros(()), s2=torch.zeros(()), guv=torch.zeros(()))
            gm = pm = 0.0
            nbad = 0
            for k in range(tf.cdiv(e["numel"], CHUNK)):
                ch = self.first[t] + k
                acc["g2"], acc["p2"], acc["d2"] = acc["g2"] + g2[ch], acc["p2"] + p2[ch], acc["d2"] + d2[ch]
                gm, pm = max(gm, float(gmax[ch])), max(pm, float(pmax[ch]))
                nbad += int(bad[ch])
                if fault == "expanded_norm":
                    acc["s2"], acc["guv"] = acc["s2"] + s2[ch], acc["guv"] + guv[ch]
            if fault == "expanded_norm" and sn[t]:
                u, v, sg = recs[t]["sn"][0], recs[t]["sn"][1], recs[t]["sn"][2].reshape(())
                n2 = (acc["s2"] - 2.0 * c[t] * acc["guv"] + c[t] * c[t] * (u * u).sum() * (v * v).sum()) / (sg * sg)
                acc["g2"] = n2.clamp_min(0.0) * inv * inv
            tgt = out[(t + 1) % n] if fault == "nonfinite_to_neighbour" else out[t]
            o = out[t]
            o["grad_sq"], o["grad_absmax"], o["param_sq"], o["param_absmax"] = float(acc["g2"]), gm, float(acc["p2"]), pm
            o["dir_sq"] = float(acc["d2"])
            if fault != "nonfinite_to_neighbour":
                o["nonfinite"] = nbad
            else:                                           # the count lands in the next tensor's record
                if t == 0:
                    out["nonfinite"] = 0
                if nbad:
                    tgt["nonfinite"] = nbad
            if fault == "not_sticky" and not nbad:
                o["bad_calls"], o["first_bad_call"] = 0, -1
            if nbad:
                tgt["bad_calls"] += 1
                if tgt["first_bad_call"] < 0:
                    tgt["first_bad_call"] = call
                if first < 0:
                    first = (t + 1) % n if fault == "nonfinite_to_neighbour" else t
        summary[0] = call + 1
        if first >= 0:
            summary[1] += 1
            if summary[2] < 0:
                summary[2], summary[3] = call, first
