"""EmulatedBackend with the gradient-tail calls of the HIP backend (the *_part producers, reduce_partials_batch,
sn_weight_bwd_batch) in plain torch, and a log of what was called in which order.

A producer's partial form writes ONE row of partials (G = 1): the sum the full form would have added to its output,
computed by that full form into zeros.  reduce_partials_batch then adds the row to the outputs — 0 + s = s exactly, so a
deferred gradient equals the immediate one in every bit and the tests can compare with torch.equal."""
from types import SimpleNamespace

import torch

from emulated_backend import EmulatedBackend

CNN_SIZES = lambda ch: [3 * ch, ch, 9 * ch, ch, 3 * ch, 3]      # noqa: E731  (g0 | gb0 | g2 | gb2 | g4 | gb4)


def _shape(sizes):
    begin = [0]
    for n in sizes:
        begin.append(begin[-1] + n)
    return SimpleNamespace(G=1, n=begin[-1], stride=begin[-1], nseg=len(sizes), begin=begin)


class TailBackend(EmulatedBackend):
    def __init__(self):
        super().__init__()
        self.log = []                 # ("part", kind, id of the partials) / ("reduce", [ids]) / ("sn", [ids of G])

    def _part(self, kind, sizes, like):
        part = torch.zeros(sum(sizes), dtype=torch.float32, device=like.device)
        self.log.append(("part", kind, id(part)))
        return part, _shape(sizes)

    def layernorm_bwd_part(self, dy, x, w, mean, rstd, dx, rows, D, dx_add=None):
        part, shape = self._part("layernorm", [D], x)
        self.layernorm_bwd(dy, x, w, mean, rstd, dx, part, rows, D, dx_add=dx_add)
        return part, shape

    def rope_bwd_part(self, d_out, xr, table, d_content, d_xr, B, S, H, dc, dr):
        part, shape = self._part("rope", [dr // 2], xr)
        self.rope_bwd(d_out, xr, table, d_content, d_xr, part, B, S, H, dc, dr)
        return part, shape

    def colsum_part(self, x, rows, cols):
        part, shape = self._part("colsum", [cols], x)
        self.colsum(x, part, rows, cols)
        return part, shape

    def cnn_bwd_part(self, dy, x, w0, s0, b0, w2, s2, b2, w4, s4, b4, dx, B, S, hidden, residual=True):
        part, shape = self._part("cnn", CNN_SIZES(hidden), dy)
        self.cnn_bwd(dy, x, w0, s0, b0, w2, s2, b2, w4, s4, b4, dx, *torch.split(part, CNN_SIZES(hidden)), B, S, hidden,
                     residual=residual)
        return part, shape

    def reduce_partials_batch(self, items):
        self.log.append(("reduce", [id(part) for part, _, _ in items]))
        for part, shape, outs in items:
            assert len(outs) == shape.nseg
            for k, o in enumerate(outs):
                o.view(-1).add_(part[shape.begin[k]:shape.begin[k + 1]])

    def sn_weight_bwd_batch(self, items):
        self.log.append(("sn", [id(it[0]) for it in items]))
        for it in items:
            self.sn_weight_bwd(*it)
