#!/usr/bin/env python3
"""Mint the dropout block fixtures from the REFERENCE implementation (build container only; see make_golden.py).

The reference's VMLA_Block is built with dropout > 0 and run in train() mode with torch.nn.functional.dropout replaced by
`input * multiplier`, the multiplier (1 / (1 - p) where kept, 0 where dropped) coming from the Philox rule of
csrc/dropout.hip (tests/emulated_dropout.py): flat index over the contiguous tensor, key (seed, index of the call within
the forward) — the attention site is call 0, the MLP site call 1 (Vi_Tools_CNN_less_V2.py:301, 203).  Recipe as
make_golden.mint_block: numpy-seeded weights, 5 train-mode warm-up forwards (noise and dropout active), then a train
forward with injected noise and keys and the backward of sum(y * gy) + 0.5 * kl.  Only DATA is written
(golden_block_drop_<name>.npz).  Run:  python tests/golden/make_golden_dropout.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import weights as W  # noqa: E402
from emulated_dropout import multiplier  # noqa: E402
from make_golden import BLOCK_WEIGHT_SEED, FULL_GRAD_MAX_REAL, import_reference, kl_value, run_with_noise  # noqa: E402

# kwargs of the reference's VMLA_Block (+ p, batch): (A) a plain self-attention block, (B) the reducing cross block of the
# Nano-48 stage geometry (sequence 48 -> 16 -> 36, features 144 -> 24 -> 108)
DROPOUT_BLOCKS = {
    "A": dict(kw=dict(heads=4, dim1=96, dim2=96, mean_var_hidden=24, seq_length=32, seq_len_reduce=16, seq_len_new=32,
                      is_cross=False), p=0.25, batch=2),
    "B": dict(kw=dict(heads=3, dim1=144, dim2=108, mean_var_hidden=24, seq_length=48, seq_len_reduce=16, seq_len_new=36,
                      is_cross=True), p=0.1, batch=2),
}
KEY_SEED = 0x5EED0D20                     # the captured forward; warm-up forward i uses KEY_SEED + 1 + i
NOISE_SEED = 9


class PhiloxDropout:
    """Stand-in for torch.nn.functional.dropout: the i-th call of a forward multiplies by the mask of key (seed, i)."""

    def __init__(self, seed):
        self.seed = seed
        self.n = 0

    def __call__(self, input, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return input
        m = multiplier((self.seed, self.n), 0, input.numel(), p).view(input.shape)
        self.n += 1
        return input.contiguous() * m


def run_with_dropout(fn, seed):
    orig = torch.nn.functional.dropout
    torch.nn.functional.dropout = PhiloxDropout(seed)
    try:
        return fn()
    finally:
        torch.nn.functional.dropout = orig


def mint_dropout_block(name, spec, vtools):
    kw, p, B = spec["kw"], spec["p"], spec["batch"]
    blk = vtools.VMLA_Block(mlp_dim=2 * kw["dim2"], force_reduce=False, dropout=p, **kw)
    shapes = {k: list(v.shape) for k, v in blk.state_dict().items()}
    blk.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_params(shapes, BLOCK_WEIGHT_SEED).items()})
    S, D1, cross = kw["seq_length"], kw["dim1"], kw["is_cross"]
    xq = torch.from_numpy(W.make_input((B, S, D1), 5, "xq"))
    xkv = torch.from_numpy(W.make_input((B, S, D1), 6, "xkv")) if cross else None
    call = lambda a, b, sm: blk(a, input_kv=b, state_manager=sm, mask=True)
    blk.train()
    for i in range(5):
        with torch.no_grad():
            run_with_dropout(lambda: run_with_noise(
                lambda: call(xq, xkv, vtools.ResidualStateManager(mode="sum")), 50 + i), KEY_SEED + 1 + i)
    out = {"shape_names": np.array(sorted(shapes)), "p": np.float32(p)}
    for k in sorted(shapes):
        out["shape/" + k] = np.array(shapes[k], dtype=np.int64)
    for k, v in blk.state_dict().items():
        if k.endswith(("weight_u", "weight_v")):
            out["warm/" + k] = v.detach().numpy().copy()
    xq = xq.clone().requires_grad_(True)
    xkv = xkv.clone().requires_grad_(True) if cross else None
    sm = vtools.ResidualStateManager(mode="sum")
    y = run_with_dropout(lambda: run_with_noise(lambda: call(xq, xkv, sm), NOISE_SEED), KEY_SEED)
    gy = torch.from_numpy(W.make_input(tuple(y.shape), 8, "gy"))
    kl = sm.get_kl_loss()
    loss = (y * gy).sum() + 0.5 * kl
    loss.backward()
    out["y"] = y.detach().numpy().copy()
    out["kl"] = kl_value(kl)
    out["loss"] = np.float32(loss.item())
    out["dxq"] = xq.grad.numpy().copy()
    if cross:
        out["dxkv"] = xkv.grad.numpy().copy()
    names, norms = [], []
    for k, prm in blk.named_parameters():
        names.append(k)
        norms.append(float(prm.grad.norm()))
        if prm.numel() <= FULL_GRAD_MAX_REAL:
            out["grad/" + k] = prm.grad.numpy().copy()
    out["grad_names"] = np.array(names)
    out["grad_norms"] = np.array(norms, dtype=np.float32)
    for k, v in blk.state_dict().items():
        if k.endswith(("weight_u", "weight_v")):
            out["post/" + k] = v.detach().numpy().copy()
    np.savez_compressed(os.path.join(HERE, f"golden_block_drop_{name}.npz"), **out)
    print("dropout block", name, "p", p, "loss", out["loss"], "kl", out["kl"], "|y|max", float(np.abs(out["y"]).max()),
          "zeros in y", int((out["y"] == 0).sum()))


def main():
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", "4")))
    import_reference()
    import Vi_Tools_CNN_less_V2 as vtools          # the reference's module (make_golden.REF is on sys.path)
    only = set(sys.argv[1:])
    for name, spec in DROPOUT_BLOCKS.items():
        if not only or name in only:
            mint_dropout_block(name, spec, vtools)


if __name__ == "__main__":
    main()
