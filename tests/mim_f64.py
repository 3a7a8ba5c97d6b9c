"""The checker of the masked-image-modelling entry points (calm_mim_draw / _apply / _huber_fwd / _huber_bwd): references
written from the formulas of include/calm_vit.h — the mask by COUNTING compares over the numpy Philox words, the element
decisions by index arithmetic, the loss pair in float64 — the cases, and the bounds.  Shared by tests/test_mim_cpu.py (on
the emulation, on its planted faults and on trainer.mim_huber_torch) and tests/test_mim_gpu.py (on the kernels).

An implementation under test is an object with
    draw(B, G, k, key, sample0)                                     -> uint8 [B, G * G]
    apply(x, mask, fill, p, in_place, lead)                         -> y [B,S,3S]
    huber(tokens, target, mask, delta, dloss, p, masked, lead)      -> (loss 0-dim, dtokens [B,S,3S])
over CPU tensors in and out; `lead` asks for tensor bases that many floats behind a 16-byte boundary (the emulation has no
addresses and ignores it), `in_place` for y = x.

Bounds:
  mask, apply          exact (bytes; bits);
  loss                 |got - ref| <= 1e-4 * ref — a sum of non-negative terms, so a relative bound is meaningful;
  dtokens              helpers.rel_err <= 1e-4, the project's fp32 kernel bound (TOL of tests/bce_f64.py), and exactly +0.0
                       wherever the mask is not set;
  NaN                  planted at an unmasked position of tokens / target: loss and dtokens keep their bits; planted at a
                       masked position: the loss and that element of dtokens are NaN."""
import numpy as np
import torch

from emulated_dropout import dropout_words
from helpers import rel_err

TOL = 1e-4
SEED, OFFSET, SAMPLE0 = 0x0123456789ABCDEF, (1 << 32) + 7, (1 << 34) + 3        # those of tests/test_drop_path_cpu.py
KEY = (SEED, OFFSET)
# (B, S, p, k)
DRAW_CASES = [(3, 8, 4, 2), (5, 12, 3, 8), (2, 9, 3, 4), (4, 224, 32, 29), (3, 224, 16, 118), (2, 32, 1, 614), (1, 224, 7, 1),
              (1, 224, 7, 1023)]
# Under KEY at G = 32: (sample, lower patch, higher patch, sorted position of the higher one) — the two patches hold the same
# word, at sorted positions pos - 1 and pos.  Found with the emulation; tests/test_mim_cpu.py asserts the ties themselves.
TIES = [(3436, 804, 870, 723), (4491, 47, 213, 259)]
# (B, S, p): one vector per patch row; vectors straddle patch edges (3p = 9); 3p = 18; rows off 16 bytes (3S = 30); 3 B S^2 %
# 4 == 3; the training shapes
HUBER_CASES = [(3, 8, 4), (2, 12, 3), (2, 24, 6), (3, 10, 5), (1, 9, 3), (2, 224, 32), (2, 224, 16), (1, 224, 7)]
FILL = (0.25, -0.5, 1.5)


def ratio_k(P, ratio=0.6):
    return min(P - 1, max(1, int(np.floor(ratio * P + 0.5))))


# ---- references ---------------------------------------------------------------------------------------------------------
def ref_words(key, sample, P):
    return dropout_words(int(key[0]), int(key[1]), sample * 1024, P)


def ref_mask(key, sample0, B, G, k):
    """uint8 numpy [B, P] from the definition: rank(i) = #{j : w_j < w_i, or w_j == w_i and j < i}; mask = rank < k."""
    P = G * G
    out = np.zeros((B, P), np.uint8)
    idx = np.arange(P)
    for b in range(B):
        w = ref_words(key, sample0 + b, P).astype(np.int64)
        before = (w[None, :] < w[:, None]) | ((w[None, :] == w[:, None]) & (idx[None, :] < idx[:, None]))
        out[b] = before.sum(axis=1) < k
    return out


def ref_element_mask(mask, S, p):
    """bool numpy [B, S, 3S]: element (b, r, 3x + c) belongs to patch (r // p) * G + x // p."""
    mask = np.asarray(mask)
    G = S // p
    r = np.arange(S)[:, None]
    x = (np.arange(3 * S) // 3)[None, :]
    return mask[:, (r // p) * G + x // p] != 0


def ref_apply(x, mask, fill, p):
    B, S, _ = x.shape
    m = torch.from_numpy(ref_element_mask(mask, S, p))
    f = torch.tensor(fill, dtype=torch.float32)[torch.arange(3 * S) % 3]
    return torch.where(m, f.expand(B, S, 3 * S), x)


def ref_huber(tokens, target, mask, delta, dloss, p, masked):
    """(loss, dtokens) in float64."""
    B, S, _ = tokens.shape
    m = torch.from_numpy(ref_element_mask(mask, S, p))
    n = 3.0 * p * p * masked
    d = tokens.double() - target.double()
    ad = d.abs()
    h = torch.where(ad <= delta, 0.5 * d * d, delta * (ad - 0.5 * delta))
    loss = h[m].sum() / n
    g = torch.where(m, float(dloss) / n * d.clamp(-delta, delta), torch.zeros((), dtype=torch.float64))
    return loss, g


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def inputs(B, S, seed=0):
    """tokens, target fp32 [B,S,3S]: differences of either sign on both sides of delta = 0.5 and 1."""
    g = torch.Generator().manual_seed(seed + 7919 * B + S)
    return torch.randn(B, S, 3 * S, generator=g), torch.randn(B, S, 3 * S, generator=g) * 0.5


def masks(B, S, p):
    """name -> uint8 [B, P]: the drawn mask at ratio 0.6, a hand-made uneven one (another count in every sample), one patch,
    all patches."""
    G = S // p
    P = G * G
    g = torch.Generator().manual_seed(31 * B + S + p)
    uneven = (torch.rand(B, P, generator=g) < torch.linspace(0.2, 0.9, B)[:, None]).to(torch.uint8)
    uneven[0, P // 2] = 1                                            # (never empty)
    if P > 1:
        uneven[0, P // 2 - 1] = 0                                    # (never full)
    one = torch.zeros(B, P, dtype=torch.uint8)
    one[B - 1, P - 2 if P > 1 else 0] = 1
    out = {"drawn": torch.from_numpy(ref_mask(KEY, SAMPLE0, B, G, ratio_k(P))), "uneven": uneven, "one": one,
           "all": torch.ones(B, P, dtype=torch.uint8)}
    if P == 1:
        del out["uneven"]
    return out


# ---- checks: each returns the list of complaints (empty: everything is within its bound) ------------------------------------
def check_draw(impl, cases=DRAW_CASES, ties=True):
    out = []
    for B, S, p, k in cases:
        G = S // p
        for sample0 in (0, SAMPLE0):
            got = impl.draw(B, G, k, KEY, sample0)
            ref = ref_mask(KEY, sample0, B, G, k)
            if got.dtype != torch.uint8 or not np.array_equal(got.numpy(), ref):
                out.append(f"draw B={B} G={G} k={k} sample0={sample0}: {int((got.numpy() != ref).sum())} bytes differ")
            elif not (got.sum(dim=1) == k).all():
                out.append(f"draw B={B} G={G} k={k}: not exactly k per sample")
        for kk in (0, G * G):
            if not bool((impl.draw(B, G, kk, KEY, SAMPLE0) == (1 if kk else 0)).all()):
                out.append(f"draw B={B} G={G} k={kk}: not all {'ones' if kk else 'zeros'}")
    B, G, k, cut = 5, 4, 7, 3                                         # a split batch with sample0 advanced equals one call
    one = impl.draw(B, G, k, KEY, SAMPLE0)
    two = torch.cat([impl.draw(cut, G, k, KEY, SAMPLE0), impl.draw(B - cut, G, k, KEY, SAMPLE0 + cut)])
    if not torch.equal(one, two):
        out.append("draw: a split batch with sample0 advanced differs from one call")
    for sample, lo, hi, pos in TIES if ties else []:
        for k, want in ((pos - 1, (0, 0)), (pos, (1, 0)), (pos + 1, (1, 1))):
            got = impl.draw(1, 32, k, KEY, sample)[0]
            if (int(got[lo]), int(got[hi])) != want or int(got.sum()) != k:
                out.append(f"draw tie sample {sample} k={k}: patches ({lo}, {hi}) -> {(int(got[lo]), int(got[hi]))}, want {want}")
    return out


def check_apply(impl, cases=HUBER_CASES):
    out = []
    for B, S, p in cases:
        x = inputs(B, S)[0]
        for name, mask in masks(B, S, p).items():
            if name == "all" and S > 32:
                continue
            ref = ref_apply(x, mask.numpy(), FILL, p)
            for in_place, lead in ((False, 0), (True, 0), (False, 1)):
                got = impl.apply(x.clone(), mask, FILL, p, in_place, lead)
                if not torch.equal(got.view(torch.int32), ref.view(torch.int32)):
                    out.append(f"apply B={B} S={S} p={p} mask={name} in_place={in_place} lead={lead}: "
                               f"{int((got != ref).sum())} elements differ")
        mask = masks(B, S, p)["drawn"]
        m = torch.from_numpy(ref_element_mask(mask.numpy(), S, p))
        xn = x.clone()
        xn[m] = float("nan")                                         # a select: masked NaNs do not reach y
        if torch.isnan(impl.apply(xn, mask, FILL, p, False, 0)).any():
            out.append(f"apply B={B} S={S} p={p}: a NaN in a masked pixel reached y")
    return out


def huber_figures(got, ref, m):
    loss, g = got
    return {"loss": abs(float(loss) - float(ref[0])), "loss_bound": TOL * float(ref[0]), "dtokens": rel_err(g, ref[1]),
            "outside": int((g[~m].view(torch.int32) != 0).sum())}


def check_huber(impl, cases=HUBER_CASES, verbose=False):
    out = []
    for B, S, p in cases:
        tokens, target = inputs(B, S)
        for name, mask in masks(B, S, p).items():
            m = torch.from_numpy(ref_element_mask(mask.numpy(), S, p))
            masked = int(mask.sum())
            variants = [(1.0, 1.0, 0)]
            if name == "drawn":
                variants += [(0.5, 1.0, 0), (1.0, 3.0, 0), (0.5, 3.0, 0), (1.0, 1.0, 1), (0.5, 3.0, 1)]
            for delta, dloss, lead in variants:
                what = f"huber B={B} S={S} p={p} mask={name} delta={delta} dloss={dloss} lead={lead}"
                got = impl.huber(tokens, target, mask, delta, dloss, p, masked, lead)
                f = huber_figures(got, ref_huber(tokens, target, mask.numpy(), delta, dloss, p, masked), m)
                if verbose:
                    print(f"{what}: loss off {f['loss']:.3e} (bound {f['loss_bound']:.3e}), dtokens {f['dtokens']:.3e}")
                if not f["loss"] <= f["loss_bound"]:
                    out.append(f"{what}: loss off by {f['loss']:.3e} > {f['loss_bound']:.3e}")
                if not f["dtokens"] <= TOL:
                    out.append(f"{what}: dtokens rel_err {f['dtokens']:.3e} > {TOL:.0e}")
                if f["outside"]:
                    out.append(f"{what}: {f['outside']} unmasked dtokens are not +0.0")
            if name != "drawn":
                continue
            # NaN: outside the mask nothing changes, inside it propagates
            base = impl.huber(tokens, target, mask, 1.0, 1.0, p, masked, 0)
            off, on = (~m).nonzero()[::97], m.nonzero()[:1]
            tn, gn = tokens.clone(), target.clone()
            tn[tuple(off[0::2].T)] = float("nan")
            gn[tuple(off[1::2].T)] = float("inf")
            got = impl.huber(tn, gn, mask, 1.0, 1.0, p, masked, 0)
            if not (torch.equal(got[0].view(torch.int32), base[0].view(torch.int32))
                    and torch.equal(got[1].view(torch.int32), base[1].view(torch.int32))):
                out.append(f"huber B={B} S={S} p={p}: a NaN / inf outside the mask changed the result")
            tn = tokens.clone()
            tn[tuple(on.T)] = float("nan")
            got = impl.huber(tn, target, mask, 1.0, 1.0, p, masked, 0)
            if not (torch.isnan(got[0]) and torch.isnan(got[1][tuple(on.T)]).all() and int(torch.isnan(got[1]).sum()) == 1):
                out.append(f"huber B={B} S={S} p={p}: a NaN inside the mask must make the loss and its own dtokens element NaN")
    return out
