"""The checker of the k-NN probe's entry points (calm_knn_normalize / _merge / _vote): references written from the contract of
include/calm_vit.h in float64 numpy — the neighbours by np.lexsort on (index, -similarity) over the WHOLE bank, never chunk
by chunk — the cases, and the bounds.  Shared by tests/test_knn_cpu.py (on the emulation, its planted faults and the torch
twins of trainer.py) and tests/test_knn_gpu.py (on the kernels).

An implementation under test is an object with, over CPU tensors in and out,
    normalize(x [N, D] fp32 / bf16, pad, lead)            -> (out fp32 [N, D], zeroed rows as an int)
    similarities(q [Nq, D] fp32, rows [n, D] fp32)          -> fp32 [Nq, n], its own GEMM
    merge(sims [Nq, n], base, best_sim, best_idx, pad, lead) -> (best_sim, best_idx), new tensors
    vote(best_sim, best_idx, bank_labels, inv_T, C)          -> scores fp32 [Nq, C]
`pad` asks for a row stride of that many elements more than the row, `lead` for a tensor base that many elements behind a
16-byte boundary (an emulation has no addresses and ignores both).

Bounds:
  exact cases, hand-built rows   bit-exact (similarity, index) state.  Queries and bank lie on the grid m / 8, |m| <= 16, with
                                 D <= 1024: every product is a multiple of 1/64 below 4 and every partial sum a multiple of 1/64
                                 below 4096 < 2^24 / 64, so the fp32 GEMM is exact in any summation order;
  realistic cases                unit rows: |fp32 dot - float64 dot| <= D * 2^-24 by the standard bound, doubled for the rounding
                                 of the two normalisations: eps = D * 2^-23.  Every returned similarity within eps of the
                                 float64 one at its index; everything above the float64 k-th value + 2 eps present, nothing
                                 below it - 2 eps; indices distinct; the list sorted under the contract's order by its own values;
  normalize                      |got - ref| <= (D + 8) * 2^-24 * |ref| per element (the sum of D squares, a square root and a
                                 division); zero and non-finite rows are +0.0 bits and counted;
  vote                           against float64 on the implementation's OWN state: |got - ref| <= 1e-4 * ref per element (a sum of
                                 non-negative terms; TOL of tests/bce_f64.py), exactly +0.0 for a class without a neighbour, equal
                                 bits for two classes built with equal votes."""
import numpy as np
import torch

TOL = 1e-4
NEG_INF = float("-inf")
# (Nq, Nb, D, k, chunk)
EXACT_CASES = [(1, 1, 1, 1, 1), (3, 5, 8, 8, 2), (2, 64, 16, 1, 64), (5, 257, 144, 20, 64), (4, 1000, 96, 200, 333),
               (2, 4099, 384, 256, 4099), (1, 16387, 144, 20, 16384)]
# (Nq, Nb, D, C, k, chunk, noise)
REALISTIC_CASES = [(33, 2000, 144, 10, 20, 512, 2.0), (7, 3001, 96, 5, 256, 1111, 1.0), (5, 300, 31, 3, 1, 300, 0.5)]
# (N, D, bf16, pad, lead)
NORMALIZE_CASES = [(5, 1, False, 0, 0), (9, 3, False, 1, 0), (6, 96, False, 0, 0), (6, 96, False, 3, 1), (7, 144, True, 0, 0),
                   (7, 144, True, 5, 2), (5, 1027, False, 1, 0), (4, 1027, True, 0, 0), (4, 1027, True, 5, 0), (3, 4096, False, 0, 0),
                   (3, 4096, True, 8, 0), (130, 40, False, 0, 0)]
VOTE_KS, VOTE_CS = (1, 20, 256), (1, 10, 257, 1000)


def empty_state(Nq, k):
    return torch.full((Nq, k), NEG_INF, dtype=torch.float32), torch.full((Nq, k), -1, dtype=torch.int64)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- references -----------------------------------------------------------------------------------------------------------
def ref_topk(sims, idx, k):
    """(sims fp32 [Nq, k], idx int64 [Nq, k]) of the entries sims [Nq, M] (fp32 numpy, stored bits) at bank indices idx [M]:
    float64 lexsort by similarity descending (NaN = -inf), then index ascending; (-inf, -1) where M < k."""
    sims = np.asarray(sims, dtype=np.float32)
    s64 = sims.astype(np.float64)
    s64[np.isnan(s64)] = -np.inf
    stored = sims.copy()
    stored[np.isnan(sims)] = -np.inf
    Nq, M = sims.shape
    out_s = np.full((Nq, k), -np.inf, dtype=np.float32)
    out_i = np.full((Nq, k), -1, dtype=np.int64)
    for q in range(Nq):
        order = np.lexsort((idx, -s64[q]))[:k]
        out_s[q, :len(order)] = stored[q, order]
        out_i[q, :len(order)] = idx[order]
    return torch.from_numpy(out_s), torch.from_numpy(out_i)


def state_diff(got, want, what):
    (gs, gi), (ws, wi) = got, want
    bad = []
    if not torch.equal(gi, wi):
        q, j = [int(v) for v in (gi != wi).nonzero()[0]]
        bad.append(f"{what}: index [{q}, {j}] is {int(gi[q, j])}, expected {int(wi[q, j])}")
    if not torch.equal(bits(gs), bits(ws)):
        q, j = [int(v) for v in (bits(gs) != bits(ws)).nonzero()[0]]
        bad.append(f"{what}: similarity [{q}, {j}] is {float(gs[q, j])!r}, expected {float(ws[q, j])!r} (bits)")
    return bad


def run_chunks(impl, chunks, Nq, k, pad=0, lead=0):
    """The state after merging chunks = [(base, sims [Nq, n])] in the given order from an empty state."""
    state = empty_state(Nq, k)
    for base, sims in chunks:
        state = impl.merge(sims, base, state[0], state[1], pad, lead)
    return state


# ---- exact cases ----------------------------------------------------------------------------------------------------------
def grid_case(Nq, Nb, D, seed=0):
    """(queries, bank) fp32 on the grid m / 8, |m| <= 16; every seventh bank row repeats the row three before it and a few
    rows repeat across the whole bank, so equal similarities occur next to each other and far apart."""
    g = torch.Generator().manual_seed(7919 * Nq + 31 * Nb + D + seed)
    q = torch.randint(-16, 17, (Nq, D), generator=g).float() / 8
    bank = torch.randint(-16, 17, (Nb, D), generator=g).float() / 8
    for i in range(6, Nb, 7):
        bank[i] = bank[i - 3]
    if Nb > 40:
        bank[Nb - 1] = bank[0]
        bank[Nb // 2] = bank[1]
    return q, bank


def chunkings(Nb, chunk):
    first = [(b, min(chunk, Nb - b)) for b in range(0, Nb, chunk)]
    other = max(1, (2 * chunk) // 3 + 1)
    second = [(b, min(other, Nb - b)) for b in range(0, Nb, other)]
    return [("in order", first), ("second chunking", second), ("reversed", first[::-1]), ("second reversed", second[::-1])]


def check_exact(impl, cases=EXACT_CASES):
    bad = []
    for Nq, Nb, D, k, chunk in cases:
        q, bank = grid_case(Nq, Nb, D)
        s64 = q.double().numpy() @ bank.double().numpy().T
        want = ref_topk(s64.astype(np.float32), np.arange(Nb, dtype=np.int64), k)
        assert np.array_equal(s64.astype(np.float32).astype(np.float64), s64)          # the grid keeps fp32 exact
        first = None
        for name, spans in chunkings(Nb, chunk):
            got = run_chunks(impl, [(b, impl.similarities(q, bank[b:b + n])) for b, n in spans], Nq, k)
            what = f"exact {(Nq, Nb, D, k, chunk)} {name}"
            bad += state_diff(got, want, what)
            if first is None:
                first = got
            elif not (torch.equal(got[1], first[1]) and torch.equal(bits(got[0]), bits(first[0]))):
                bad.append(f"{what}: the state depends on the chunking")
    return bad


# ---- hand-built rows for merge alone -----------------------------------------------------------------------------------------
def row_cases():
    """[(name, k, [(base, sims fp32 [Nq, n])], pad, lead)]"""
    f = lambda *rows: torch.tensor(rows, dtype=torch.float32)
    g = torch.Generator().manual_seed(11)
    cases = []
    cases.append(("all equal", 20, [(0, torch.full((2, 3000), 0.5))], 0, 0))
    cases.append(("all equal, k = 256", 256, [(0, torch.full((1, 1500), -0.25))], 0, 0))
    asc = torch.arange(2000, dtype=torch.float32)[None, :] / 2048
    cases.append(("strictly ascending", 256, [(0, asc)], 0, 0))
    cases.append(("strictly descending", 256, [(0, asc.flip(1).contiguous())], 0, 0))
    cases.append(("-0.0 next to +0.0", 6, [(0, f([-1.0, -0.0, 0.0, -0.0, 0.0, -2.0, 0.0, -0.0, -3.0]))], 0, 0))
    cases.append(("-inf entries", 6, [(0, f([NEG_INF, 1.0, NEG_INF, NEG_INF, 0.5, NEG_INF, NEG_INF]))], 0, 0))
    cases.append(("-inf entries, bank below k", 6, [(0, f([NEG_INF, 1.0, NEG_INF, NEG_INF]))], 0, 0))
    cases.append(("all -inf, two chunks", 5, [(0, f([NEG_INF] * 3)), (3, f([NEG_INF] * 4))], 0, 0))
    nan = float("nan")
    cases.append(("NaN ranks as -inf", 5, [(0, f([nan, NEG_INF, 0.25, nan, -1e30, NEG_INF, nan]))], 0, 0))
    cases.append(("NaN among many", 20, [(0, torch.where(torch.rand(3, 1500, generator=g) < 0.3, torch.tensor(nan),
                                                             torch.randint(-3, 4, (3, 1500), generator=g).float()))], 0, 0))
    a, b = torch.zeros(1, 50), torch.zeros(1, 50)
    a[0, 49] = b[0, 0] = 2.0
    cases.append(("duplicated maximum across a chunk boundary", 1, [(0, a), (50, b)], 0, 0))
    cases.append(("duplicated maximum across a chunk boundary, reversed", 1, [(50, b), (0, a)], 0, 0))
    cases.append(("duplicated maximum across a chunk boundary, k = 3", 3, [(50, b), (0, a)], 0, 0))
    hi = torch.rand(2, 400, generator=g) + 2.0
    lo = torch.rand(2, 1200, generator=g)
    cases.append(("a warm state beats the whole chunk", 20, [(0, hi), (400, lo)], 0, 0))
    cases.append(("a chunk replaces the whole state", 20, [(400, lo[:, :30].contiguous()), (0, hi)], 0, 0))
    ties = torch.randint(-5, 6, (3, 1003), generator=g).float() / 4
    cases.append(("row stride % 4 == 1", 20, [(0, ties)], 2, 0))               # 1003 + 2 = 1005 = 4 * 251 + 1
    cases.append(("row stride % 4 == 1, base off 16 bytes", 256, [(0, ties), (1003, ties.flip(1).contiguous())], 2, 3))
    cases.append(("base above 2^31", 20, [((1 << 31) + 5, ties), (3 * (1 << 31), ties.flip(1).contiguous()), (7, ties)], 0, 0))
    heavy = torch.randint(0, 3, (4, 5000), generator=g).float()
    cases.append(("ties at the k-th value of a cold state", 256, [(0, heavy)], 0, 1))
    cases.append(("ties at the k-th value, three chunks", 100, [(5000, heavy), (0, heavy.flip(1).contiguous()),
                                                                 (10000, heavy[:, :777].contiguous())], 0, 0))
    return cases


def check_rows(impl):
    bad = []
    for name, k, chunks, pad, lead in row_cases():
        Nq = chunks[0][1].shape[0]
        sims = np.concatenate([s.numpy() for _, s in chunks], axis=1)
        idx = np.concatenate([b + np.arange(s.shape[1], dtype=np.int64) for b, s in chunks])
        want = ref_topk(sims, idx, k)
        got = run_chunks(impl, chunks, Nq, k, pad, lead)
        bad += state_diff(got, want, f"rows '{name}'")
        if name == "a warm state beats the whole chunk":            # the state is the first chunk's, bit for bit
            warm = run_chunks(impl, chunks[:1], Nq, k, pad, lead)
            if not (torch.equal(warm[1], got[1]) and torch.equal(bits(warm[0]), bits(got[0]))):
                bad.append(f"rows '{name}': the state changed")
    return bad


# ---- realistic cases ----------------------------------------------------------------------------------------------------------
def cluster_case(Nq, Nb, D, C, noise, seed=0):
    """(bank [Nb, D], bank labels, queries [Nq, D], query labels): class centroids plus noise, fp32, not normalised."""
    g = torch.Generator().manual_seed(104729 + 13 * Nb + D + seed)
    cent = torch.randn(C, D, generator=g) * 3.0
    bl, ql = torch.arange(Nb) % C, torch.arange(Nq) % C
    bank = cent[bl] + noise * torch.randn(Nb, D, generator=g)
    q = cent[ql] + noise * torch.randn(Nq, D, generator=g)
    return bank, bl, q, ql


def unit64(x):
    x = x.double()
    return x / x.norm(dim=1, keepdim=True)


def tolerant_diff(got_s, got_i, s64, k, eps, what):
    """The realistic rule for one query set: got [Nq, k] against float64 similarities s64 [Nq, Nb] (numpy); k <= Nb."""
    bad, worst = [], 0.0
    gs, gi = got_s.double().numpy(), got_i.numpy()
    Nq, Nb = s64.shape
    for q in range(Nq):
        if (gi[q] < 0).any() or (gi[q] >= Nb).any() or len(set(gi[q].tolist())) != k:
            bad.append(f"{what}: query {q}: indices are not k distinct bank items")
            continue
        err = np.abs(gs[q] - s64[q, gi[q]]).max()
        worst = max(worst, err / eps)
        if err > eps:
            bad.append(f"{what}: query {q}: a similarity is {err:.3e} from float64 (eps {eps:.3e})")
        kth = np.sort(s64[q])[::-1][k - 1]
        member = np.zeros(Nb, dtype=bool)
        member[gi[q]] = True
        if (~member & (s64[q] > kth + 2 * eps)).any():
            bad.append(f"{what}: query {q}: an item above the k-th value + 2 eps is missing")
        if (member & (s64[q] < kth - 2 * eps)).any():
            bad.append(f"{what}: query {q}: an item below the k-th value - 2 eps is present")
        srt = all(gs[q, j] > gs[q, j + 1] or (gs[q, j] == gs[q, j + 1] and gi[q, j] < gi[q, j + 1]) for j in range(k - 1))
        if not srt:
            bad.append(f"{what}: query {q}: the list is not sorted by (similarity descending, index ascending)")
    return bad, worst


def check_realistic(impl, cases=REALISTIC_CASES):
    bad = []
    for Nq, Nb, D, C, k, chunk, noise in cases:
        bank, _, q, _ = cluster_case(Nq, Nb, D, C, noise)
        bn, qn = impl.normalize(bank, 0, 0)[0], impl.normalize(q, 0, 0)[0]
        got = run_chunks(impl, [(b, impl.similarities(qn, bn[b:b + chunk])) for b in range(0, Nb, chunk)], Nq, k)
        s64 = (unit64(q) @ unit64(bank).T).numpy()
        what = f"realistic {(Nq, Nb, D, C, k, chunk)}"
        b, worst = tolerant_diff(got[0], got[1], s64, k, D * 2.0 ** -23, what)
        print(f"{what}: worst |sim - float64| / eps = {worst:.4f}")
        bad += b
    return bad


# ---- normalize --------------------------------------------------------------------------------------------------------------
def normalize_case(N, D, bf16, seed=0):
    g = torch.Generator().manual_seed(17 * N + D + seed)
    x = torch.randn(N, D, generator=g) * 3.0
    if N > 1:
        x[1] = 0.0                                                  # norm 0
    if N > 2:
        x[2, D // 2] = float("nan")
    if N > 3:
        x[3, D - 1] = float("inf")
    if N > 4:
        x[4] = -0.0
    if N > 8:
        x[8, 0] = NEG_INF
    return x.bfloat16() if bf16 else x


def check_normalize(impl, cases=NORMALIZE_CASES):
    bad = []
    for N, D, bf16, pad, lead in cases:
        x = normalize_case(N, D, bf16)
        out, zeroed = impl.normalize(x, pad, lead)
        what = f"normalize {(N, D, 'bf16' if bf16 else 'fp32', pad, lead)}"
        x64 = x.double()
        nrm = x64.norm(dim=1)
        ok = torch.isfinite(x64).all(dim=1) & (nrm > 0)
        if out.dtype != torch.float32 or tuple(out.shape) != (N, D):
            bad.append(f"{what}: fp32 [N, D] expected")
            continue
        if int(zeroed) != int((~ok).sum()):
            bad.append(f"{what}: {int(zeroed)} zeroed rows counted, expected {int((~ok).sum())}")
        if bool((bits(out[~ok]) != 0).any()):
            bad.append(f"{what}: a zero or non-finite row is not all +0.0")
        ref = x64[ok] / nrm[ok][:, None]
        err = (out[ok].double() - ref).abs()
        tol = (D + 8) * 2.0 ** -24
        ratio = float((err / (tol * ref.abs()).clamp(min=1e-300)).max()) if err.numel() else 0.0
        print(f"{what}: worst error / bound = {ratio:.4f}")
        if not ratio <= 1.0:
            bad.append(f"{what}: an element is {ratio:.3f} x the bound (D + 8) * 2^-24 from float64")
    return bad


# ---- vote -------------------------------------------------------------------------------------------------------------------
def vote_case(k, C, seed=0):
    """(best_sim [Nq, k], best_idx [Nq, k], bank_labels [Nb], inv_T, (class a, class b) built with equal votes in row 1 or
    None).  Row 0: real -inf similarities in front of empty slots; row 1: the equal-vote classes; row 2: empty slots at the
    end; the others random.  Some bank labels lie outside [0, C)."""
    g = torch.Generator().manual_seed(1009 * k + C + seed)
    Nq, Nb = 6, 4 * k + 50
    labels = torch.randint(0, C, (Nb,), generator=g)
    labels[::9] = -1
    labels[4::9] = C
    labels[5::11] = C + 5
    sims = (torch.rand(Nq, k, generator=g) * 2 - 1).sort(dim=1, descending=True).values
    idx = torch.stack([torch.randperm(Nb, generator=g)[:k] for _ in range(Nq)])
    real = max(k // 2, 1)
    sims[0] = NEG_INF
    idx[0, real:] = -1
    equal = None
    if C >= 2 and k >= 2:
        a, b = 0, C - 1
        ia, ib = (labels == a).nonzero()[:, 0], (labels == b).nonzero()[:, 0]
        pairs = min(k // 2, len(ia), len(ib))
        if pairs:
            for p in range(pairs):                                  # slots 2p / 2p + 1: one similarity, labels a / b
                sims[1, 2 * p + 1] = sims[1, 2 * p]
                idx[1, 2 * p], idx[1, 2 * p + 1] = ia[p], ib[p]
            other = (labels != a) & (labels != b)
            rest = other.nonzero()[:, 0]
            idx[1, 2 * pairs:] = rest[:k - 2 * pairs]
            equal = (a, b)
    if k > 2:
        sims[2, k - k // 3:] = NEG_INF
        idx[2, k - k // 3:] = -1
    return sims.contiguous(), idx.contiguous(), labels, 1.0 / 0.07, equal


def ref_vote(best_sim, best_idx, labels, inv_T, C):
    s, idx, lab = best_sim.double().numpy(), best_idx.numpy(), labels.numpy()
    t = float(np.float32(inv_T))
    out = np.zeros((s.shape[0], C))
    for q in range(s.shape[0]):
        for j in range(s.shape[1]):
            i = idx[q, j]
            if i < 0 or i >= len(lab) or not 0 <= lab[i] < C:
                continue
            d = 0.0 if s[q, j] == s[q, 0] else s[q, j] - s[q, 0]
            out[q, lab[i]] += np.exp(d * t)
    return out


def check_vote(impl, ks=VOTE_KS, cs=VOTE_CS):
    bad = []
    for k in ks:
        for C in cs:
            sims, idx, labels, inv_T, equal = vote_case(k, C)
            got = impl.vote(sims, idx, labels, inv_T, C)
            what = f"vote k={k} C={C}"
            if got.dtype != torch.float32 or tuple(got.shape) != (sims.shape[0], C):
                bad.append(f"{what}: fp32 [Nq, C] expected")
                continue
            ref = ref_vote(sims, idx, labels, inv_T, C)
            g = got.double().numpy()
            if not np.isfinite(g).all() or (np.abs(g - ref) > TOL * ref).any():
                q, c = [int(v[0]) for v in np.nonzero(~(np.abs(g - ref) <= TOL * ref))]
                bad.append(f"{what}: scores[{q}, {c}] = {g[q, c]!r}, float64 says {ref[q, c]!r}")
            if bool((bits(got)[torch.from_numpy(ref == 0)] != 0).any()):
                bad.append(f"{what}: a class without a neighbour is not exactly +0.0")
            if equal is not None and int(bits(got)[1, equal[0]]) != int(bits(got)[1, equal[1]]):
                bad.append(f"{what}: two classes with equal votes differ in their bits")
    return bad


CHECKS = {"exact": check_exact, "rows": check_rows, "realistic": check_realistic, "normalize": check_normalize,
          "vote": check_vote}
