"""Cases and reference of the reject_pairwise tests (tests/test_pairwise_host.py, tests/test_gpu_pairwise.py).

The reference is ``reference_pairwise``: numpy, written from the rule of DESIGN.md §14 with a plain loop per pair: float32 distances
operation by operation, ``np.sort`` of the valid values and the expressions of the rule written out in float64 (no ``np.median``), and
a plain loop per frame for the blame.  The rule is comparisons, five float32 operations and a correctly rounded square root per
distance, and a handful of IEEE double operations per pair, so the kernels (and the CPU program built from their header) must equal it
bit for bit: the tolerance is 0 on ``out`` (compared as uint32 words), ``flag``, ``pair_n``, ``pair_med`` and ``pair_mad`` (uint64).
"""

import numpy as np

TS = (1, 2, 3, 63, 64, 65, 129, 1000)
KS = (1, 2, 3, 23, 64)
MAD_TO_SIGMA = 1.4826
THR = 6.0 * MAD_TO_SIGMA  # n_sigma = 6, the default, as prep.reject_pairwise computes it
MIN_DEV = 0.002
QNAN = np.uint32(0x7FC00000)
QNAN64 = np.uint64(0x7FF8000000000000)
BIG = 1.0  # a displacement that no distribution of the cases holds


def pair_index(a, b, K):
    return a * (2 * K - a - 1) // 2 + (b - a - 1)


def pairs(K):
    return [(a, b) for a in range(K - 1) for b in range(a + 1, K)]


def reference_pairwise(kp, thr, min_dev, votes):
    """kp [T, 3K] float32 -> (out [T, 3K] float32, flag [T, K] uint8, pair_n [P] int64, pair_med [P], pair_mad [P] float64)"""
    kp = np.asarray(kp, dtype=np.float32)
    T, K = kp.shape[0], kp.shape[1] // 3
    x = kp.reshape(T, K, 3)
    present = np.isfinite(x).all(axis=2)
    P = K * (K - 1) // 2
    thr, min_dev = float(thr), float(min_dev)
    pair_n = np.zeros(P, np.int64)
    pair_med = np.full(P, np.nan, np.float64)
    pair_mad = np.full(P, np.nan, np.float64)
    pair_med.view(np.uint64)[:] = QNAN64
    pair_mad.view(np.uint64)[:] = QNAN64
    bad = np.zeros((T, K, K), bool)
    with np.errstate(all="ignore"):
        for p, (a, b) in enumerate(pairs(K)):
            assert p == pair_index(a, b, K)
            dx, dy, dz = x[:, a, 0] - x[:, b, 0], x[:, a, 1] - x[:, b, 1], x[:, a, 2] - x[:, b, 2]  # float32, one operation each
            d = np.sqrt((dx * dx + dy * dy) + dz * dz)
            assert d.dtype == np.float32
            valid = present[:, a] & present[:, b] & np.isfinite(d)
            n = int(np.count_nonzero(valid))
            pair_n[p] = n
            if n < 3:
                continue
            s = np.sort(d[valid])
            med = 0.5 * (float(s[(n - 1) // 2]) + float(s[n // 2]))  # (Python floats are IEEE doubles: a float32 converts exactly)
            e = np.abs(d.astype(np.float64) - med).astype(np.float32)
            E = np.sort(e[valid])
            mad = 0.5 * (float(E[(n - 1) // 2]) + float(E[n // 2]))
            pair_med[p], pair_mad[p] = med, mad
            e64 = e.astype(np.float64)
            is_bad = valid & (e64 > thr * mad) & (e64 > min_dev)
            if is_bad.any():
                bad[:, a, b] = is_bad
                bad[:, b, a] = is_bad
    return _blame(kp, bad, votes) + (pair_n, pair_med, pair_mad)


def _blame(kp, bad, votes):
    """bad [T, K, K] (symmetric) -> (out, flag) by the blame rule, a plain loop per frame"""
    T, K = bad.shape[:2]
    flag = np.zeros((T, K), np.uint8)
    for t in np.flatnonzero(bad.any(axis=(1, 2))):
        B = bad[t].copy()
        while True:
            c = B.sum(axis=1)
            k = int(np.argmax(c))  # (the first maximum: ties go to the lowest k)
            if c[k] < votes:
                break
            flag[t, k] = 1
            B[k, :] = False
            B[:, k] = False
    out = np.array(kp).reshape(T, K, 3)
    out.view(np.uint32)[flag == 1] = QNAN
    return out.reshape(T, 3 * K), flag


def reference_pairwise_all_pairs(kp, thr, min_dev, votes):
    """``reference_pairwise`` with every pair's loop body written for all pairs at once (one ``np.sort`` along time of the [T, P]
    distances, the frames that are not valid sorted to the end as +inf and never indexed): the same operations on the same
    values, a hundred times faster at K = 64.  It is what ``reference`` hands to the tests; tests/test_pairwise_host.py holds
    it against ``reference_pairwise`` on every case, bit for bit."""
    kp = np.asarray(kp, dtype=np.float32)
    T, K = kp.shape[0], kp.shape[1] // 3
    x = kp.reshape(T, K, 3)
    present = np.isfinite(x).all(axis=2)
    ab = np.array(pairs(K), dtype=np.int64).reshape(-1, 2)
    A, B = ab[:, 0], ab[:, 1]
    P, col = len(A), np.arange(len(A))
    thr, min_dev = np.float64(thr), np.float64(min_dev)
    nan64 = np.array([QNAN64], np.uint64).view(np.float64)[0]
    with np.errstate(all="ignore"):
        dx, dy, dz = x[:, A, 0] - x[:, B, 0], x[:, A, 1] - x[:, B, 1], x[:, A, 2] - x[:, B, 2]
        d = np.sqrt((dx * dx + dy * dy) + dz * dz)
        assert d.dtype == np.float32 and d.shape == (T, P)
        valid = present[:, A] & present[:, B] & np.isfinite(d)
        n = valid.sum(axis=0).astype(np.int64)
        ok = n >= 3
        r0, r1 = np.where(ok, (n - 1) // 2, 0), np.where(ok, n // 2, 0)
        s = np.sort(np.where(valid, d, np.float32(np.inf)), axis=0)
        med = np.float64(0.5) * (s[r0, col].astype(np.float64) + s[r1, col].astype(np.float64))
        e = np.abs(d.astype(np.float64) - med[None, :]).astype(np.float32)
        E = np.sort(np.where(valid, e, np.float32(np.inf)), axis=0)
        mad = np.float64(0.5) * (E[r0, col].astype(np.float64) + E[r1, col].astype(np.float64))
        e64 = e.astype(np.float64)
        is_bad = valid & ok[None, :] & (e64 > (thr * mad)[None, :]) & (e64 > min_dev)
    bad = np.zeros((T, K, K), bool)
    bad[:, A, B] = is_bad
    bad[:, B, A] = is_bad
    pair_med, pair_mad = np.where(ok, med, nan64), np.where(ok, mad, nan64)
    pair_med.view(np.uint64)[~ok] = QNAN64
    pair_mad.view(np.uint64)[~ok] = QNAN64
    return _blame(kp, bad, votes) + (n, pair_med, pair_mad)


def skeleton(T, K, rng, noise=0.001, move=0.05):
    """[T, K, 3] float32: K points of a rigid shape of about 30 cm that drifts by ``move`` and jitters by ``noise`` per keypoint"""
    t = np.arange(T, dtype=np.float64)[:, None, None]
    shape = rng.uniform(-0.15, 0.15, (1, K, 3))
    drift = move * np.sin(2 * np.pi * rng.uniform(0.002, 0.01, (1, 1, 3)) * t + rng.uniform(0, 2 * np.pi, (1, 1, 3)))
    return (shape + drift + noise * rng.standard_normal((T, K, 3))).astype(np.float32)


# ---- the patterns: each works on x [T, K, 3] in place and may return parameters that differ from the defaults ---------------------
def p_no_defect(x, rng):
    pass


def p_missing(x, rng):  # every keypoint is missing in some frames, by a NaN or an infinity in one coordinate
    T, K = x.shape[:2]
    for k in range(K):
        for t in range(T):
            if (t + k) % 5 == 0:
                x[t, k, t % 3] = (np.nan, np.inf, -np.inf)[(t + k) % 3]


def p_pair_counts(x, rng):  # the pairs (0, 1), (0, 2), (1, 2) have 0, 2 and 3 valid frames
    T = x.shape[0]
    x[2:, 0] = np.nan
    x[:2, 1] = np.nan
    x[5:, 1] = np.nan


def p_identical(x, rng):  # mad = 0 for every pair: min_dev alone decides; one displacement below it and one above
    T, K = x.shape[:2]
    x[:] = x[0]
    x[T // 2, 0, 0] += np.float32(0.0005)
    x[T // 3, K - 1, 1] += np.float32(0.5)
    return dict(votes=1)


def _tie_kps(K):
    return (K - 1) // 3, K - 1


def p_tie(x, rng):  # two wrong keypoints with K - 1 bad pairs each and votes = K - 1: the lower index goes, the other one stays
    T, K = x.shape[:2]
    a, b = _tie_kps(K)
    x[T // 2, a, 0] += np.float32(BIG)
    x[T // 2, b, 1] -= np.float32(BIG)
    return dict(votes=K - 1)


def _two_wrong_kps(K):
    return K // 3, (2 * K) // 3


def p_two_wrong(x, rng):  # an innocent third keypoint has two bad pairs until the first removal
    T, K = x.shape[:2]
    a, b = _two_wrong_kps(K)
    x[T // 2, a, 2] += np.float32(BIG)
    x[T // 2, b, 0] -= np.float32(2 * BIG)
    return dict(votes=2)


def _noise(x, rng, size=0.1, missing=0.05):
    T, K = x.shape[:2]
    hit = rng.random((T, K)) < 0.03
    x[hit] += (size * rng.standard_normal((int(hit.sum()), 3))).astype(np.float32)
    x[rng.random((T, K)) < missing] = np.nan


def p_noise_votes_1(x, rng):
    _noise(x, rng)
    return dict(votes=1, min_dev=0.0)


def p_noise_votes_2(x, rng):
    _noise(x, rng)


def p_noise_votes_K_minus_1(x, rng):  # (every pair of a keypoint must be valid and bad: large displacements, nothing missing)
    _noise(x, rng, size=1.0, missing=0.0)
    return dict(votes=max(x.shape[1] - 1, 1), thr=3.0 * MAD_TO_SIGMA)


def p_huge(x, rng):  # coordinates of 1e20: present keypoints whose distances are infinite, so their pairs are not valid there
    T, K = x.shape[:2]
    for t in range(T):
        if t % 7 == 3 or T < 3:
            x[t, K - 1, 0] = np.float32(1e20)
            x[t, 0, 1] = np.float32(-1e20)


def p_zeros_and_denormals(x, rng):  # a still keypoint 0 at -0.0 / +0.0 / denormal coordinates: finite values that pass bit for bit
    T = x.shape[0]
    x[:] = x[0] + (0.001 * rng.standard_normal(x.shape)).astype(np.float32)
    for t in range(T):
        x[t, 0, 0] = np.float32(-0.0 if t % 2 else 0.0)
        x[t, 0, 1] = np.float32((t % 50) * 1e-45)
        x[t, 0, 2] = np.float32(-1e-42)


def _line(x, bits, rng):  # keypoint 0 at the origin and keypoint 1 on the x axis: d of the pair (0, 1) has exactly these bits
    x[:, 0] = 0.0
    x[:, 1] = 0.0
    x[:, 1, 0] = np.asarray(bits, np.uint32).view(np.float32)


def p_second_pass_only(x, rng):  # d of (0, 1) differs in the bits 10 .. 20 alone: only the second selection pass separates them
    _line(x, np.uint32(0x3F800000) | (rng.integers(0, 2048, x.shape[0]).astype(np.uint32) << np.uint32(10)), rng)


def p_third_pass_only(x, rng):  # ... in the last 10 bits alone
    _line(x, np.uint32(0x3F800000) | rng.integers(0, 1024, x.shape[0]).astype(np.uint32), rng)


def _tie_rank(x, rng, where):
    """d of (0, 1) is 1, 2 or 3: the rank (n - 1) / 2 is the first, a middle or the last of the 2s"""
    T = x.shape[0]
    r0 = (T - 1) // 2
    m2 = max(T // 4, 1)
    m1 = {"first": r0, "middle": r0 - m2 // 2, "last": r0 - m2 + 1}[where]
    m1 = max(m1, 0)
    v = np.full(T, 3.0, np.float32)
    v[:m1] = 1.0
    v[m1:m1 + m2] = 2.0
    _line(x, rng.permutation(v).view(np.uint32), rng)


def p_tie_rank_first(x, rng):
    _tie_rank(x, rng, "first")


def p_tie_rank_middle(x, rng):
    _tie_rank(x, rng, "middle")


def p_tie_rank_last(x, rng):
    _tie_rank(x, rng, "last")


# name -> (pattern, least T, least K) at which it holds what it is meant to; below that it does not fit the shape
PATTERNS = {
    "no_defect": (p_no_defect, 1, 1), "missing": (p_missing, 1, 1), "pair_counts": (p_pair_counts, 5, 3),
    "identical": (p_identical, 3, 2), "tie": (p_tie, 3, 2), "two_wrong": (p_two_wrong, 3, 4),
    "noise_votes_1": (p_noise_votes_1, 1, 1), "noise_votes_2": (p_noise_votes_2, 1, 1),
    "noise_votes_K_minus_1": (p_noise_votes_K_minus_1, 3, 2), "huge": (p_huge, 1, 1),
    "zeros_and_denormals": (p_zeros_and_denormals, 1, 1), "second_pass_only": (p_second_pass_only, 3, 2),
    "third_pass_only": (p_third_pass_only, 3, 2), "tie_rank_first": (p_tie_rank_first, 3, 2),
    "tie_rank_middle": (p_tie_rank_middle, 3, 2), "tie_rank_last": (p_tie_rank_last, 3, 2),
}  # fmt: skip


def make_case(name, T, K):
    """-> (kp [T, 3K] float32, thr, min_dev, votes)"""
    names = list(PATTERNS)
    rng = np.random.default_rng(1_000_000 * (names.index(name) + 1) + 100 * T + K)
    x = skeleton(T, K, rng)
    par = dict(thr=THR, min_dev=MIN_DEV, votes=2)
    par.update(PATTERNS[name][0](x, rng) or {})
    return np.ascontiguousarray(x.reshape(T, 3 * K)), par["thr"], par["min_dev"], par["votes"]


def cases(ks=KS, ts=TS):
    """(name, T, K) of every case: every pattern that fits at every T x K of the grid"""
    return [(name, T, K) for K in ks for T in ts for name, (_, t_min, k_min) in PATTERNS.items() if T >= t_min and K >= k_min]


_REF = {}


def reference(name, T, K):
    """(kp, thr, min_dev, votes, (out, flag, pair_n, pair_med, pair_mad)) of a case, computed once and shared (read-only)"""
    key = (name, T, K)
    if key not in _REF:
        kp, thr, min_dev, votes = make_case(name, T, K)
        want = reference_pairwise_all_pairs(kp, thr, min_dev, votes)
        for a in (kp, *want):
            a.setflags(write=False)
        _REF[key] = (kp, thr, min_dev, votes, want)
    return _REF[key]


def check(got, kp, want, label=""):
    """Tolerance 0 on the five outputs; a rejected keypoint is three quiet NaNs 0x7FC00000, every other element the input's bits."""
    names = ("out", "flag", "pair_n", "pair_med", "pair_mad")
    dtypes = (np.float32, np.uint8, np.int64, np.float64, np.float64)
    for name, dt, g, w in zip(names, dtypes, got, want):
        g = np.asarray(g)
        assert g.dtype == dt and g.shape == w.shape, (label, name, g.dtype, g.shape, w.shape)
        bits = {4: np.uint32, 8: np.uint64, 1: np.uint8}[g.dtype.itemsize]
        np.testing.assert_array_equal(g.view(bits), w.view(bits), err_msg=f"{label} {name} (bits)")
    want_flag = want[1]
    T, K = want_flag.shape
    g, x = np.asarray(got[0]).reshape(T, K, 3).view(np.uint32), np.asarray(kp).reshape(T, K, 3).view(np.uint32)
    assert (g[want_flag == 1] == QNAN).all(), label
    np.testing.assert_array_equal(g[want_flag == 0], x[want_flag == 0], err_msg=f"{label} passed entries (bits)")


# ---- the motivating case: 40-frame left / right swaps in the golden rodent recording --------------------------------------------
def swap_pairs(kp_names):
    """The left / right keypoint pairs (index of ...L, index of ...R) in the order of the sorted names"""
    names = list(kp_names)
    return [(names.index(n), names.index(n[:-1] + "R")) for n in sorted(names) if n.endswith("L") and n[:-1] + "R" in names]


def swapped_recording(mocap, kp_names, run=40, first=50, step=60):
    """-> (kp with every left / right pair swapped for ``run`` frames, wrong [T, K] bool): the first run starts at ``first``, each
    later one ``step`` frames after the one before"""
    kp = np.array(mocap, dtype=np.float32)
    T, K = kp.shape[0], kp.shape[1] // 3
    x = kp.reshape(T, K, 3)
    wrong = np.zeros((T, K), bool)
    for i, (l, r) in enumerate(swap_pairs(kp_names)):
        t0 = first + i * step
        x[t0:t0 + run, [l, r]] = x[t0:t0 + run, [r, l]]
        wrong[t0:t0 + run, [l, r]] = True
    return kp, wrong
