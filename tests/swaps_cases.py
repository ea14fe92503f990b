"""Cases and reference of the repair_swaps tests (tests/test_swaps_host.py, tests/test_gpu_swaps.py).

The reference is ``reference_swaps``: numpy, written from the rule of DESIGN.md §15 with a plain loop per candidate and frame over
the float32 distances of §14 and the statistics of ``pairwise_cases.reference_pairwise_all_pairs``.  The rule is comparisons, the
single IEEE operations of §14 and integer counts, so the kernel (and the CPU program built from its header) must equal it bit for
bit: the tolerance is 0 on ``out`` (compared as uint32 words), ``flag`` (uint8), ``pair_n``, ``pair_med`` and ``pair_mad`` (uint64).
"""

import numpy as np

import pairwise_cases as pc

TS = (1, 2, 3, 63, 64, 65, 129, 1000)
KS = (2, 3, 4, 5, 23, 64)  # the smallest K with a third keypoint is 3; 4 and 5: two candidates without / with a keypoint outside; 64: the capacity
THR = pc.THR  # n_sigma = 6, the default, as prep.repair_swaps computes it
MIN_DEV = 0.002
MIN_BAD = 3


def distances(kp):
    """kp [T, 3K] float32 -> (d [T, P] float32, valid [T, P] bool): §14's distance of every pair and frame, operation by operation"""
    kp = np.asarray(kp, dtype=np.float32)
    T, K = kp.shape[0], kp.shape[1] // 3
    x = kp.reshape(T, K, 3)
    present = np.isfinite(x).all(axis=2)
    ab = np.array(pc.pairs(K), dtype=np.int64).reshape(-1, 2)
    A, B = ab[:, 0], ab[:, 1]
    with np.errstate(all="ignore"):
        dx, dy, dz = x[:, A, 0] - x[:, B, 0], x[:, A, 1] - x[:, B, 1], x[:, A, 2] - x[:, B, 2]
        d = np.sqrt((dx * dx + dy * dy) + dz * dz)
        assert d.dtype == np.float32
        valid = present[:, A] & present[:, B] & np.isfinite(d)
    return d, valid


def _pidx(i, j, K):
    return pc.pair_index(i, j, K) if i < j else pc.pair_index(j, i, K)


def _exchange(kp, cand, flag):
    """-> out: the three words of a and of b exchanged where flag[t, s]"""
    T, K = kp.shape[0], kp.shape[1] // 3
    out = np.array(kp, dtype=np.float32).reshape(T, K, 3)
    src = np.asarray(kp, dtype=np.float32).reshape(T, K, 3).view(np.uint32)
    w = out.view(np.uint32)
    for s, (a, b) in enumerate(cand):
        rows = flag[:, s] == 1
        w[rows, a] = src[rows, b]
        w[rows, b] = src[rows, a]
    return out.reshape(T, 3 * K)


def reference_swaps(kp, cand, thr, min_dev, min_bad, counts=False):
    """kp [T, 3K] float32, cand [(a, b)] -> (out [T, 3K] float32, flag [T, S] uint8, pair_n [P] int64, pair_med [P], pair_mad [P]
    float64); with ``counts`` also (b0 [T, S], b1 [T, S]) at the end.  A plain loop per candidate and frame."""
    kp = np.asarray(kp, dtype=np.float32)
    T, K = kp.shape[0], kp.shape[1] // 3
    S = len(cand)
    thr, min_dev = np.float64(thr), np.float64(min_dev)
    pair_n, pair_med, pair_mad = pc.reference_pairwise_all_pairs(kp, thr, min_dev, 1)[2:]
    d, valid = distances(kp)
    flag = np.zeros((T, S), np.uint8)
    B0, B1 = np.zeros((T, S), np.int64), np.zeros((T, S), np.int64)

    def bad(dist, p):  # bad(d; p): e = (float)|(double)d - med_p|; (double)e > thr * mad_p and (double)e > min_dev
        e = np.abs(dist.astype(np.float64) - pair_med[p]).astype(np.float32).astype(np.float64)
        return ((e > thr * pair_mad[p]) & (e > min_dev)).astype(np.int64)

    with np.errstate(all="ignore"):
        for s, (a, b) in enumerate(cand):
            ks = [k for k in range(K) if k not in (a, b)]
            pa = np.array([_pidx(a, k, K) for k in ks], dtype=np.int64)
            pb = np.array([_pidx(b, k, K) for k in ks], dtype=np.int64)
            enough = (pair_n[pa] >= 3) & (pair_n[pb] >= 3)
            for t in range(T):
                counted = enough & valid[t, pa] & valid[t, pb]
                if not counted.any():
                    continue
                qa, qb = pa[counted], pb[counted]
                da, db = d[t, qa], d[t, qb]
                b0 = int((bad(da, qa) + bad(db, qb)).sum())  # the frame as labelled
                b1 = int((bad(db, qa) + bad(da, qb)).sum())  # the frame with the labels exchanged
                B0[t, s], B1[t, s] = b0, b1
                if b0 >= min_bad and 2 * b1 <= b0:
                    flag[t, s] = 1
    res = (_exchange(kp, cand, flag), flag, pair_n, pair_med, pair_mad)
    return res + (B0, B1) if counts else res


def reference_swaps_all_frames(kp, cand, thr, min_dev, min_bad, counts=False):
    """``reference_swaps`` with the body of the loop over frames written for all frames at once (a loop per candidate is left): the
    same operations on the same values, a hundred times faster.  It is what ``reference`` hands to the tests;
    tests/test_swaps_host.py holds it against ``reference_swaps`` on every case, bit for bit."""
    kp = np.asarray(kp, dtype=np.float32)
    T, K = kp.shape[0], kp.shape[1] // 3
    S = len(cand)
    thr, min_dev = np.float64(thr), np.float64(min_dev)
    pair_n, pair_med, pair_mad = pc.reference_pairwise_all_pairs(kp, thr, min_dev, 1)[2:]
    d, valid = distances(kp)
    bound = thr * pair_mad
    B0, B1 = np.zeros((T, S), np.int64), np.zeros((T, S), np.int64)

    def bad(dist, p):
        e = np.abs(dist.astype(np.float64) - pair_med[p][None, :]).astype(np.float32).astype(np.float64)
        return (e > bound[p][None, :]) & (e > min_dev)

    with np.errstate(all="ignore"):
        for s, (a, b) in enumerate(cand):
            ks = [k for k in range(K) if k not in (a, b)]
            if not ks:
                continue
            pa = np.array([_pidx(a, k, K) for k in ks], dtype=np.int64)
            pb = np.array([_pidx(b, k, K) for k in ks], dtype=np.int64)
            counted = ((pair_n[pa] >= 3) & (pair_n[pb] >= 3))[None, :] & valid[:, pa] & valid[:, pb]
            da, db = d[:, pa], d[:, pb]
            B0[:, s] = ((bad(da, pa) & counted).astype(np.int64) + (bad(db, pb) & counted)).sum(axis=1)
            B1[:, s] = ((bad(db, pa) & counted).astype(np.int64) + (bad(da, pb) & counted)).sum(axis=1)
    flag = ((B0 >= min_bad) & (2 * B1 <= B0)).astype(np.uint8)
    res = (_exchange(kp, cand, flag), flag, pair_n, pair_med, pair_mad)
    return res + (B0, B1) if counts else res


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def cands_in_order(K):
    """K / 2 candidates (0, 1), (2, 3), ..."""
    return [(2 * i, 2 * i + 1) for i in range(K // 2)]


def cands_shuffled(K, rng):
    """K / 2 candidates over a permutation of the keypoints, each in either order"""
    perm = rng.permutation(K)
    return [(int(perm[2 * i]), int(perm[2 * i + 1])) for i in range(K // 2)]


def exchange_frames(x, cand, hit):
    """Exchanges, in x [T, K, 3] in place, the keypoints of candidate s in the frames where hit [T, S]"""
    for s, (a, b) in enumerate(cand):
        rows = np.flatnonzero(hit[:, s])
        x[rows[:, None], [a, b]] = x[rows[:, None], [b, a]]


def _random_swaps(x, cand, rng, share=0.15):
    hit = rng.random((x.shape[0], len(cand))) < share
    exchange_frames(x, cand, hit)
    return hit


def p_no_defect(x, rng):
    return dict(cand=cands_in_order(x.shape[1]))


def p_swaps(x, rng):  # 15 % of the frames of every candidate, K / 2 candidates
    cand = cands_shuffled(x.shape[1], rng)
    _random_swaps(x, cand, rng)
    return dict(cand=cand)


def p_one_reversed(x, rng):  # one candidate, the higher index first
    K = x.shape[1]
    cand = [(K - 1, K - 2)]
    _random_swaps(x, cand, rng)
    return dict(cand=cand)


def p_no_candidates(x, rng):  # S = 0: the swaps stay
    _random_swaps(x, cands_in_order(x.shape[1]), rng)
    return dict(cand=[])


def p_tile_edges(x, rng):  # swaps in the frames 63, 64, 65 and in the last frame, of one candidate each (the next one in turn)
    T, K = x.shape[:2]
    cand = cands_in_order(K)
    hit = np.zeros((T, len(cand)), bool)
    for i, t in enumerate((63, 64, 65, T - 1)):
        if t < T:
            hit[t, i % len(cand)] = True
    exchange_frames(x, cand, hit)
    return dict(cand=cand)


def p_swaps_missing(x, rng):  # swaps, then every keypoint missing in some frames by a NaN or an infinity in one coordinate
    cand = cands_shuffled(x.shape[1], rng)
    _random_swaps(x, cand, rng)
    pc.p_missing(x, rng)
    return dict(cand=cand)


def p_pair_counts(x, rng):  # pairs with n < 3 decide nothing and count for nobody
    cand = cands_in_order(x.shape[1])
    _random_swaps(x, cand, rng)
    pc.p_pair_counts(x, rng)
    return dict(cand=cand)


def p_huge(x, rng):  # present keypoints whose pairs are not valid
    cand = [(0, x.shape[1] - 1)] + [(2 * i - 1, 2 * i) for i in range(1, (x.shape[1] - 1) // 2)]
    _random_swaps(x, cand, rng)
    pc.p_huge(x, rng)
    return dict(cand=cand)


def p_identical(x, rng):  # mad = 0 for every pair: min_dev alone decides
    T = x.shape[0]
    cand = cands_in_order(x.shape[1])
    x[:] = x[0]
    hit = np.zeros((T, len(cand)), bool)
    hit[T // 2, 0] = True
    hit[T // 3, -1] = True
    exchange_frames(x, cand, hit)
    return dict(cand=cand)


def p_zeros_and_denormals(x, rng):  # keypoint 0 at -0.0 / +0.0 / denormals, exchanged with keypoint 1: the bits must move exactly
    cand = cands_in_order(x.shape[1])
    pc.p_zeros_and_denormals(x, rng)
    _random_swaps(x, cand, rng)
    return dict(cand=cand)


def _clear_swaps(x, rng):  # 15 % swaps of K / 2 candidates in a skeleton whose keypoints are far apart next to its noise
    cand = cands_in_order(x.shape[1])
    _random_swaps(x, cand, rng)
    return cand


def p_min_bad_1(x, rng):
    return dict(cand=_clear_swaps(x, rng), min_bad=1)


def p_min_bad_largest(x, rng):  # 2 (K - 2): the largest count there is
    return dict(cand=_clear_swaps(x, rng), min_bad=max(2 * (x.shape[1] - 2), 1))


def p_min_bad_never(x, rng):  # 2 (K - 2) + 1: no frame has that many
    return dict(cand=_clear_swaps(x, rng), min_bad=2 * (x.shape[1] - 2) + 1)


def p_ties(x, rng):  # displaced keypoints next to the swaps, so that b1 is not 0: some frame has 2 b1 == b0 > 0, some 2 b1 == b0 + 1
    cand = cands_in_order(x.shape[1])
    _random_swaps(x, cand, rng, share=0.3)
    pc._noise(x, rng, size=0.05, missing=0.02)
    return dict(cand=cand, min_bad=1)


# name -> (pattern, least T, least K) at which it holds what it is meant to; below that it does not fit the shape
PATTERNS = {
    "no_defect": (p_no_defect, 1, 2), "swaps": (p_swaps, 1, 2), "one_reversed": (p_one_reversed, 1, 2),
    "no_candidates": (p_no_candidates, 1, 2), "tile_edges": (p_tile_edges, 1, 2), "swaps_missing": (p_swaps_missing, 1, 2),
    "pair_counts": (p_pair_counts, 5, 3), "huge": (p_huge, 1, 3), "identical": (p_identical, 3, 3),
    "zeros_and_denormals": (p_zeros_and_denormals, 1, 2), "min_bad_1": (p_min_bad_1, 1, 2),
    "min_bad_largest": (p_min_bad_largest, 1, 2), "min_bad_never": (p_min_bad_never, 1, 2),
}  # fmt: skip
# the cases of the decision's edge: (name, T, K, seed) found by a search over seeds on the CPU (tests/test_swaps_host.py says how);
# make_case asserts that both frames occur
TIES = (("ties", 129, 5, 1), ("ties", 1000, 23, 1))


def _seed(name, T, K):
    return 1_000_000 * (list(PATTERNS).index(name) + 1) + 100 * T + K


def make_case(name, T, K):
    """-> (kp [T, 3K] float32, cand [(a, b)], thr, min_dev, min_bad)"""
    par = dict(thr=THR, min_dev=MIN_DEV, min_bad=MIN_BAD)
    if name == "ties":
        (seed,) = [sd for n, t, k, sd in TIES if (t, k) == (T, K)]
        rng = np.random.default_rng(seed)
        x = pc.skeleton(T, K, rng)
        par.update(p_ties(x, rng))
        kp = np.ascontiguousarray(x.reshape(T, 3 * K))
        b0, b1 = reference_swaps_all_frames(kp, par["cand"], par["thr"], par["min_dev"], par["min_bad"], counts=True)[5:]
        assert ((2 * b1 == b0) & (b0 > 0)).any() and (2 * b1 == b0 + 1).any(), ("ties: the seed no longer holds both frames", T, K, seed)
        return kp, par["cand"], par["thr"], par["min_dev"], par["min_bad"]
    rng = np.random.default_rng(_seed(name, T, K))
    x = pc.skeleton(T, K, rng)
    par.update(PATTERNS[name][0](x, rng) or {})
    return np.ascontiguousarray(x.reshape(T, 3 * K)), par["cand"], par["thr"], par["min_dev"], par["min_bad"]


def cases(ks=KS, ts=TS):
    """(name, T, K) of every case: every pattern that fits at every T x K of the grid, and the cases of the decision's edge"""
    grid = [(name, T, K) for K in ks for T in ts for name, (_, t_min, k_min) in PATTERNS.items() if T >= t_min and K >= k_min]
    return grid + [(name, T, K) for name, T, K, _ in TIES if K in ks and T in ts]


_REF = {}


def reference(name, T, K):
    """(kp, cand, thr, min_dev, min_bad, (out, flag, pair_n, pair_med, pair_mad)) of a case, computed once and shared (read-only)"""
    key = (name, T, K)
    if key not in _REF:
        kp, cand, thr, min_dev, min_bad = make_case(name, T, K)
        want = reference_swaps_all_frames(kp, cand, thr, min_dev, min_bad)
        for a in (kp, *want):
            a.setflags(write=False)
        _REF[key] = (kp, cand, thr, min_dev, min_bad, want)
    return _REF[key]


def check(got, kp, cand, want, label=""):
    """Tolerance 0 on the five outputs; where a candidate swaps its two keypoints are exchanged, every other element is the input's
    bits."""
    names = ("out", "flag", "pair_n", "pair_med", "pair_mad")
    dtypes = (np.float32, np.uint8, np.int64, np.float64, np.float64)
    for name, dt, g, w in zip(names, dtypes, got, want):
        g = np.asarray(g)
        assert g.dtype == dt and g.shape == w.shape, (label, name, g.dtype, g.shape, w.shape)
        bits = {4: np.uint32, 8: np.uint64, 1: np.uint8}[g.dtype.itemsize]
        np.testing.assert_array_equal(g.view(bits), w.view(bits), err_msg=f"{label} {name} (bits)")
    flag = want[1]
    T, K = np.asarray(kp).shape[0], np.asarray(kp).shape[1] // 3
    g, x = np.asarray(got[0]).reshape(T, K, 3).view(np.uint32), np.asarray(kp).reshape(T, K, 3).view(np.uint32)
    moved = np.zeros((T, K), bool)
    for s, (a, b) in enumerate(cand):
        rows = flag[:, s] == 1
        moved[rows, a] = moved[rows, b] = True
        np.testing.assert_array_equal(g[rows, a], x[rows, b], err_msg=f"{label} exchanged (bits)")
        np.testing.assert_array_equal(g[rows, b], x[rows, a], err_msg=f"{label} exchanged (bits)")
    np.testing.assert_array_equal(g[~moved], x[~moved], err_msg=f"{label} passed entries (bits)")
