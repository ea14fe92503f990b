"""Cases and reference of the fill_donors tests (tests/test_donor_host.py, tests/test_gpu_donor.py).

The reference is ``reference_donor``: the rule of DESIGN.md §17 in float64 with plain loops -- Python floats are IEEE doubles, every
operation below is one of + - * / in the order the rule states, and the one rounding to float32 happens at the end.  The kernel and
the CPU program built from csrc/stac_donor.hpp must equal it bit for bit: the tolerance is 0 on ``out`` (as bits), ``gap`` and ``src``.
``gap`` is ``prep_cases.reference_fill``'s: the same definition as ``fill_missing``'s.
"""

import numpy as np

import prep_cases as pc

TS = (1, 63, 64, 65, 129, 200)
KS = (4, 5, 23, 64)
DS = (1, 4, 8)
LEFT = 255  # src of a keypoint that is missing and left so


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _frame(A, B, C):
    """The frame of the donors at A, B, C (lists of three floats) -> (a, u, w, m, uu, ww, mm) or None if a squared length is not > 0."""
    u = [B[i] - A[i] for i in range(3)]
    v = [C[i] - A[i] for i in range(3)]
    uu = _dot(u, u)
    if not uu > 0.0:
        return None
    s = _dot(v, u) / uu
    w = [v[i] - s * u[i] for i in range(3)]
    ww = _dot(w, w)
    m = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
    mm = _dot(m, m)
    if not (ww > 0.0 and mm > 0.0):
        return None
    return A, u, w, m, uu, ww, mm


def _local(x, valid, f, k, a, b, c):
    """(alpha, beta, gamma) of keypoint k in the donors' frame in frame f, or None if a donor is missing there or there is no frame"""
    if not (valid[f, a] and valid[f, b] and valid[f, c]):
        return None
    F = _frame(x[f][a], x[f][b], x[f][c])
    if F is None:
        return None
    A, u, w, m, uu, ww, mm = F
    r = [x[f][k][i] - A[i] for i in range(3)]
    return [_dot(r, u) / uu, _dot(r, w) / ww, _dot(r, m) / mm]


def _try(x, valid, t, p, n, k, a, b, c):
    """One triple for the missing (t, k): the three float32 values, or None if the triple is not usable"""
    if not (valid[t, a] and valid[t, b] and valid[t, c]):
        return None
    F = _frame(x[t][a], x[t][b], x[t][c])
    if F is None:
        return None
    Lp = _local(x, valid, p, k, a, b, c) if p >= 0 else None
    Ln = _local(x, valid, n, k, a, b, c) if n >= 0 else None
    if (p >= 0 and Lp is None) or (n >= 0 and Ln is None):
        return None
    if p >= 0 and n >= 0:
        wgt = float(t - p) / float(n - p)
        L = [Lp[i] + (Ln[i] - Lp[i]) * wgt for i in range(3)]
    else:
        L = Lp if p >= 0 else Ln
    A, u, w, m = F[:4]
    with np.errstate(over="ignore", invalid="ignore"):
        o = np.array([((A[i] + L[0] * u[i]) + L[1] * w[i]) + L[2] * m[i] for i in range(3)], np.float64).astype(np.float32)  # the one rounding
    return o if np.isfinite(o).all() else None


def is_triple(k, K, row):
    a, b, c = (int(v) for v in row)
    return all(0 <= v < K for v in (a, b, c)) and len({a, b, c, k}) == 4


def reference_donor(kp, don):
    """kp [T, 3K] float32, don [K, D, 3] integers -> (out [T, 3K] float32, gap [T, K] int32, src [T, K] uint8) by the rule."""
    kp = np.asarray(kp, dtype=np.float32)
    don = np.asarray(don)
    T, K = kp.shape[0], kp.shape[1] // 3
    assert don.shape[0] == K and don.shape[2] == 3 and 1 <= don.shape[1] <= 8
    x3 = kp.reshape(T, K, 3)
    valid = np.isfinite(x3).all(axis=2)
    x = x3.astype(np.float64).tolist()  # (float32 -> float64 is exact; only entries of valid keypoints are ever read)
    out = x3.copy()
    src = np.zeros((T, K), np.uint8)
    gap = pc.reference_fill(kp, "linear")[1]
    for k in range(K):
        idx = np.flatnonzero(valid[:, k])
        for t in np.flatnonzero(~valid[:, k]).tolist():
            src[t, k] = LEFT
            if idx.size == 0:  # an empty track is left as it is
                continue
            at = int(np.searchsorted(idx, t))
            p = int(idx[at - 1]) if at > 0 else -1
            n = int(idx[at]) if at < idx.size else -1
            for d in range(don.shape[1]):
                if not is_triple(k, K, don[k, d]):
                    break  # the end of the list
                o = _try(x, valid, t, p, n, k, *(int(v) for v in don[k, d]))
                if o is not None:
                    out[t, k] = o
                    src[t, k] = d + 1
                    break
    return out.reshape(T, 3 * K), gap, src


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def base_series(T, K, seed):
    """A shape of K points that turns and drifts, with a little noise, plus the special values of ``prep_cases.base_series`` (-0.0,
    denormals, the largest float: a donor that holds one makes a triple overflow, which is one way of being unusable)."""
    rng = np.random.default_rng(seed)
    shape = rng.uniform(-0.05, 0.05, (K, 3))
    ang = np.linspace(0.0, 1.5, T)
    rot = np.stack([np.stack([np.cos(ang), -np.sin(ang), 0 * ang], 1), np.stack([np.sin(ang), np.cos(ang), 0 * ang], 1),
                    np.stack([0 * ang, 0 * ang, 1 + 0 * ang], 1)], 1)
    x = (np.einsum("tij,kj->tki", rot, shape) + np.linspace(0, 0.3, T)[:, None, None] + rng.standard_normal((T, K, 3)) * 1e-4).astype(np.float32)
    special = np.array([-0.0, 1e-45, -3e-41, 1.17549435e-38, 3.4028235e38, -3.4028235e38], np.float32)
    n = min(T * K * 3, special.size)
    x.reshape(-1)[rng.choice(T * K * 3, size=n, replace=False)] = special[:n]
    return x


def default_table(K, D):
    """Row d of keypoint k: three consecutive ones of the other keypoints, starting at the d-th (K >= 4: always a triple)."""
    don = np.zeros((K, D, 3), np.int32)
    for k in range(K):
        others = [j for j in range(K) if j != k]
        for d in range(D):
            don[k, d] = [others[(d + i) % len(others)] for i in range(3)]
    return don


def _span(x, k, lo, hi, value=np.nan):
    T = x.shape[0]
    lo, hi = max(lo, 0), min(hi, T - 1)
    if lo <= hi:
        x[lo:hi + 1, k, :] = value


def p_none(x, don, rng):
    pass


def p_random_holes(x, don, rng):
    """runs of geometric length (mean 6) that start at 4 % of the (frame, keypoint)s"""
    T, K = x.shape[:2]
    for t, k in zip(*np.nonzero(rng.random((T, K)) < 0.04)):
        _span(x, k, t, t + int(rng.geometric(1 / 6.0)) - 1)


def p_tile_borders(x, don, rng):
    """a run that crosses the border of the first tile, one longer than two tiles, one that ends on a tile's last frame"""
    K = x.shape[1]
    _span(x, 0, 60, 70)
    _span(x, K - 1, 10, 150)
    _span(x, 1, 120, 127)
    _span(x, 2, 64, 64)


def p_leading_trailing(x, don, rng):
    T, K = x.shape[:2]
    _span(x, 0, 0, min(5, T - 2))
    _span(x, 1, max(T - 4, 1), T - 1)
    if T >= 3:  # both on one track
        _span(x, K - 1, 0, 0)
        _span(x, K - 1, T - 1, T - 1)


def p_empty_track(x, don, rng):
    """track 2 has no valid frame (and is a donor of others); track 0 has a hole"""
    x[:, 2, :] = np.nan
    _span(x, 0, 3, 6)


def p_donor_missing(x, don, rng):
    """keypoint 0 has three runs; its first donor (keypoint 1, in row 0 only where K >= 5) is missing inside the first run only (frame
    7: that frame falls through to row 1), at the p of the second (19) and at the n of the third (45)"""
    K, D = don.shape[:2]
    don[0, 0] = (1, 2, 3)
    if D > 1:
        don[0, 1] = (2, 3, 4) if K >= 5 else (3, 2, 1)
    _span(x, 0, 5, 9)
    _span(x, 0, 20, 24)
    _span(x, 0, 40, 44)
    for t in (7, 19, 45):
        _span(x, 1, t, t)


def p_all_unusable(x, don, rng):
    """frame 3: every keypoint missing (no donor at t); keypoint 0 is also missing 10 .. 12 while all its donors are missing at 9, its p"""
    K = x.shape[1]
    _span(x, 0, 3, 3)
    for k in range(1, K):
        _span(x, k, 3, 3)
        _span(x, k, 9, 9)
    _span(x, 0, 10, 12)


def p_degenerate(x, don, rng):
    """keypoint 0's list: coincident donors (uu == 0), then donors that are exactly collinear on integer coordinates (ww == 0), then,
    where K >= 7, a good row"""
    K, D = don.shape[:2]
    x[:, 1] = x[:, 2] = (1.0, 2.0, 3.0)
    x[:, 3] = (2.0, 4.0, 6.0)
    if K >= 5:
        x[:, 4] = (3.0, 6.0, 9.0)
    rows = [(1, 2, 3), (1, 3, 4) if K >= 5 else (1, 3, 2), (4, 5, 6) if K >= 7 else (-1, -1, -1)]
    for d in range(D):
        don[0, d] = rows[d] if d < len(rows) else (-1, -1, -1)
    _span(x, 0, 2, 4)
    _span(x, 0, 62, 66)


def p_mutual(x, don, rng):
    """keypoints 0 and 1 are missing in the same frames and name each other in row 0; row 1 names neither"""
    K, D = don.shape[:2]
    don[0, 0] = (1, 2, 3)
    don[1, 0] = (0, 2, 3)
    if D > 1 and K >= 5:
        don[0, 1] = don[1, 1] = (2, 3, 4)
    for k in (0, 1):
        _span(x, k, 4, 8)
        _span(x, k, 61, 67)


def p_infinities(x, don, rng):
    T, K = x.shape[:2]
    x[T // 3, 0, 0] = np.inf
    x[(2 * T) // 3, 0, 2] = -np.inf
    x[T // 2, K - 1, 1] = -np.inf
    _span(x, 1, T // 2, T // 2 + 1, np.inf)
    _span(x, 2, T // 3, T // 3, -np.inf)  # a donor of keypoint 0 in the frame where 0 is missing


def p_table_ends(x, don, rng):
    """rows that end a list: an index out of range (K, -1, the ends of int32), a repeated index, the keypoint itself; keypoint 3 has a
    good row 0, the end in row 1 and a good row behind it that is never reached"""
    K, D = don.shape[:2]
    don[0, 0] = (1, 2, K)
    don[1, 0] = (0, 0, 2)
    don[2, 0] = (2, 3, 0)
    if D > 1:
        don[3, 1] = (-1, -1, -1)
    if K >= 5:
        don[4, 0] = (2**31 - 1, 1, 2)
    if K >= 6:
        don[5, 0] = (1, -2**31, 2)
    for k in range(min(K, 6)):
        _span(x, k, 5 + 8 * k, 9 + 8 * k)
    _span(x, 0, 60, 61)   # row 0 of keypoint 3 is unusable here (its donor 0 is missing at t) and row 1 is the end
    _span(x, 3, 60, 61)


PATTERNS = {
    "none": p_none, "random_holes": p_random_holes, "tile_borders": p_tile_borders, "leading_trailing": p_leading_trailing,
    "empty_track": p_empty_track, "donor_missing": p_donor_missing, "all_unusable": p_all_unusable, "degenerate": p_degenerate,
    "mutual": p_mutual, "infinities": p_infinities, "table_ends": p_table_ends,
}  # fmt: skip


def make_case(pattern, T, K, D):
    """-> (kp [T, 3K] float32, don [K, D, 3] int32)"""
    seed = 1000 * list(PATTERNS).index(pattern) + 7 * T + 3 * K + D
    x = base_series(T, K, seed)
    don = default_table(K, D)
    PATTERNS[pattern](x, don, np.random.default_rng(seed + 1))
    return np.ascontiguousarray(x.reshape(T, 3 * K)), don


def case_list():
    """(pattern, T, K, D): every pattern at every T, with K and D rotating so that every pattern meets every K and every D, and the
    random holes over the whole K x D grid at two tiles and a frame and over the whole T x K grid."""
    out = []
    for i, name in enumerate(PATTERNS):
        for j, T in enumerate(TS):
            out.append((name, T, KS[(i + j) % len(KS)], DS[(i + j) % len(DS)]))
    for K in KS:
        for D in DS:
            out.append(("random_holes", 129, K, D))
        for T in TS:
            out.append(("random_holes", T, K, 4))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


CASES = case_list()
_REF = {}


def reference(pattern, T, K, D):
    """(kp, don, out, gap, src) of a case, computed once and shared (read-only) among the tests"""
    key = (pattern, T, K, D)
    if key not in _REF:
        kp, don = make_case(pattern, T, K, D)
        res = (kp, don) + reference_donor(kp, don)
        for a in res:
            a.setflags(write=False)
        _REF[key] = res
    return _REF[key]


def check(got_out, got_gap, got_src, kp, want_out, want_gap, want_src, label=""):
    """Tolerance 0: ``gap`` and ``src`` equal, ``out`` equal by bit pattern everywhere (what stays missing keeps the input's words)."""
    got_out, got_gap, got_src = np.asarray(got_out), np.asarray(got_gap), np.asarray(got_src)
    assert got_out.dtype == np.float32 and got_out.shape == want_out.shape, (label, got_out.dtype, got_out.shape)
    assert got_gap.dtype == np.int32 and got_gap.shape == want_gap.shape, (label, got_gap.dtype, got_gap.shape)
    assert got_src.dtype == np.uint8 and got_src.shape == want_src.shape, (label, got_src.dtype, got_src.shape)
    np.testing.assert_array_equal(got_src, want_src, err_msg=f"{label} src")
    np.testing.assert_array_equal(got_gap, want_gap, err_msg=f"{label} gap")
    np.testing.assert_array_equal(got_out.view(np.uint32), want_out.view(np.uint32), err_msg=f"{label} out (bits)")
    T, K = want_src.shape
    same = np.repeat((want_src == 0) | (want_src == LEFT), 3, axis=1)
    np.testing.assert_array_equal(got_out.view(np.uint32)[same], np.asarray(kp).view(np.uint32)[same], err_msg=f"{label} passed through (bits)")


# ---- what it is worth: the series of the issue's two measurements ------------------------------------------------------------------
def linear_fill(kp):
    return pc.reference_fill(kp, "linear")[0]


def rigid_series(T=300, K=6, seed=5):
    """A rigid shape of 6 points in +-0.05 that turns 0.83 rad per 40 frames about a tilted axis and drifts, float32"""
    rng = np.random.default_rng(seed)
    shape = rng.uniform(-0.05, 0.05, (K, 3))
    axis = np.array([0.3, -0.5, 0.81])
    axis /= np.linalg.norm(axis)
    kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    out = np.zeros((T, K, 3))
    for t in range(T):
        a = 0.83 * t / 40.0
        rot = np.eye(3) + np.sin(a) * kx + (1 - np.cos(a)) * (kx @ kx)
        out[t] = shape @ rot.T + np.array([0.002, -0.001, 0.0005]) * t
    return out.astype(np.float32).reshape(T, 3 * K)


def punch(kp, k, starts, length):
    """A copy of kp with keypoint k missing in ``length`` frames from every start that leaves a valid frame behind the hole"""
    x = kp.copy().reshape(kp.shape[0], -1, 3)
    holes = np.zeros(x.shape[:2], bool)
    for s in starts:
        if s + length < x.shape[0]:
            x[s:s + length, k] = np.nan
            holes[s:s + length, k] = True
    return x.reshape(kp.shape), holes
