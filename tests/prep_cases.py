"""Cases and reference of the fill_missing tests (tests/test_prep_host.py, tests/test_gpu_prep.py).

The reference is ``reference_fill``: numpy float64, written from the rule of DESIGN.md §10 with plain loops per track over
``np.flatnonzero(valid)``; its one float32 rounding happens at the end.  Every operation of the rule is a correctly rounded IEEE
double operation on exactly converted integers and floats, so the kernel (and the CPU statement of its staged scan) must equal it
bit for bit: the tolerance is 0 on ``out`` and on ``gap``.
"""

import numpy as np

MODES = ("linear", "hold")
KS = (1, 2, 23, 70)


def shapes_T(tile):
    """The frame counts of the issue for a tile of ``tile`` frames (without repeats, in order)."""
    out = []
    for T in (1, 2, 3, tile - 1, tile, tile + 1, 2 * tile + 1, 5 * tile + 7):
        if T >= 1 and T not in out:
            out.append(T)
    return out


def reference_fill(kp, mode):
    """kp [T, 3K] float32 -> (out [T, 3K] float32, gap [T, K] int32) by the rule, in float64."""
    assert mode in MODES
    kp = np.asarray(kp, dtype=np.float32)
    T, K = kp.shape[0], kp.shape[1] // 3
    x = kp.reshape(T, K, 3)
    valid = np.isfinite(x).all(axis=2)
    out = x.astype(np.float64)
    gap = np.zeros((T, K), np.int32)
    for k in range(K):
        idx = np.flatnonzero(valid[:, k])
        if idx.size == 0:  # an empty track is left as it is
            gap[:, k] = T
            continue
        first, last = int(idx[0]), int(idx[-1])
        for t in range(0, first):  # leading run: copy n
            out[t, k] = out[first, k]
            gap[t, k] = first
        for t in range(last + 1, T):  # trailing run: copy p
            out[t, k] = out[last, k]
            gap[t, k] = T - 1 - last
        for p, n in zip(idx[:-1].tolist(), idx[1:].tolist()):
            for t in range(p + 1, n):
                gap[t, k] = n - p - 1
                for c in range(3):
                    a, b = np.float64(x[p, k, c]), np.float64(x[n, k, c])
                    if mode == "linear":
                        w = np.float64(t - p) / np.float64(n - p)
                        out[t, k, c] = a + (b - a) * w
                    else:
                        out[t, k, c] = a if (t - p) <= (n - t) else b
    res = out.astype(np.float32)  # the one rounding
    assert np.array_equal(res[valid].view(np.uint32), x[valid].view(np.uint32))  # (float32 -> float64 -> float32 is exact)
    return res.reshape(T, 3 * K), gap


def base_series(T, K, seed):
    """Finite float32 data with a few values whose bits a careless copy would change (-0.0, denormals, the largest float)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, K, 3)) * np.float32(0.05) + rng.standard_normal((1, K, 3))).astype(np.float32)
    special = np.array([-0.0, 1e-45, -3e-41, 1.17549435e-38, 3.4028235e38, -3.4028235e38], np.float32)
    n = min(T * K * 3, 2 * special.size)
    at = rng.choice(T * K * 3, size=n, replace=False)
    x.reshape(-1)[at] = np.resize(special, n)
    return x


def _span(x, k, lo, hi, value=np.nan):
    """frames lo .. hi (inclusive, clipped to the series) of track k missing"""
    T = x.shape[0]
    lo, hi = max(lo, 0), min(hi, T - 1)
    if lo <= hi:
        x[lo:hi + 1, k, :] = value


def _only(x, k, t):
    """track k valid in frame t alone"""
    keep = x[t, k].copy()
    x[:, k, :] = np.nan
    x[t, k] = keep


def p_none(x, tile, rng):
    pass


def p_empty_track(x, tile, rng):
    x[:, x.shape[1] // 2, :] = np.nan  # (K >= 3: between two good ones)


def p_single_valid_start(x, tile, rng):
    _only(x, 0, 0)


def p_single_valid_middle(x, tile, rng):
    _only(x, x.shape[1] - 1, x.shape[0] // 2)


def p_single_valid_end(x, tile, rng):
    _only(x, 0, x.shape[0] - 1)


def p_leading_and_trailing(x, tile, rng):
    T, K = x.shape[:2]
    _span(x, 0, 0, min(2, T - 2))
    _span(x, K - 1, max(T - 4, 1), T - 1)
    if T >= 3:  # both on one track
        _span(x, K // 2, 0, 0)
        _span(x, K // 2, T - 1, T - 1)


def p_run_ends_on_last_frame_of_tile(x, tile, rng):
    _span(x, 0, tile - 3, tile - 1)
    _span(x, x.shape[1] - 1, 2 * tile - 1, 2 * tile - 1)


def p_run_starts_on_first_frame_of_tile(x, tile, rng):
    _span(x, 0, tile, tile + 2)
    _span(x, x.shape[1] - 1, 2 * tile, 2 * tile)


def p_run_over_three_tiles(x, tile, rng):
    _span(x, 0, tile, 4 * tile + min(2, tile - 1))  # tiles 1, 2, 3 whole, ends inside tile 4
    _span(x, x.shape[1] - 1, tile - 1, 4 * tile)    # one frame more on both sides


def p_alternating(x, tile, rng):
    x[1::2, 0, :] = np.nan
    x[0::2, x.shape[1] - 1, :] = np.nan


def p_only_y_nan(x, tile, rng):
    T = x.shape[0]
    for t in (1, tile, T - 2):
        if 0 <= t < T:
            x[t, 0, 1] = np.nan
    x[T // 2, x.shape[1] - 1, 1] = np.nan


def p_infinities(x, tile, rng):
    T, K = x.shape[:2]
    x[T // 3, 0, 0] = np.inf
    x[(2 * T) // 3, 0, 2] = -np.inf
    x[T // 2, K - 1, 1] = -np.inf
    _span(x, K // 2, T // 2, T // 2 + 1, np.inf)


def p_hold_tie(x, tile, rng):
    _span(x, 0, 1, 3)                    # p = 0, n = 4: frame 2 is as far from both
    _span(x, x.shape[1] - 1, tile - 2, tile + 2)  # five frames across a tile border, the tie on the border
    _span(x, x.shape[1] // 2, 2, 2)      # length 1


def p_random_30_percent(x, tile, rng):
    x[rng.random(x.shape[:2]) < 0.3] = np.nan


PATTERNS = {
    "none": p_none, "empty_track": p_empty_track, "single_valid_start": p_single_valid_start,
    "single_valid_middle": p_single_valid_middle, "single_valid_end": p_single_valid_end,
    "leading_and_trailing": p_leading_and_trailing, "run_ends_on_last_frame_of_tile": p_run_ends_on_last_frame_of_tile,
    "run_starts_on_first_frame_of_tile": p_run_starts_on_first_frame_of_tile, "run_over_three_tiles": p_run_over_three_tiles,
    "alternating": p_alternating, "only_y_nan": p_only_y_nan, "infinities": p_infinities, "hold_tie": p_hold_tie,
    "random_30_percent": p_random_30_percent,
}  # fmt: skip


def make_case(pattern, T, K, tile):
    """-> kp [T, 3K] float32 with the pattern's holes; ``tile`` places the runs that are about tile borders"""
    seed = 1000 * list(PATTERNS).index(pattern) + 7 * T + K
    x = base_series(T, K, seed)
    PATTERNS[pattern](x, tile, np.random.default_rng(seed + 1))
    return np.ascontiguousarray(x.reshape(T, 3 * K))


_REF = {}


def reference(pattern, T, K, tile, mode):
    """(kp, out, gap) of a case, computed once and shared (read-only) among the tests"""
    key = (pattern, T, K, tile, mode)
    if key not in _REF:
        kp = make_case(pattern, T, K, tile)
        out, gap = reference_fill(kp, mode)
        for a in (kp, out, gap):
            a.setflags(write=False)
        _REF[key] = (kp, out, gap)
    return _REF[key]


def check(got_out, got_gap, kp, want_out, want_gap, label=""):
    """Tolerance 0: ``gap`` equal; ``out`` equal by bit pattern on every track that has a valid frame (valid entries are the
    input's bits, filled entries the reference's); an empty track keeps its NaNs and infinities where they were."""
    got_out, got_gap = np.asarray(got_out), np.asarray(got_gap)
    assert got_out.dtype == np.float32 and got_out.shape == want_out.shape, (label, got_out.dtype, got_out.shape)
    assert got_gap.dtype == np.int32 and got_gap.shape == want_gap.shape, (label, got_gap.dtype, got_gap.shape)
    np.testing.assert_array_equal(got_gap, want_gap, err_msg=f"{label} gap")
    T, K = want_gap.shape
    g, w, x = got_out.reshape(T, K, 3), want_out.reshape(T, K, 3), np.asarray(kp).reshape(T, K, 3)
    valid = np.isfinite(x).all(axis=2)
    empty = ~valid.any(axis=0)
    np.testing.assert_array_equal(g[:, ~empty].view(np.uint32), w[:, ~empty].view(np.uint32), err_msg=f"{label} out (bits)")
    np.testing.assert_array_equal(g[valid].view(np.uint32), x[valid].view(np.uint32), err_msg=f"{label} valid entries (bits)")
    assert np.isfinite(g[:, ~empty]).all(), label
    if empty.any():
        e, xe = g[:, empty], x[:, empty]
        np.testing.assert_array_equal(np.isnan(e), np.isnan(xe), err_msg=f"{label} empty track NaN")
        np.testing.assert_array_equal(np.isposinf(e), np.isposinf(xe), err_msg=f"{label} empty track +inf")
        np.testing.assert_array_equal(np.isneginf(e), np.isneginf(xe), err_msg=f"{label} empty track -inf")
        fin = np.isfinite(xe)
        np.testing.assert_array_equal(e[fin].view(np.uint32), xe[fin].view(np.uint32), err_msg=f"{label} empty track finite")
