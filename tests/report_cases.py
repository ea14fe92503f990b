"""The fit report (DESIGN.md "Fit report"): a numpy float64 reference of the rule and the cases that tests/test_report_host.py (the
passes of csrc/stac_report.hip stated on the CPU) and tests/test_gpu_report.py (the kernels) share.  Every array is read-only."""

import functools
import math

import numpy as np

NAN_BITS = 0x7FC00000
KS = (1, 2, 23, 70)
PERMILLE = {1: (1000,), 3: (0, 500, 1000), 8: (0, 1, 250, 500, 900, 990, 999, 1000)}
PATTERNS = ("zero_residual", "one_counted", "none_counted", "nonfinite_each_slot", "gap_excluded", "low_bits_only", "mid_bits_only",
            "exponent_spread", "rank_inside_a_tie", "argmax_tie", "random")
EXACT = ("sqerr", "frame_sse", "frame_n", "count", "max", "argmax", "hist", "quant")


def shapes_N(tile):
    return [1, 2, 3, tile - 1, tile, tile + 1, 2 * tile + 1, 5 * tile + 7]


def n_quant_of(name, K):
    """Which of the three permille sets a (pattern, K) runs with: every pattern meets every set over the four K."""
    return (1, 3, 8)[(PATTERNS.index(name) + KS.index(K)) % 3] if K in KS else 3


def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def reference_report(markers, kp, gap, permille):
    """The rule in numpy float64: plain loops per keypoint over the counted frames, ``np.sort`` of the bit patterns, integer rank
    arithmetic, ``math.fsum`` for ``sum`` and a sequential loop over the keypoints for ``frame_sse``."""
    markers = np.asarray(markers, np.float32)
    N, K = markers.shape[:2]
    y = np.asarray(kp, np.float32).reshape(N, K, 3)
    g = np.zeros((N, K), np.int32) if gap is None else np.asarray(gap, np.int32)
    with np.errstate(all="ignore"):
        d = markers.astype(np.float64) - y.astype(np.float64)
        e = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]  # left to right, every operation rounded once
        finite = np.isfinite(markers).all(axis=2) & np.isfinite(y).all(axis=2)
        sqerr = e.astype(np.float32)  # one rounding; above FLT_MAX: +inf
    sqerr.view(np.uint32)[~finite] = NAN_BITS
    counted = finite & (g == 0)
    frame_n = counted.sum(axis=1).astype(np.int32)
    frame_sse = np.zeros(N, np.float64)
    for k in range(K):  # ascending k, sequentially from +0.0 (each frame's sum is its own chain)
        frame_sse = np.where(counted[:, k], frame_sse + np.where(counted[:, k], e[:, k], 0.0), frame_sse)
    Q = len(permille)
    count = np.zeros(K, np.int64)
    total = np.zeros(K, np.float64)
    mx = np.full(K, NAN_BITS, np.uint32)
    argmax = np.full(K, -1, np.int64)
    hist = np.zeros((K, 1024), np.int64)
    quant = np.full((K, Q), NAN_BITS, np.uint32)
    bits = sqerr.view(np.uint32)
    for k in range(K):
        frames = np.flatnonzero(counted[:, k])
        n = count[k] = len(frames)
        total[k] = math.fsum(e[frames, k].tolist())
        if n == 0:
            continue
        b = bits[frames, k]
        assert (b <= 0x7F800000).all()  # non-negative, never -0.0, never NaN: the bit patterns order like the values
        s = np.sort(b)
        mx[k] = s[-1]
        argmax[k] = frames[np.flatnonzero(b == s[-1])[0]]
        hist[k] = np.bincount(b >> 21, minlength=1024)
        for q, p in enumerate(permille):
            quant[k, q] = s[(int(p) * (int(n) - 1)) // 1000]
    out = {"sqerr": sqerr, "frame_sse": frame_sse, "frame_n": frame_n, "count": count, "sum": total, "max": mx.view(np.float32),
           "argmax": argmax, "hist": hist, "quant": quant.view(np.float32)}
    _freeze(*out.values())
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def check(got, want, label=""):
    """Tolerance 0, floats as bit patterns, for everything but ``sum``: |sum - fsum| <= count * 2^-52 * fsum (twice the first-order
    bound of recursive summation of non-negative terms in any order); a non-finite fsum must be met exactly."""
    for name in EXACT:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.shape == w.shape and g.dtype == w.dtype, (label, name, g.shape, w.shape, g.dtype, w.dtype)
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{label}: {name}")
    g, w, n = np.asarray(got["sum"], np.float64), want["sum"], want["count"]
    assert g.shape == w.shape
    for k in range(len(w)):
        if not math.isfinite(w[k]):
            assert g[k] == w[k], (label, "sum", k, g[k], w[k])
        else:
            assert abs(g[k] - w[k]) <= float(n[k]) * 2.0 ** -52 * w[k], (label, "sum", k, g[k], w[k], int(n[k]))


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def _base(N, K, seed):
    rng = np.random.default_rng(seed)
    kp = (0.05 * rng.standard_normal((N, K, 3))).astype(np.float32)
    return rng, kp


def _noise(rng, N, K, scale=0.001):
    return (scale * rng.standard_normal((N, K, 3))).astype(np.float32)


def tie_frames(N, tile, k):
    """Frames of the ``argmax_tie`` maximum of keypoint k: in different tiles where N has them; odd keypoints start later."""
    want = (3, tile + 5, 3 * tile + 1) if k % 2 == 0 else (tile + 5, 3 * tile + 1, 4 * tile + 2)
    frames = [t for t in want if t < N]
    return frames or [N - 1]


def one_counted_frame(N, k):
    return (0, N // 2, N - 1)[k % 3]


@functools.lru_cache(maxsize=None)
def case(name, N, K, tile):
    """-> (markers [N, K, 3] float32, kp [N, 3K] float32, gap [N, K] int32 or None)"""
    rng, kp = _base(N, K, 1000 * PATTERNS.index(name) + 7 * N + K)
    gap = None
    if name == "zero_residual":
        m = kp.copy()
    elif name == "one_counted":
        m = kp + _noise(rng, N, K)
        gap = np.zeros((N, K), np.int32)
        for k in range(K):
            keep = one_counted_frame(N, k)
            if k % 2:
                gap[:, k] = 5
                gap[keep, k] = 0
            else:
                saved = kp[keep, k].copy()
                kp[:, k, k % 3] = np.nan
                kp[keep, k] = saved
    elif name == "none_counted":
        m = kp + _noise(rng, N, K)
        gap = np.zeros((N, K), np.int32)
        kp[:, 0, :] = np.nan
        if K > 1:
            gap[:, K - 1] = N
    elif name == "nonfinite_each_slot":
        m = kp + _noise(rng, N, K)
        i = 0
        for bad in (np.nan, np.inf, -np.inf):
            for slot in range(6):
                p = (5 * i + 1) % (N * K)
                (m if slot < 3 else kp)[p // K, p % K, slot % 3] = bad
                i += 1
    elif name == "gap_excluded":
        m = kp + _noise(rng, N, K)
        holes = rng.random((N, K)) < 0.1
        holes.flat[(N * K) // 2] = True
        gap = np.where(holes, 3, 0).astype(np.int32)
        m[holes] += np.float32(1.0)
    elif name in ("low_bits_only", "mid_bits_only"):
        kp[:] = 0.0
        m = np.zeros((N, K, 3), np.float32)
        if name == "low_bits_only":  # x = 1 + j 2^-23: x^2 rounds to 1 + 2 j 2^-23, 2 j < 1024
            m[..., 0] = np.float32(1.0) + rng.integers(0, 512, (N, K)).astype(np.float32) * np.float32(2.0 ** -23)
        else:  # x^2 in [1, 1.2321): one quarter-octave bin
            m[..., 0] = (1.0 + 0.11 * rng.random((N, K))).astype(np.float32)
    elif name == "exponent_spread":
        kp[:] = 0.0
        m = np.zeros((N, K, 3), np.float32)
        i = np.arange(N * K).reshape(N, K)
        m[..., 2] = (10.0 ** (-22.0 + 52.0 * ((i * 37) % 1009) / 1008.0)).astype(np.float32)
    elif name == "rank_inside_a_tie":
        kp[:] = 0.0
        m = np.zeros((N, K, 3), np.float32)
        levels = np.concatenate([np.full(N // 3, 0.5), np.full(N // 3, 1.5), np.full(N - 2 * (N // 3), 2.5)]).astype(np.float32)
        for k in range(K):
            m[:, k, 1] = rng.permutation(levels)
    elif name == "argmax_tie":
        m = kp + _noise(rng, N, K)
        for k in range(K):
            for t in tie_frames(N, tile, k):
                kp[t, k] = 0.0  # (so that the residual is the same in every frame to the bit)
                m[t, k] = np.array([0.25, -0.5, 0.125], np.float32)
    elif name == "random":
        m = kp + _noise(rng, N, K)
        gap = np.where(rng.random((N, K)) < 0.03, 2, 0).astype(np.int32)
    else:
        raise KeyError(name)
    m = np.ascontiguousarray(m, np.float32)
    kp2 = np.ascontiguousarray(kp.reshape(N, 3 * K), np.float32)
    return _freeze(m, kp2, gap)


@functools.lru_cache(maxsize=None)
def reference(name, N, K, tile, Q):
    """-> (markers, kp, gap, permille, the reference's outputs) of a case; computed once and shared"""
    m, kp, gap = case(name, N, K, tile)
    return m, kp, gap, PERMILLE[Q], reference_report(m, kp, gap, PERMILLE[Q])


def all_cases(tile):
    """Every (pattern, N, K, Q) of the GPU test"""
    return [(name, N, K, n_quant_of(name, K)) for N in shapes_N(tile) for K in KS for name in PATTERNS]
