"""Cases and reference of the reject_outliers tests (tests/test_outlier_host.py, tests/test_gpu_outlier.py).

The reference is ``reference_reject``: numpy float64, written from the rule of DESIGN.md §11 with plain loops per track, coordinate
and frame: ``np.sort`` of the valid window values and the expressions of the rule written out (no ``np.median``, no scipy).  The rule
is comparisons plus five IEEE double operations per coordinate, so the kernel (and the CPU program built from its header) must equal
it bit for bit: the tolerance is 0 on ``out`` (compared as uint32 words) and on ``flag``.
"""

import numpy as np

HS = (1, 5, 16)
KS = (1, 2, 23, 70)
THR = 3.0 * 1.4826  # n_sigma = 3, the identifier's conventional value, as prep.reject_outliers computes it
QNAN = np.uint32(0x7FC00000)


def shapes_T(h, tile):
    """The frame counts of the issue for half-width ``h`` and a tile of ``tile`` frames (without repeats, in order)."""
    out = []
    for T in (1, 2, h, h + 1, 2 * h + 1, tile - 1, tile, tile + 1, 2 * tile + 1, 5 * tile + 7):
        if T >= 1 and T not in out:
            out.append(T)
    return out


def reference_reject(kp, h, thr, min_dev):
    """kp [T, 3K] float32 -> (out [T, 3K] float32, flag [T, K] uint8) by the rule, in float64."""
    kp = np.asarray(kp, dtype=np.float32)
    T, K = kp.shape[0], kp.shape[1] // 3
    x = kp.reshape(T, K, 3)
    valid = np.isfinite(x).all(axis=2)
    thr, min_dev, half = np.float64(thr), np.float64(min_dev), np.float64(0.5)
    flag = np.zeros((T, K), np.uint8)
    with np.errstate(all="ignore"):
        for k in range(K):
            vk = valid[:, k]
            for c in range(3):
                col = x[:, k, c]
                for t in range(T):
                    if not vk[t]:
                        continue
                    lo, hi = max(0, t - h), min(T - 1, t + h)
                    w = col[lo:hi + 1][vk[lo:hi + 1]]
                    n = w.size
                    if n < 3:
                        continue
                    s = np.sort(w)
                    med = half * (np.float64(s[(n - 1) // 2]) + np.float64(s[n // 2]))
                    D = np.sort(np.abs(w.astype(np.float64) - med))
                    mad = half * (D[(n - 1) // 2] + D[n // 2])
                    dc = np.abs(np.float64(col[t]) - med)
                    if dc > thr * mad and dc > min_dev:
                        flag[t, k] = 1
    out = np.array(kp).reshape(T, K, 3)
    assert not (flag.astype(bool) & ~valid).any()  # only a keypoint that is not missing can be rejected
    out.view(np.uint32)[flag == 1] = QNAN
    return out.reshape(T, 3 * K), flag


def smooth_track(T, rng, noise=0.002):
    """[T, 3] float32: a slow movement (a few cm over hundreds of frames) plus white noise of ``noise``"""
    t = np.arange(T, dtype=np.float64)[:, None]
    phase, freq = rng.uniform(0, 2 * np.pi, (1, 3)), rng.uniform(0.002, 0.01, (1, 3))
    return (rng.uniform(-0.3, 0.3, (1, 3)) + 0.05 * np.sin(freq * t * 2 * np.pi + phase) + noise * rng.standard_normal((T, 3))).astype(np.float32)


def _at(x, frames):
    T = x.shape[0]
    return sorted({int(t) for t in frames if 0 <= int(t) < T})


def _spike(x, frames, rng, coords=(0, 1, 2), size=0.25):
    for t in _at(x, frames):
        for c in coords:
            x[t, c] += np.float32(size * rng.choice((-1.0, 1.0)) * rng.uniform(0.5, 1.5))


# ---- the patterns: each works on one track x [T, 3] in place --------------------------------------------------------------------
def p_smooth(x, h, tile, rng):
    pass


def p_spikes_at_edges_and_tile_borders(x, h, tile, rng):
    _spike(x, (0, x.shape[0] - 1, tile - 1, tile), rng)


def p_spikes_random(x, h, tile, rng):
    _spike(x, np.flatnonzero(rng.random(x.shape[0]) < 0.05), rng)


def p_run_of_h(x, h, tile, rng):  # a run of wrong values of h frames: every one of them is a minority of its window
    t = max(0, min(tile - h // 2, x.shape[0] - h - 2))
    x[t:t + h] += np.float32(0.3)


def p_run_of_h_plus_1(x, h, tile, rng):  # h + 1 frames: the known limit, the frames in the middle are their window's majority
    t = max(0, min(tile - h // 2, x.shape[0] - h - 3))
    x[t:t + h + 1] += np.float32(0.3)


def p_spike_in_one_coordinate(x, h, tile, rng):
    _spike(x, (1, x.shape[0] // 2, tile, x.shape[0] - 2), rng, coords=(1,))


def p_spikes_next_to_nan_runs(x, h, tile, rng):
    """Islands of 1, 2, 3, 4, 5, ... valid frames between NaN runs of 2 h + 1, h and 1 frames (windows with n < 3, even and odd n),
    a spike in every island"""
    T = x.shape[0]
    keep = np.zeros(T, bool)
    t, size, runs = 0, 1, (2 * h + 1, h, 1)
    while t < T:
        keep[t:t + size] = True
        _spike(x, (t + size // 2,), rng)
        t += size + runs[size % 3]
        size = size % 6 + 1
    x[~keep] = np.nan


def p_all_nan(x, h, tile, rng):
    x[:] = np.nan


def p_constant(x, h, tile, rng):
    """a still marker: mad = 0, a few frames differ in the last bit, one real spike"""
    x[:] = x[0]
    for t in _at(x, (2, tile - 1, x.shape[0] - 3)):
        x[t, t % 3] = np.nextafter(x[t, t % 3], np.float32(np.inf))
    _spike(x, (x.shape[0] // 2,), rng)


def p_ties_and_signed_zeros(x, h, tile, rng):
    x[:] = rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, 1.0, 2.0, -1.0], np.float32), size=x.shape)


def p_denormals(x, h, tile, rng):
    x[:] = (rng.integers(-40, 40, x.shape).astype(np.float64) * 1e-45).astype(np.float32)
    for t in _at(x, (1, x.shape[0] // 2, tile)):
        x[t, 0] = np.float32(3e-41)


def p_magnitudes_of_1e30(x, h, tile, rng):
    x *= np.float32(1e30)
    for t in _at(x, (0, x.shape[0] // 3, tile - 1)):
        x[t, 2] = np.float32(3.0e38) * np.float32(rng.choice((-1.0, 1.0)))


def p_infinite_coordinates(x, h, tile, rng):
    T = x.shape[0]
    for i, t in enumerate(_at(x, (1, T // 3, tile - 1, tile + 2, T - 2))):
        x[t, i % 3] = np.float32(np.inf if i % 2 else -np.inf)  # missing; its finite coordinates pass bit for bit
    _spike(x, (2, T // 3 + 1, tile, T - 3), rng)


def p_nan_in_one_coordinate(x, h, tile, rng):
    for t in _at(x, (0, x.shape[0] // 2, tile)):
        x[t, 1] = np.nan
    _spike(x, (1, x.shape[0] // 2 + 2), rng)


PATTERNS = {
    "smooth": p_smooth, "spikes_at_edges_and_tile_borders": p_spikes_at_edges_and_tile_borders, "spikes_random": p_spikes_random,
    "run_of_h": p_run_of_h, "run_of_h_plus_1": p_run_of_h_plus_1, "spike_in_one_coordinate": p_spike_in_one_coordinate,
    "spikes_next_to_nan_runs": p_spikes_next_to_nan_runs, "all_nan": p_all_nan, "constant": p_constant,
    "ties_and_signed_zeros": p_ties_and_signed_zeros, "denormals": p_denormals, "magnitudes_of_1e30": p_magnitudes_of_1e30,
    "infinite_coordinates": p_infinite_coordinates, "nan_in_one_coordinate": p_nan_in_one_coordinate,
}  # fmt: skip
MIXED = "mixed"  # track k carries pattern (k + T) mod 14: every pattern at every shape with K >= 14, a rotating choice below


def make_case(name, h, T, K, tile):
    """-> kp [T, 3K] float32: every track a smooth noisy series with the pattern ``name`` (``mixed``: a different one per track)"""
    names = list(PATTERNS)
    seed = 100_000 * (names.index(name) + 1 if name != MIXED else 0) + 1000 * h + 7 * T + K
    rng = np.random.default_rng(seed)
    x = np.empty((T, K, 3), np.float32)
    for k in range(K):
        x[:, k] = smooth_track(T, rng)
        track = np.array(x[:, k])
        PATTERNS[names[(k + T) % len(names)] if name == MIXED else name](track, h, tile, rng)
        x[:, k] = track
    return np.ascontiguousarray(x.reshape(T, 3 * K))


def cases(tile):
    """(name, h, T, K, min_dev) of every case: ``mixed`` at every h x T x K of the issue, and every pattern on its own at
    T = 2 tile + 1, K = 2 with min_dev = 0 and min_dev = 0.01 (the floor that keeps a still marker)"""
    out = []
    for h in HS:
        for T in shapes_T(h, tile):
            for K in KS:
                out.append((MIXED, h, T, K, 0.0))
        out.append((MIXED, h, 2 * tile + 1, 23, 0.01))
        for name in PATTERNS:
            for min_dev in (0.0, 0.01):
                out.append((name, h, 2 * tile + 1, 2, min_dev))
    return out


_REF = {}


def reference(name, h, T, K, tile, min_dev):
    """(kp, out, flag) of a case, computed once and shared (read-only) among the tests"""
    key = (name, h, T, K, tile, min_dev)
    if key not in _REF:
        kp = make_case(name, h, T, K, tile)
        out, flag = reference_reject(kp, h, THR, min_dev)
        for a in (kp, out, flag):
            a.setflags(write=False)
        _REF[key] = (kp, out, flag)
    return _REF[key]


def check(got_out, got_flag, kp, want_out, want_flag, label=""):
    """Tolerance 0: ``flag`` equal, ``out`` equal as uint32 words; a rejected keypoint is three quiet NaNs 0x7FC00000 and every other
    element is the input's bits."""
    got_out, got_flag = np.asarray(got_out), np.asarray(got_flag)
    assert got_out.dtype == np.float32 and got_out.shape == want_out.shape, (label, got_out.dtype, got_out.shape)
    assert got_flag.dtype == np.uint8 and got_flag.shape == want_flag.shape, (label, got_flag.dtype, got_flag.shape)
    np.testing.assert_array_equal(got_flag, want_flag, err_msg=f"{label} flag")
    np.testing.assert_array_equal(got_out.view(np.uint32), want_out.view(np.uint32), err_msg=f"{label} out (bits)")
    T, K = want_flag.shape
    g, x = got_out.reshape(T, K, 3).view(np.uint32), np.asarray(kp).reshape(T, K, 3).view(np.uint32)
    assert (g[want_flag == 1] == QNAN).all(), label
    np.testing.assert_array_equal(g[want_flag == 0], x[want_flag == 0], err_msg=f"{label} passed entries (bits)")
