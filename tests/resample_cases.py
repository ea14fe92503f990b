"""Cases and the reference shared by tests/test_resample_host.py (a CPU build of csrc/stac_resample.hpp) and
tests/test_gpu_resample.py (the kernel): ``taps64`` -- the tap table from its formula, a copy of its own and not an import from
``post.py`` --, ``restate`` -- the rule of DESIGN.md "Resampling fitted poses" in numpy float32, a loop over the tap j, vectorised
over clips, outputs and columns, every operation one IEEE float32 operation in the rule's order -- and the case list.  Kernel, CPU
build and restatement agree bit for bit (tolerance 0); ``assert_same_bits`` compares the words of everything that is not a NaN and
the places of the NaNs.
"""

import numpy as np

from smooth_cases import assert_same_bits  # noqa: F401  (the comparison is smoothing's)

# the ratios of the issue's scipy check: 300 -> 50, 120 -> 50, 200 -> 50, 30 -> 50, 50 -> 100, 100 -> 30
SCIPY_RATIOS = ((1, 6), (5, 12), (1, 4), (5, 3), (2, 1), (3, 10))


def taps64(U, D, lobes=10, beta=5.0, normalise=True):
    """[U, W] float64: h[i] = (1 / M) sinc((i - half) / M) kaiser(2 half + 1, beta)[i], M = max(U, D), half = lobes M, divided by
    its sum and multiplied by U; H = half // U + 1, W = 2 H; tap j of phase r is h[half + r - (j - H + 1) U], 0 outside the filter;
    with ``normalise`` every row divided by its own sum."""
    M = max(U, D)
    half = lobes * M
    h = np.array([(1.0 / M) * np.sinc((i - half) / M) for i in range(2 * half + 1)]) * np.kaiser(2 * half + 1, beta)
    h = h / h.sum()
    h = h * U
    H = half // U + 1
    t = np.zeros((U, 2 * H))
    for r in range(U):
        for j in range(2 * H):
            i = half + r - (j - H + 1) * U
            if 0 <= i <= 2 * half:
                t[r, j] = h[i]
    if normalise:
        t = t / t.sum(axis=1)[:, None]
    return t


def taps32(U, D, lobes=10, beta=5.0):
    return np.ascontiguousarray(taps64(U, D, lobes, beta), dtype=np.float32)


def rows(L, U, D):
    return ((L - 1) * U) // D + 1


def index(L, U, D):
    """(n, r) of the outputs of a clip of L rows, with Python integers."""
    m = [i * D for i in range(rows(L, U, D))]
    return np.array([p // U for p in m], dtype=np.int64), np.array([p % U for p in m], dtype=np.int64)


def restate(x, L, U, D, taps, quat_cols=(), lb=None, ub=None, dtype=np.float32):
    """The rule, in numpy ``dtype``: x [N, C] of whole clips of L rows -> [(N / L) Lo, C]."""
    x, taps = np.asarray(x), np.asarray(taps)
    assert x.dtype == dtype and taps.dtype == dtype and x.ndim == 2 and taps.ndim == 2 and taps.shape[0] == U and taps.shape[1] % 2 == 0
    N, C = x.shape
    W = taps.shape[1]
    H = W // 2
    assert L >= 1 and N % L == 0
    X = x.reshape(N // L, L, C)
    n, r = index(L, U, D)
    with np.errstate(all="ignore"):
        acc = None
        for j in range(W):
            src = np.clip(n + (j - H + 1), 0, L - 1)  # rows outside the clip are its first or last row
            prod = taps[r, j][None, :, None] * X[:, src, :]
            acc = prod if j == 0 else acc + prod
        if lb is not None:
            lo, hi = np.asarray(lb, dtype)[None, None, :], np.asarray(ub, dtype)[None, None, :]
            acc = np.where(acc < lo, lo, np.where(acc > hi, hi, acc))  # comparisons: a NaN stays
        out = acc.astype(dtype)
        for col in quat_cols:
            c = X[:, n, col:col + 4]
            a = None
            for j in range(W):
                y = X[:, np.clip(n + (j - H + 1), 0, L - 1), col:col + 4]
                d = ((c[..., 0] * y[..., 0] + c[..., 1] * y[..., 1]) + c[..., 2] * y[..., 2]) + c[..., 3] * y[..., 3]
                sg = np.where(d < 0, dtype(-1.0), dtype(1.0))
                prod = taps[r, j][None, :, None] * (sg[..., None] * y)
                a = prod if j == 0 else a + prod
            nrm = np.sqrt(((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]) + a[..., 3] * a[..., 3])
            assert a.dtype == dtype and nrm.dtype == dtype
            out[:, :, col:col + 4] = np.where((nrm > 0)[..., None], a / nrm[..., None], c)
    assert out.dtype == dtype
    return out.reshape(-1, C)


def scalar_cols(C, quat_cols):
    inq = np.zeros(C, bool)
    for c in quat_cols:
        inq[c:c + 4] = True
    return np.flatnonzero(~inq)


def make_input(L, clips, C, quat_cols, seed=0, specials=True):
    """x [clips * L, C] float32.  Scalar columns: a random walk plus noise.  Quaternion blocks: a chain of small random rotations from
    a random start, an eighth of the rows negated (q and -q) and an eighth rescaled by 0.5 .. 2.  ``specials`` adds one all-zero
    quaternion, one NaN quaternion component, with three clips a whole block column of zeros in clip 1 (the norm is 0) and a NaN
    in the first and in a middle row of two scalar columns."""
    rng = np.random.default_rng([seed, L, clips, C, len(quat_cols)])
    N = L * clips
    q = np.cumsum(rng.standard_normal((N, C)) * 0.05, axis=0) + rng.standard_normal((N, C)) * 0.02
    for col in quat_cols:
        step = rng.standard_normal((N, 4)) * 0.1
        cur = rng.standard_normal(4)
        for i in range(N):
            cur = cur / np.linalg.norm(cur)
            q[i, col:col + 4] = cur
            cur = cur + step[i]
        neg = rng.choice(N, size=max(N // 8, 1), replace=False)
        q[neg, col:col + 4] *= -1.0
        big = rng.choice(N, size=max(N // 8, 1), replace=False)
        q[big, col:col + 4] *= rng.uniform(0.5, 2.0, size=(big.size, 1))
    q = np.ascontiguousarray(q.astype(np.float32))
    if specials:
        sc = scalar_cols(C, quat_cols)
        if len(quat_cols):
            q[min(2, N - 1), quat_cols[0]:quat_cols[0] + 4] = 0.0
            q[N - 1 - min(1, N - 1), quat_cols[-1] + 2] = np.nan
            if clips >= 3:
                q[L:2 * L, quat_cols[0]:quat_cols[0] + 4] = 0.0
        if sc.size:
            q[0, sc[0]] = np.nan
            q[(clips - 1) * L + L // 2, sc[-1]] = np.nan
    return q


def make_bounds(C, quat_cols, seed=0):
    """lb, ub [C] float32: a third of the scalar columns unbounded, a third with a box the walk leaves on both sides, a third with
    one wide box; quaternion columns -1 / 1 as the engine holds them (the rule never clamps those)."""
    rng = np.random.default_rng([seed, C, 78])
    lb, ub = np.full(C, -np.inf, np.float32), np.full(C, np.inf, np.float32)
    for i, j in enumerate(scalar_cols(C, quat_cols)):
        if i % 3 == 1:
            lb[j], ub[j] = np.float32(-rng.uniform(0.01, 0.2)), np.float32(rng.uniform(0.01, 0.2))
        elif i % 3 == 2:
            lb[j], ub[j] = np.float32(-50.0), np.float32(50.0)
    for c in quat_cols:
        lb[c:c + 4], ub[c:c + 4] = -1.0, 1.0
    return lb, ub


def alternating_quats(L, n):
    """A smooth chain of unit quaternions [L, 4], the same with every odd row negated, and the sign [Lo, 1] of the centre row ``n`` of
    every output: what the alternating series must come out multiplied by."""
    rng = np.random.default_rng([L, 4])
    v = np.cumsum(rng.standard_normal((L, 4)) * 0.05, axis=0) + np.array([1.0, 0.0, 0.0, 0.0])
    q = np.ascontiguousarray((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32))
    flip = q * np.where(np.arange(L) % 2 == 0, 1.0, -1.0).astype(np.float32)[:, None]
    return q, np.ascontiguousarray(flip), np.where(np.asarray(n) % 2 == 0, 1.0, -1.0).astype(np.float32)[:, None]


def clip_len_for(Lo, U, D):
    """The shortest clip with ``Lo`` outputs, or None where no clip has exactly that many (U > D skips counts)."""
    L = -(-(Lo - 1) * D // U) + 1
    return L if rows(L, U, D) == Lo else None


def cases(tile_rows, band=64):
    """The case list: (label, U, D, taps [U, W] float32, L, clips, C, quat_cols, bounded).  ``tile_rows(C, U, D, W)``: the kernel's
    tile rule (``post.resample_tile_rows``), by which the clip lengths around a tile are sized; ``band``: its widest band."""
    out = []

    def add(label, U, D, lobes, L, clips, C, cols, bounded, taps=None):
        out.append((f"{label}: {U}/{D} lobes={lobes} L={L} clips={clips} C={C} cols={cols} bounds={bounded}", U, D,
                    taps32(U, D, lobes) if taps is None else taps, L, clips, C, list(cols), bounded))

    # ratios and lobes, on the rodent's row
    for i, (U, D, lobes) in enumerate([(1, 2, 1), (2, 1, 1), (1, 6, 1), (5, 12, 1), (5, 3, 1), (32, 1, 1), (1, 6, 10), (5, 12, 10), (1, 12, 10)]):
        add("ratio", U, D, lobes, 41, 2, 74, [3], bool(i & 1))
    # clip lengths: every tap clamped (1, 2, H, W - 1), the last output on and off the last sample, outputs around the tile
    for U, D, lobes in ((5, 12, 1), (1, 6, 10)):
        W = taps32(U, D, lobes).shape[1]
        T = tile_rows(74, U, D, W)
        lens = {1, 2, W // 2, W - 1}
        on =next(L for L in range(W, W + 2 * D + 1) if ((L - 1) * U) % D == 0)
        off = next(L for L in range(W, W + 2 * D + 1) if ((L - 1) * U) % D != 0)
        lens |= {on, off} | {clip_len_for(Lo, U, D) for Lo in (T, T + 1, 2 * T + 1)}
        for i, L in enumerate(sorted(lens)):
            add(f"length (tile {T})", U, D, lobes, L, (1, 3)[i & 1], 74, [3], bool(i & 2))
    T = tile_rows(74, 2, 1, 4)
    for Lo in (T + 1, 2 * T + 1):  # (2 L - 1 outputs: an odd count only)
        add(f"length (tile {T})", 2, 1, 1, clip_len_for(Lo, 2, 1), 2, 74, [3], False)
    # columns: one scalar, one quaternion alone, a free joint, the rodent, the mouse with blocks across its band border and in its last
    # four columns, the keypoint form, a ball joint in the last four columns, the band and its neighbours (a block across the border)
    for i, (C, cols) in enumerate([(1, []), (4, [0]), (7, [3]), (74, [3]), (230, [3, 56, 226]), (69, []), (13, [3, 9]), (band, [3, 60]),
                                   (band - 1, [3, 59]), (band + 1, [3, 31, 61]), (512, [3, 62, 126, 508])]):
        add("columns", 5, 12, 1, 30, (3, 1)[i & 1], C, cols, bool(i & 2))
        if C in (74, 230, band + 1):
            add("columns", 1, 6, 10, 30, 2, C, cols, True)
    add("columns, widest window", 1, 12, 10, 20, 1, 512, [3, 62, 126, 508], True)
    # a table of the widest window at the largest U (no Kaiser table is that wide): the tile is shorter than U, so the phase rows are
    # staged per tile
    rng = np.random.default_rng(5)
    wide = rng.standard_normal((32, 256))
    wide = np.ascontiguousarray((wide / wide.sum(axis=1, keepdims=True)).astype(np.float32))
    assert tile_rows(band, 32, 1, 256) < 32
    add("phase rows per tile", 32, 1, None, 3, 2, band, [3, 60], True, taps=wide)
    return out
