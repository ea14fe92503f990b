"""Cases and the reference shared by tests/test_smooth_host.py (a CPU build of csrc/stac_smooth.hpp) and tests/test_gpu_smooth.py
(the kernel): column layouts, inputs, and ``restate`` -- the rule of DESIGN.md "Smoothing fitted poses" in numpy float32, written
from the rule and not from the header: a loop over the window position j, vectorised over clips, frames and columns, every
operation one IEEE float32 operation in the rule's order.  Kernel, CPU build and restatement therefore agree bit for bit
(tolerance 0); ``assert_same_bits`` compares the words of everything that is not a NaN and the places of the NaNs.
"""

import numpy as np

from conftest import GOLDEN

HALF_WINDOWS = (1, 2, 5, 16)
JNT_FREE, JNT_BALL = 0, 1


def golden_layout(name):
    """(nq, first columns of the quaternion blocks) of a model of tests/golden/: the free joint's block and every ball joint's."""
    with np.load(GOLDEN / f"{name}_tables.npz", allow_pickle=True) as d:
        nq, jt, adr = int(d["nq"]), np.asarray(d["jnt_type"]), np.asarray(d["jnt_qposadr"])
    return nq, [int(a) + 3 for a in adr[jt == JNT_FREE]] + [int(a) for a in adr[jt == JNT_BALL]]


# name -> (nq, quaternion start columns)
LAYOUTS = {
    "scalar1": (1, []),
    "ball4": (4, [0]),
    "free7": (7, [3]),
    "free8": (8, [3]),
    "rodent74": golden_layout("rodent"),
    "mouse230": golden_layout("mouse"),
    "tail_ball13": (13, [3, 9]),  # a free joint, two hinges, and a ball joint in the last four columns
}
assert LAYOUTS["rodent74"][0] == 74 and LAYOUTS["mouse230"][0] == 230


def clip_lengths(T, H):
    """The clip lengths at which the kernel takes another path, for a tile of T frames: one window, one more, just short of two
    windows, around one tile, a tile and a halo, more than two tiles.  A length below the window is no input (the entry point
    refuses it), so those collapse onto W."""
    W = 2 * H + 1
    return sorted({max(L, W) for L in (W, W + 1, 2 * W - 1, T - 1, T, T + 1, T + H, 2 * T + 3)})


def scalar_cols(nq, quat_cols):
    inq = np.zeros(nq, bool)
    for c in quat_cols:
        inq[c:c + 4] = True
    return np.flatnonzero(~inq)


def _quat_mul64(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _dots(X, col, H):
    """The alignment dot products d of the rule for the block at ``col``: [C, L, W] float32."""
    C, L, _ = X.shape
    W = 2 * H + 1
    t = np.arange(L)
    s = np.clip(t - H, 0, L - W)
    c = X[:, :, col:col + 4]
    out = np.empty((C, L, W), np.float32)
    for j in range(W):
        y = X[:, s + j, col:col + 4]
        out[:, :, j] = ((c[..., 0] * y[..., 0] + c[..., 1] * y[..., 1]) + c[..., 2] * y[..., 2]) + c[..., 3] * y[..., 3]
    return out


def make_input(L, clips, nq, quat_cols, H, seed=0, specials=True):
    """qpos [clips * L, nq] float32.  Scalar columns: a random walk plus noise.  Quaternion blocks: a chain of random-axis rotation
    steps of 0.02 .. 0.4 rad from a random start, built like ``post_cases.qvel_input``, with an eighth of the frames negated (q and
    -q) and an eighth rescaled by 0.5 .. 2.  The builder asserts that no alignment dot product of the rule is exactly zero on this
    clean input (there the sign, and with it the hemisphere, would hang on a rounding).  ``specials`` then adds: one all-zero
    quaternion, one NaN quaternion component, with three clips a whole block column of zeros in clip 1 (the norm is 0: the
    ``n > 0`` branch), and one NaN in a scalar column in a head window and one in an interior window."""
    rng = np.random.default_rng([seed, L, clips, nq, H, len(quat_cols)])
    N = L * clips
    q = np.cumsum(rng.standard_normal((N, nq)) * 0.05, axis=0) + rng.standard_normal((N, nq)) * 0.02
    for col in quat_cols:
        cur = rng.standard_normal(4)
        cur /= np.linalg.norm(cur)
        for r in range(N):
            q[r, col:col + 4] = cur
            axis = rng.standard_normal(3)
            axis /= np.linalg.norm(axis)
            ang = rng.uniform(0.02, 0.4)
            cur = _quat_mul64(cur, np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * axis]))
            cur /= np.linalg.norm(cur)
        for r in rng.choice(N, size=max(N // 8, 1), replace=False):
            q[r, col:col + 4] *= -1.0
        for r in rng.choice(N, size=max(N // 8, 1), replace=False):
            q[r, col:col + 4] *= rng.uniform(0.5, 2.0)
    q = np.ascontiguousarray(q.astype(np.float32))
    for col in quat_cols:
        assert not np.any(_dots(q.reshape(clips, L, nq), col, H) == 0), "the case itself is ill-posed: an alignment dot product of 0"
    if specials:
        sc = scalar_cols(nq, quat_cols)
        if quat_cols:
            q[min(2, N - 1), quat_cols[0]:quat_cols[0] + 4] = 0.0           # one all-zero quaternion
            q[N - 1 - min(1, N - 1), quat_cols[-1] + 2] = np.nan            # one NaN component near the end of the last clip
            if clips >= 3:
                q[L:2 * L, quat_cols[0]:quat_cols[0] + 4] = 0.0             # every window of clip 1 sums to zero
        if sc.size:
            q[0, sc[0]] = np.nan                                            # a head window
            q[(clips - 1) * L + L // 2, sc[-1]] = np.nan                    # an interior window (when L > W)
    return q


def make_bounds(nq, quat_cols, seed=0):
    """lb, ub [nq] float32: a third of the scalar columns unbounded (-inf / +inf), a third with a box the walk leaves on both
    sides, a third with one wide box; quaternion columns -1 / 1 as the engine holds them (the rule never clamps those)."""
    rng = np.random.default_rng([seed, nq, 77])
    lb, ub = np.full(nq, -np.inf, np.float32), np.full(nq, np.inf, np.float32)
    for i, j in enumerate(scalar_cols(nq, quat_cols)):
        if i % 3 == 1:
            lb[j], ub[j] = np.float32(-rng.uniform(0.01, 0.2)), np.float32(rng.uniform(0.01, 0.2))
        elif i % 3 == 2:
            lb[j], ub[j] = np.float32(-50.0), np.float32(50.0)
    for c in quat_cols:
        lb[c:c + 4], ub[c:c + 4] = -1.0, 1.0
    return lb, ub


def restate(x, L, taps, quat_cols, lb=None, ub=None):
    """The rule, in numpy float32: x [N, nq] of whole clips of L rows -> [N, nq]."""
    x = np.asarray(x)
    taps = np.asarray(taps)
    assert x.dtype == np.float32 and taps.dtype == np.float32 and x.ndim == 2 and taps.ndim == 2 and taps.shape[0] == taps.shape[1]
    N, nq = x.shape
    W = taps.shape[0]
    H = W // 2
    assert W == 2 * H + 1 and L >= W and N % L == 0
    X = x.reshape(N // L, L, nq)
    t = np.arange(L)
    s = np.clip(t - H, 0, L - W)   # the window of frame t starts here, inside its clip
    p = t - s                       # and the frame stands at this position of it
    with np.errstate(all="ignore"):
        acc = None
        for j in range(W):
            prod = taps[p, j][None, :, None] * X[:, s + j, :]
            acc = prod if j == 0 else acc + prod
        if lb is not None:
            lo, hi = np.asarray(lb, np.float32)[None, None, :], np.asarray(ub, np.float32)[None, None, :]
            acc = np.where(acc < lo, lo, np.where(acc > hi, hi, acc))  # comparisons: a NaN stays
        out = acc.astype(np.float32)
        for col in quat_cols:
            c = X[:, :, col:col + 4]
            a = None
            for j in range(W):
                y = X[:, s + j, col:col + 4]
                d = ((c[..., 0] * y[..., 0] + c[..., 1] * y[..., 1]) + c[..., 2] * y[..., 2]) + c[..., 3] * y[..., 3]
                sg = np.where(d < 0, np.float32(-1.0), np.float32(1.0))
                prod = taps[p, j][None, :, None] * (sg[..., None] * y)
                a = prod if j == 0 else a + prod
            n = np.sqrt(((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]) + a[..., 3] * a[..., 3])
            assert a.dtype == np.float32 and n.dtype == np.float32
            out[:, :, col:col + 4] = np.where((n > 0)[..., None], a / n[..., None], c)
    assert out.dtype == np.float32
    return out.reshape(N, nq)


def assert_same_bits(got, want, label=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32, (label, got.shape, want.shape, got.dtype)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{label}: NaN places")
    g, w = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{label}: {bad.size} of {g.size} words differ, first at flat index {bad[0]} of the non-NaN values"
