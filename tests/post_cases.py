"""Cases and checks shared by tests/test_post_host.py (a CPU build of csrc/stac_post.hpp) and tests/test_gpu_post.py (the
kernels): inputs, the host reference (``stac_mjx_amd.utils``, untouched) and the tolerances.

Tolerances (derived, not tuned).  Bit-equal: the stitched arrays and every qvel column but the root gyro -- each operation in
them is one IEEE float32 / float64 add, subtract, multiply, divide or convert in a stated order.  Gyro columns 3..5: both sides
evaluate the same double expression from bit-equal float32 inputs and differ by the few-ulp errors of two double math libraries
(1e-15 relative against float32's 6e-8), so a value can cross at most one float32 rounding boundary, which the following
float32 division by dt can widen to two: at most 2 float32 ulp at the host value.
"""

from types import SimpleNamespace

import numpy as np

from stac_mjx_amd import utils

OV = utils.CONTINUOUS_BATCH_OVERLAP
STITCH_CF = [(C, F) for C in (1, 2, 3, 5) for F in (1, 4, 9, 10, 11, 12, 25)]
STITCH_TRAILING = [(1,), (3,), (69,), (74,), (67, 4), (23, 3)]
STITCH_BIG = (300, 50, (74,))

QVEL_FC = [(1, 3), (2, 4), (7, 3), (250, 2)]
QVEL_NQ = [(True, 7), (True, 8), (True, 74), (False, 1), (False, 5), (False, 74)]
QVEL_DT = [0.02, 1.0 / 300.0, 1.0]
MAX_QVEL = 20.0


def stitch_rows(C, F, ov=OV):
    return F + ov + max(C - 2, 0) * F + max(F - ov, 0)


def stitch_input(C, F, trailing, seed=0):
    """Standard normal [C, F + 10, *trailing] with a few NaNs in head rows, tail rows and body rows."""
    rng = np.random.default_rng([seed, C, F, int(np.prod(trailing))])
    x = rng.standard_normal((C, F + OV) + tuple(trailing)).astype(np.float32)
    flat = x.reshape(C, F + OV, -1)
    D = flat.shape[2]
    flat[0, 0, 0] = np.nan                      # head row of the first clip (a plain copy)
    flat[0, F + OV - 1, D - 1] = np.nan         # tail row: faded when there is a next clip
    flat[C - 1, min(OV, F + OV - 1), D // 2] = np.nan  # body (or tail) row of the last clip
    if C > 1:
        flat[1, 0, D // 2] = np.nan             # head row of clip 1: the other operand of a fade
        flat[C // 2, F, 0] = np.nan             # first tail row of a middle clip
    return x


def host_stitch(x, F):
    """``utils.handle_edge_effects`` on one array [C, F + 10, ...] (it takes the five arrays of a StacData, flat)."""
    flat = x.reshape((-1,) + x.shape[2:])
    data = SimpleNamespace(**{name: flat.copy() for name in ("qpos", "kp_data", "xpos", "xquat", "marker_sites")})
    out = utils.handle_edge_effects(data, F)
    for name in ("kp_data", "xpos", "xquat", "marker_sites"):
        np.testing.assert_array_equal(getattr(out, name), out.qpos)
    assert out.qpos.dtype == np.float32
    return out.qpos


def _quat_mul64(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def qvel_input(F, C, nq, freejoint, dt, seed=0):
    """qpos [C * F, nq] float32.  Root quaternion (free joint): a chain of random-axis rotation steps with angles uniform in
    [1e-4, 3] rad, with some exactly repeated frames (the zero branch), some frames negated (q and -q; the steps next to
    those are at least 0.1 rad, so that no normalised difference is exactly w = -1) and some scaled by 0.5 .. 2.  Joints: a
    random walk with jumps beyond max_qvel * dt in both signs and one of exactly max_qvel * dt."""
    rng = np.random.default_rng([seed, F, C, nq, int(freejoint), int(round(1e6 * dt))])
    N = F * C
    q = np.cumsum(rng.standard_normal((N, nq)) * (0.3 * MAX_QVEL * dt), axis=0)
    j0 = 7 if freejoint else 0
    nj = nq - j0
    negate = set(rng.choice(N, size=max(N // 8, 1), replace=False).tolist()) if N > 1 else set()
    if freejoint:
        q[:, :3] = np.cumsum(rng.standard_normal((N, 3)) * 0.01, axis=0)
        cur = rng.standard_normal(4)
        cur /= np.linalg.norm(cur)
        for r in range(N):
            q[r, 3:7] = cur
            axis = rng.standard_normal(3)
            axis /= np.linalg.norm(axis)
            lo = 0.1 if (r in negate or r + 1 in negate) else 1e-4
            ang = rng.uniform(lo, 3.0)
            cur = _quat_mul64(cur, np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * axis]))
            cur /= np.linalg.norm(cur)
        for r in sorted(negate):
            q[r, 3:7] *= -1.0
        for r in rng.choice(N, size=max(N // 8, 1), replace=False):
            q[r, 3:7] *= rng.uniform(0.5, 2.0)
    q = q.astype(np.float32)
    if nj > 0 and N > 1:
        step = np.float32(MAX_QVEL * dt)
        rows = rng.choice(N - 1, size=min(N - 1, 4), replace=False)
        for k, r in enumerate(rows):
            j = j0 + int(rng.integers(nj))
            q[r + 1, j] = q[r, j] + np.float32((3.0 if k % 2 == 0 else -3.0) * step)  # clipped, both signs
        q[1, j0] = q[0, j0] = np.float32(0.0)
        q[1, j0] = step  # a difference of exactly max_qvel * dt
    if N > 2:  # exactly repeated frames, away from the negated ones
        for r in rng.choice(N - 1, size=max(N // 10, 1), replace=False):
            if r not in negate and r + 1 not in negate:
                q[r + 1] = q[r]
    return np.ascontiguousarray(q)


def host_qvel(qpos, F, dt, freejoint):
    """``utils.compute_velocity_from_kinematics`` per clip of F rows, concatenated (as ``main.run_stac`` applies it)."""
    clips = qpos.reshape(-1, F, qpos.shape[-1])
    with np.errstate(all="ignore"):
        out = np.concatenate([utils.compute_velocity_from_kinematics(c, dt=dt, freejoint=freejoint, max_qvel=MAX_QVEL) for c in clips])
    assert out.dtype == np.float32
    return out


def assert_host_gyro_is_meaningful(qpos, F):
    """No normalised quaternion difference of the host computation has w == -1 exactly (there the reference divides by sin(pi))."""
    for c in qpos.reshape(-1, F, qpos.shape[-1]):
        q = np.concatenate([c, c[-1:]], axis=0)
        with np.errstate(all="ignore"):
            diff = utils.quat_diff(q[:-1, 3:7], q[1:, 3:7])
            diff = diff / np.linalg.norm(diff, axis=-1, keepdims=True)
        assert diff.dtype == np.float32
        assert not np.any(diff[:, 0] == np.float32(-1.0)), "the case itself is ill-posed: a quaternion difference with w == -1"


def check_qvel(got, want, freejoint, label=""):
    """Bit-equal outside the gyro columns, at most 2 float32 ulp inside; returns (gyro values not bit-equal, gyro values)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32, (got.shape, want.shape, got.dtype)
    if not freejoint:
        np.testing.assert_array_equal(got, want)
        return 0, 0
    np.testing.assert_array_equal(got[:, :3], want[:, :3])
    np.testing.assert_array_equal(got[:, 6:], want[:, 6:])
    g, w = got[:, 3:6], want[:, 3:6]
    np.testing.assert_array_equal(np.isnan(g), np.isnan(w))
    ok = ~np.isnan(w)
    differ = int(np.count_nonzero(g[ok] != w[ok]))
    print(f"qvel {label}: {differ} of {int(ok.sum())} gyro values are not bit-equal to the host's")
    err = np.abs(g[ok].astype(np.float64) - w[ok].astype(np.float64))
    bound = 2.0 * np.spacing(np.abs(w[ok])).astype(np.float64)
    worst = float((err / np.maximum(bound / 2.0, 1e-300)).max()) if err.size else 0.0
    assert np.all(err <= bound), f"gyro off by {worst:.3g} ulp (at most 2 allowed)"
    return differ, int(ok.sum())
