"""An independent float64 statement of the kinematics and of the offset phase -- numpy only, no ctypes, no shared code with
oracle/stac_oracle.c.

Written from MuJoCo's kinematics rule (mj_kinematics: a body starts at its parent's frame moved by body_pos / body_quat, then
each of its joints acts in turn) and from the sums of `_m_opt` (include/stac_hip.h, stac_core.py:148-170).  Every rotation is
applied as the 3 x 3 matrix of its quaternion and no care is taken over the order of the operations: it shares neither the
arithmetic nor the structure of the restatement it checks (tests/test_kin_ref_host.py).
"""

from __future__ import annotations

import numpy as np

FREE, BALL, SLIDE, HINGE = 0, 1, 2, 3  # mjtJoint


def rot(q):
    """The 3 x 3 matrix of a quaternion (w, x, y, z) as MuJoCo defines it (mju_quat2Mat): v -> q v q*.  For a unit quaternion it
    is the rotation matrix; body_quat is stored in float32 and unit only to that rounding, and for such a q this matrix is |q|^2
    times a rotation -- which is what the model means: MJX composes the stored quaternions and never renormalises a body's."""
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def mul(a, b):
    """Hamilton product a (x) b."""
    aw, av, bw, bv = a[0], a[1:], b[0], b[1:]
    return np.concatenate([[aw * bw - av @ bv], aw * bv + bw * av + np.cross(av, bv)])


def _unit(v):
    return v / np.linalg.norm(v)


def fk(tables, qpos):
    """xpos[nbody,3], xquat[nbody,4], site_xpos[K,3] of one pose, float64."""
    t = tables
    f64 = lambda a: np.asarray(a, np.float64)
    q, q0 = f64(qpos), f64(t.qpos0)
    body_pos, body_quat, jnt_pos, jnt_axis, site_pos = f64(t.body_pos), f64(t.body_quat), f64(t.jnt_pos), f64(t.jnt_axis), f64(t.site_pos)
    xpos, xquat = np.zeros((t.nbody, 3)), np.zeros((t.nbody, 4))
    xquat[0] = [1, 0, 0, 0]
    for b in range(1, t.nbody):
        p = int(t.body_parentid[b])
        pos = xpos[p] + rot(xquat[p]) @ body_pos[b]
        quat = mul(xquat[p], body_quat[b])
        j0 = int(t.body_jntadr[b])
        for j in range(j0, j0 + int(t.body_jntnum[b])):
            a, ty = int(t.jnt_qposadr[j]), int(t.jnt_type[j])
            if ty == FREE:
                pos, quat = q[a:a + 3].copy(), _unit(q[a + 3:a + 7])
            elif ty == SLIDE:
                pos = pos + rot(quat) @ jnt_axis[j] * (q[a] - q0[a])
            else:
                if ty == BALL:
                    ql = _unit(q[a:a + 4])
                else:
                    th = q[a] - q0[a]
                    ql = np.concatenate([[np.cos(th / 2)], jnt_axis[j] * np.sin(th / 2)])
                anchor = pos + rot(quat) @ jnt_pos[j]
                quat = mul(quat, ql)
                pos = anchor - rot(quat) @ jnt_pos[j]
        xpos[b], xquat[b] = pos, quat
    sb = np.asarray(t.site_bodyid, np.int64)
    sites = np.stack([xpos[b] + rot(xquat[b]) @ site_pos[k] for k, b in enumerate(sb)]) if len(sb) else np.zeros((0, 3))
    return xpos, xquat, sites


def m_sums(tables, kp, q):
    """The cross-frame sums of the offset phase: s[K,3] = sum_t R(xquat_b)^T (y - xpos_b), z2 = sum |y - xpos_b|^2, and T."""
    K = tables.nsite
    kp = np.asarray(kp, np.float64).reshape(-1, K, 3)
    q = np.asarray(q, np.float64).reshape(len(kp), -1)
    sb = np.asarray(tables.site_bodyid, np.int64)
    s, z2 = np.zeros((K, 3)), 0.0
    for t in range(len(kp)):
        xpos, xquat, _ = fk(tables, q[t])
        z = kp[t] - xpos[sb]
        s += np.stack([rot(xquat[b]).T @ z[k] for k, b in enumerate(sb)])
        z2 += (z * z).sum()
    return s, z2, len(kp)


def m_closed_form(sums, m0, d, lam):
    """offsets[K,3] and the objective at them from m_sums: m0[K,3] the previous offsets, d[K,3] the 0/1 regularisation mask, lam
    the coefficient."""
    s, z2, T = sums
    m0, d, lam = np.asarray(m0, np.float64).reshape(s.shape), np.asarray(d, np.float64).reshape(s.shape), float(lam)
    m = (s + lam * d * m0) / (T + lam * d)
    err = z2 - 2 * (m * s).sum() + T * (m * m).sum() + lam * ((d * (m - m0)) ** 2).sum()
    return m, err


def m_opt(tables, kp, q, m0, d, lam):
    """The closed form of the offset phase over T frames, float64: kp[T,3K], q[T,nq] -> offsets[K,3], err."""
    return m_closed_form(m_sums(tables, kp, q), m0, d, lam)
