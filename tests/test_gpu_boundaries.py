"""Capacity edges of the compiled kernel shapes: models that sit on each side of every edge at which the host moves a launch
from one instantiation to another (or refuses it), HIP vs the oracle at tolerance 0, plus float64 checks that do not share the
kernels' arithmetic.

Each case names a model (`_edge_tables`: exactly nq coordinates and K fit sites), the lane width / developer switches of the
launch, and what must happen: the instantiation `stac_debug_last_q_kernel` reports after the q_phase (G, NQR, WPE, SPECP), or a
refusal with STAC_ERR_CAPACITY (-3) -- at model creation or at the launch.  The edges (stac_shapes.hpp, the STAC_Q_*SHAPES
tables: a shape holds nq <= G * NQR; the lean kernels hold K <= lean_site_rounds(G, NQR) * G sites in registers; stac_q.hip:
K <= 4096, P + 3 <= kMaxKinds, LM n <= 192, latency roles of 8 lanes up to nq = 80 and of 16 up to 128) are listed with the
cases; test_every_shape_edge_has_cases (CPU) fails when a shape is added to the tables without cases on both sides of its edge.
"""

import re

import numpy as np
import pytest

from conftest import ROOT
from helpers import _edge_tables
from test_gpu_parity import _box, _compare_phase, _last_q_kernel, _np, _q_phase_twice

EPS = 2.0 ** -24  # float32 unit roundoff

# ---- float64 tolerances (derived from float32 rounding, not fitted to the results) -------------------------------------------
# FK: every level of the tree composes one quaternion product and one rotated offset (a handful of roundings each, at most 4 ulp
# of the level's magnitude per step, carried by the deeper levels) -> 16 ulp per level of depth, plus two for the root and site.
FK_ULPS_PER_LEVEL = 16
# m-phase: m* is an average over T frames of R^T (y - p) -- the f32 FK error of p and R (above) enters once, the sum and the
# division add a few ulp: twice the FK budget.  The objective: its terms cancel (sum of squares minus cross terms), so its
# error is relative to the magnitude S of the squared terms before they cancel, again twice the FK budget per level.
M_ULPS_PER_LEVEL = 32
ERR_ULPS_PER_LEVEL = 64


def _fk_tol(depth, scale):
    return FK_ULPS_PER_LEVEL * (depth + 2) * EPS * max(1.0, scale)


# ---- the case table ------------------------------------------------------------------------------------------------------
THR2 = {"STAC_HIP_WPE": "2", "STAC_HIP_SPEC": "0"}
THR3 = {"STAC_HIP_WPE": "3", "STAC_HIP_SPEC": "0"}
THR4 = {"STAC_HIP_WPE": "4", "STAC_HIP_SPEC": "0"}


def _lat(g):
    return {"STAC_HIP_SPEC": "1", "STAC_HIP_SPECG": str(g)}


REFUSE_CREATE, REFUSE_LAUNCH, FIT_OR_CAPACITY = "refused at creation", "refused at launch", "fits or is refused for capacity"
FREE, FIXED = {}, {"free_root": False}

# (id, nq, K, builder flags, lanes, env, part groups, expected)   part groups: None = two random groups, an int = that many random
# groups, "false1" = one all-false group.  expected: (G, NQR, WPE, SPECP) after the q_phase, or one of the three outcomes above.
_EDGE_CASES = [
    # nq edges of the lean shapes (free root, hinges): <16,3,3> 48 | <16,5,*> 80 | <32,2,8> 64 | <32,3,*> 96 | <32,8,*> 256
    ("lean16w3-nq48", 48, 8, FREE, 16, THR3, None, (16, 3, 3, 1)),
    ("lean16w3-nq49", 49, 8, FREE, 16, THR3, None, (16, 5, 3, 1)),
    ("lean16-nq80", 80, 8, FREE, 16, THR2, None, (16, 5, 2, 1)),
    ("lean16-nq81", 81, 8, FREE, 16, THR2, None, (16, 8, 2, 0)),       # no lean shape of 16 lanes holds 81: generic
    ("lean16w3-nq80", 80, 8, FREE, 16, THR3, None, (16, 5, 3, 1)),
    ("lean16w3-nq81", 81, 8, FREE, 16, THR3, None, (16, 8, 3, 0)),
    ("lat16leanR8-nq80", 80, 8, FREE, 0, dict(_lat(16), STAC_HIP_SPECR="8"), None, (16, 5, 2, 9)),   # two wavefronts per chain
    ("lat16leanR8-nq81", 81, 8, FREE, 0, dict(_lat(16), STAC_HIP_SPECR="8"), None, (16, 8, 2, 4)),
    ("lat16lean-nq48", 48, 8, FREE, 0, _lat(16), None, (16, 3, 2, 5)),
    ("lat16lean-nq49", 49, 8, FREE, 0, _lat(16), None, (16, 5, 2, 5)),
    ("lat16lean-nq80", 80, 8, FREE, 0, _lat(16), None, (16, 5, 2, 5)),
    ("lat16lean-nq81", 81, 8, FREE, 0, _lat(16), None, (16, 8, 2, 4)),
    ("lat32lean-nq64", 64, 8, FREE, 0, _lat(32), None, (32, 2, 2, 9)),
    ("lat32lean-nq65", 65, 8, FREE, 0, _lat(32), None, (32, 3, 2, 9)),
    ("lean32-nq96", 96, 8, FREE, 32, THR2, None, (32, 3, 2, 1)),
    ("lean32-nq97", 97, 8, FREE, 32, THR2, None, (32, 8, 2, 1)),
    ("lat32lean-nq96", 96, 8, FREE, 0, _lat(32), None, (32, 3, 2, 9)),
    ("lat32lean-nq97", 97, 8, FREE, 0, _lat(32), None, (32, 8, 2, 9)),
    ("lean32-nq256", 256, 8, FREE, 32, THR2, None, (32, 8, 2, 1)),
    ("lean32-nq257", 257, 8, FREE, 32, THR2, None, REFUSE_LAUNCH),     # nq <= 256 in every shape
    # (nq = 256 in latency mode: this 257-body tree's latency layout does not fit the LDS -- pick_spec_shape finds no workgroup --
    #  and the host runs the throughput kernel of the width pick_lanes chose instead; see _LDS_LIMITED_EDGES)
    ("lat32lean-nq256", 256, 8, FREE, 0, _lat(32), None, (32, 8, 2, 1)),
    ("lat32lean-nq257", 257, 8, FREE, 0, _lat(32), None, REFUSE_LAUNCH),
    # nq edges of the generic shapes (fixed root: never lean)
    ("gen8-nq80", 80, 8, FIXED, 8, THR2, None, (8, 10, 2, 0)),
    ("gen8-nq81", 81, 8, FIXED, 8, THR2, None, (8, 16, 2, 0)),
    ("gen8-nq128", 128, 8, FIXED, 8, THR2, None, (8, 16, 2, 0)),
    ("gen8-nq129", 129, 8, FIXED, 8, THR2, None, (16, 16, 2, 0)),     # no 8-lane shape holds 129: the next width
    ("gen16-nq80", 80, 8, FIXED, 16, THR2, None, (16, 5, 2, 0)),
    ("gen16-nq81", 81, 8, FIXED, 16, THR2, None, (16, 8, 2, 0)),
    ("gen16-nq128", 128, 8, FIXED, 16, THR2, None, (16, 8, 2, 0)),
    ("gen16-nq129", 129, 8, FIXED, 16, THR2, None, (16, 16, 2, 0)),
    ("gen16-nq256", 256, 8, FIXED, 16, THR2, None, (16, 16, 2, 0)),
    ("gen16-nq257", 257, 8, FIXED, 16, THR2, None, REFUSE_LAUNCH),
    ("gen16w3-nq80", 80, 8, FIXED, 16, THR3, None, (16, 5, 3, 0)),
    ("gen16w3-nq81", 81, 8, FIXED, 16, THR3, None, (16, 8, 3, 0)),
    ("gen16w3-nq128", 128, 8, FIXED, 16, THR3, None, (16, 8, 3, 0)),
    ("gen16w3-nq129", 129, 8, FIXED, 16, THR3, None, (16, 16, 2, 0)),  # (no 3-per-SIMD shape holds 129: the 2-per-SIMD one)
    ("gen32-nq96", 96, 8, FIXED, 32, THR2, None, (32, 3, 2, 0)),
    ("gen32-nq97", 97, 8, FIXED, 32, THR2, None, (32, 4, 2, 0)),
    ("gen32-nq128", 128, 8, FIXED, 32, THR2, None, (32, 4, 2, 0)),
    ("gen32-nq129", 129, 8, FIXED, 32, THR2, None, (32, 8, 2, 0)),
    ("gen32-nq256", 256, 8, FIXED, 32, THR2, None, (32, 8, 2, 0)),
    ("gen32-nq257", 257, 8, FIXED, 32, THR2, None, REFUSE_LAUNCH),
    ("gen32w4-nq96", 96, 8, FIXED, 32, THR4, None, (32, 3, 4, 0)),
    ("gen32w4-nq97", 97, 8, FIXED, 32, THR4, None, (32, 4, 2, 0)),
    ("gen64-nq128", 128, 8, FIXED, 64, THR2, None, (64, 2, 2, 0)),
    ("gen64-nq129", 129, 8, FIXED, 64, THR2, None, (64, 4, 2, 0)),
    ("gen64w4-nq128", 128, 8, FIXED, 64, THR4, None, (64, 2, 4, 0)),
    ("gen64w4-nq129", 129, 8, FIXED, 64, THR4, None, (64, 4, 2, 0)),
    ("gen64-nq256", 256, 8, FIXED, 64, THR2, None, (64, 4, 2, 0)),
    ("gen64-nq257", 257, 8, FIXED, 64, THR2, None, REFUSE_LAUNCH),
    # latency group width: 8 lanes per role up to nq = 80, 16 up to 128 (stac_q.hip, plan_q)
    ("lat8-nq80", 80, 8, FIXED, 0, _lat(8), None, (8, 10, 2, 8)),
    ("lat8-nq81", 81, 8, FIXED, 0, _lat(8), None, (16, 8, 2, 4)),
    ("lat8R4-nq80", 80, 8, FIXED, 0, dict(_lat(8), STAC_HIP_SPECR="4"), None, (8, 10, 2, 4)),
    ("lat8R4-nq81", 81, 8, FIXED, 0, dict(_lat(8), STAC_HIP_SPECR="4"), None, (16, 8, 2, 4)),
    ("lat16-nq80", 80, 8, FIXED, 0, _lat(16), None, (16, 5, 2, 4)),
    ("lat16-nq81", 81, 8, FIXED, 0, _lat(16), None, (16, 8, 2, 4)),
    ("lat16-nq128", 128, 8, FIXED, 0, _lat(16), None, (16, 8, 2, 4)),
    ("lat16-nq129", 129, 8, FIXED, 0, _lat(16), None, (32, 8, 2, 8)),
    ("lat32-nq96", 96, 8, FIXED, 0, _lat(32), None, (32, 3, 2, 8)),
    ("lat32-nq97", 97, 8, FIXED, 0, _lat(32), None, (32, 8, 2, 8)),
    ("lat32-nq256", 256, 8, FIXED, 0, _lat(32), None, (64, 4, 2, 0)),   # (latency layout too large: throughput fallback)
    ("lat32-nq257", 257, 8, FIXED, 0, _lat(32), None, REFUSE_LAUNCH),
    ("lat64-nq128", 128, 8, FIXED, 0, _lat(64), None, (64, 2, 2, 8)),
    ("lat64-nq129", 129, 8, FIXED, 0, _lat(64), None, (64, 4, 2, 8)),
    ("lat64-nq256", 256, 8, FIXED, 0, _lat(64), None, (64, 4, 2, 0)),   # (latency layout too large: throughput fallback)
    ("lat64-nq257", 257, 8, FIXED, 0, _lat(64), None, REFUSE_LAUNCH),
    # nqpad = (nq + 3) & ~3: every residue
    ("nqpad-12", 12, 6, FREE, 16, THR2, None, (16, 5, 2, 1)),
    ("nqpad-13", 13, 6, FREE, 16, THR2, None, (16, 5, 2, 1)),
    ("nqpad-14", 14, 6, FREE, 16, THR2, None, (16, 5, 2, 1)),
    ("nqpad-15", 15, 6, FREE, 16, THR2, None, (16, 5, 2, 1)),
    # site edges: one and two sites
    ("K1", 19, 1, FREE, 16, THR2, None, (16, 5, 2, 1)),
    ("K2", 19, 2, FREE, 16, THR2, None, (16, 5, 2, 1)),
    ("K1-fixed", 19, 1, FIXED, 8, THR2, None, (8, 10, 2, 0)),
    # lean sites in registers: K <= lean_site_rounds(G, NQR) * G -- 32 at 16 lanes, 32 at 32 lanes with nq <= 96 (NQR 2 / 3:
    # one round), 64 at 32 lanes with NQR 8 (two rounds)
    ("lean16-K32", 40, 32, FREE, 16, THR2, None, (16, 5, 2, 1)),
    ("lean16-K33", 40, 33, FREE, 16, THR2, None, (16, 5, 2, 0)),
    ("lean32-K32", 40, 32, FREE, 32, THR2, None, (32, 3, 2, 1)),
    ("lean32-K33", 40, 33, FREE, 32, THR2, None, (32, 3, 2, 0)),
    ("lat32lean-K32", 40, 32, FREE, 0, _lat(32), None, (32, 2, 2, 9)),   # (32, 2, 8) of the latency lean table holds 40: NQR 2
    ("lat32lean-K33", 40, 33, FREE, 0, _lat(32), None, (32, 3, 2, 8)),
    ("lean32wide-K64", 120, 64, FREE, 32, THR2, None, (32, 8, 2, 1)),
    ("lean32wide-K65", 120, 65, FREE, 32, THR2, None, (32, 4, 2, 0)),    # (generic: <32,4,*> holds 120)
    # generic sites in registers: K <= 3G (same instantiation either side: the LDS loss tree takes over)
    ("gen8-K24", 20, 24, FIXED, 8, THR2, None, (8, 10, 2, 0)),
    ("gen8-K25", 20, 25, FIXED, 8, THR2, None, (8, 10, 2, 0)),
    ("gen16-K48", 20, 48, FIXED, 16, THR2, None, (16, 5, 2, 0)),
    ("gen16-K49", 20, 49, FIXED, 16, THR2, None, (16, 5, 2, 0)),
    ("gen32-K96", 20, 96, FIXED, 32, THR2, None, (32, 3, 2, 0)),
    ("gen32-K97", 20, 97, FIXED, 32, THR2, None, (32, 3, 2, 0)),
    ("gen64-K192", 20, 192, FIXED, 64, THR2, None, (64, 2, 2, 0)),
    ("gen64-K193", 20, 193, FIXED, 64, THR2, None, (64, 2, 2, 0)),
    # K > 64: the c_r2 layout and the end of the root fast path (free root, root optimisation on)
    ("root-K64", 19, 64, FREE, 16, THR2, None, (16, 5, 2, 0)),
    ("root-K65", 19, 65, FREE, 16, THR2, None, (16, 5, 2, 0)),
    ("root-K64-lat", 19, 64, FREE, 0, _lat(8), None, (8, 10, 2, 8)),
    ("root-K65-lat", 19, 65, FREE, 0, _lat(8), None, (8, 10, 2, 8)),
    ("K4096", 10, 4096, FREE, 0, {}, None, FIT_OR_CAPACITY),
    ("K4097", 10, 4097, FREE, 0, {}, None, REFUSE_CREATE),
    # part groups: kinds = P + 3 <= kMaxKinds = 40
    ("P0", 19, 6, FREE, 16, THR2, 0, (16, 5, 2, 1)),
    ("P1-false", 19, 6, FREE, 16, THR2, "false1", (16, 5, 2, 1)),
    ("P37", 19, 6, FREE, 16, THR2, 37, (16, 5, 2, 1)),
    ("P38", 19, 6, FREE, 16, THR2, 38, REFUSE_LAUNCH),
    # one active body
    ("free-root-only", 7, 1, FREE, 16, THR2, None, (16, 5, 2, 1)),            # naj == 1
    ("free-root-only-lat", 7, 1, FREE, 0, _lat(16), None, (16, 3, 2, 5)),
    ("free-root-only-lat32", 7, 2, FREE, 0, _lat(32), None, (32, 2, 2, 9)),
    ("hinge-only", 1, 1, FIXED, 16, THR2, None, (16, 5, 2, 0)),               # nq = 1
    ("slide-root", 4, 2, {"free_root": False, "slide_root": True}, 16, THR2, None, (16, 5, 2, 0)),  # root_dims = 4
    ("oriented-root", 7, 2, {"oriented_root": True}, 16, THR2, None, (16, 5, 2, 1)),
    # other joint / body kinds at the small end
    ("oriented-below", 19, 4, {"oriented": True}, 16, THR2, None, (16, 5, 2, 1)),
    ("ball-K1", 12, 1, {"ball": True}, 16, THR2, None, (16, 5, 2, 0)),
    ("ball-K2", 12, 2, {"ball": True}, 8, THR2, None, (8, 10, 2, 0)),
]

# LM: n (optimised coordinates on the root paths of the sites) <= 192
LM_FITS = "fits"
_LM_EDGE_CASES = [
    ("lm-nq192", 192, 8, FIXED, 0, LM_FITS),         # (eight chains of 24 hinges: the LM kernel holds it, bit for bit)
    ("lm-nq193", 193, 8, FIXED, 0, REFUSE_LAUNCH),   # the same tree with one hinge more: "more than 192 optimised coordinates"
]


def _setup(nq, K, flags, P, rng):
    t = _edge_tables(nq, K, **flags)
    assert (t.nq, t.nsite) == (nq, K)
    lb, ub = _box(t)
    free = int(t.jnt_type[0]) == 0
    slide = bool(flags.get("slide_root"))
    if P is None:
        part = np.zeros((2, nq), np.uint8)
        part[0] = rng.random(nq) < 0.5
        part[1, nq // 2:] = 1
    elif P == "false1":
        part = np.zeros((1, nq), np.uint8)
    else:
        part = (rng.random((P, nq)) < 0.3).astype(np.uint8)
    trunk = (rng.random(K) < 0.6).astype(np.uint8)
    trunk[0] = 1
    kw = dict(part_masks=part, trunk_kps=trunk, root_kp_idx=0, root_dims=4 if slide else 7, do_root_opt=free or slide)
    return t, lb, ub, kw


def _poses(t, lb, ub, orc, n, rng, noise=2e-3):
    q = np.tile(t.qpos0, (n, 1)) + rng.normal(0, 0.15, (n, t.nq)).astype(np.float32)
    q = np.clip(q, np.where(np.isfinite(lb), lb, -3), np.where(np.isfinite(ub), ub, 3)).astype(np.float32)
    kp = np.stack([orc.fk(x.copy())["site_xpos"].reshape(-1) for x in q]).astype(np.float32)
    return q, (kp + rng.normal(0, noise, kp.shape)).astype(np.float32)


def _quat_mat(qs):
    q = qs / np.linalg.norm(qs, axis=-1, keepdims=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def _check_fk(eng, orc, o64, t, q):
    """HIP FK == the oracle bit for bit, and within the float32 bound of the float64 twin."""
    fk = eng.fk(q)
    depth = int(t.body_depth.max())
    for i in range(len(q)):
        r, r64 = orc.fk(q[i].copy()), o64.fk(q[i].copy())
        for k in ("xpos", "xquat", "site_xpos", "qpos"):
            np.testing.assert_array_equal(_np(fk[k][i]), r[k], err_msg=k)
        for k in ("xpos", "site_xpos"):
            got, ref = _np(fk[k][i]).astype(np.float64), np.asarray(r64[k], np.float64)
            tol = _fk_tol(depth, np.abs(ref).max())
            assert np.abs(got - ref).max() <= tol, (k, np.abs(got - ref).max(), tol)
        # quaternions: unit magnitude, the same bound on each component (sign fixed by the twin)
        got, ref = _np(fk["xquat"][i]).astype(np.float64), np.asarray(r64["xquat"], np.float64)
        assert np.abs(got - ref).max() <= _fk_tol(depth, 1.0)


def _check_m_phase(eng, orc, o64, t, q, kp, rng):
    """m_partial / m_finish at T = 1 and T = 3 == the oracle bit for bit; the offsets against the float64 closed form
    m* = (sum_t R_t^T (y_t - p_t) + c d m0) / (T + c d) from float64 poses, and the returned error against the float64 objective
    sum_t ||y_t - p_t - R_t m||^2 + c ||d (m - m0)||^2 at the returned m."""
    K = t.nsite
    depth = int(t.body_depth.max())
    m0 = (t.site_pos + rng.normal(0, 3e-3, (K, 3))).astype(np.float32)
    d = (rng.random((K, 3)) < 0.5).astype(np.float32)
    c = 0.7
    for T in (1, 3):
        part = eng.m_partial(kp[:T], q[:T])
        ref_part = orc.m_partial(kp[:T], q[:T])
        np.testing.assert_array_equal(_np(part), ref_part)
        off, err = eng.m_finish(part, m0, d, c)
        ref_off, ref_err = orc.m_finish(ref_part, m0, d, c)
        np.testing.assert_array_equal(_np(off), ref_off)
        assert float(err) == np.float32(ref_err)
        # float64 closed form
        ps, Rs = [], []
        for i in range(T):
            r = o64.fk(q[i].copy())
            ps.append(np.asarray(r["xpos"], np.float64)[t.site_bodyid])
            Rs.append(_quat_mat(np.asarray(r["xquat"], np.float64)[t.site_bodyid]))
        y = kp[:T].reshape(T, K, 3).astype(np.float64)
        num = sum(np.einsum("kji,kj->ki", Rs[i], y[i] - ps[i]) for i in range(T)) + c * d * m0
        m_star = num / (T + c * d)
        got = _np(off).astype(np.float64)
        scale = max(np.abs(y).max(), np.abs(np.stack(ps)).max(), np.abs(m0).max())
        tol_m = M_ULPS_PER_LEVEL * (depth + 2) * EPS * max(1.0, scale)
        assert np.abs(got - m_star).max() <= tol_m, (T, np.abs(got - m_star).max(), tol_m)
        res = [y[i] - ps[i] - np.einsum("kij,kj->ki", Rs[i], got) for i in range(T)]
        obj = sum((r * r).sum() for r in res) + c * ((d * (got - m0)) ** 2).sum()
        S = sum(((np.abs(y[i] - ps[i]) + np.abs(got)) ** 2).sum() for i in range(T)) + c * ((d * (np.abs(got) + np.abs(m0))) ** 2).sum()
        tol_e = ERR_ULPS_PER_LEVEL * (depth + 2) * EPS * S
        assert abs(float(err) - obj) <= tol_e, (T, float(err), obj, tol_e)


# q_solve: tolerance and bound of the solves whose stopping residual is recomputed in float64 (the starts are the poses the targets
# were made from, so the solves stop well before the bound; every case must check at least one)
QS_TOL, QS_MAXITER = 1e-3, 400


def _residual64_slack(orc, o64, t, x, q0, kp, qs, ks, g32):
    """A bound on |float64 residual - float32 residual| at x, propagated from the float32 kinematics at x (measured against the
    float64 twin there) through the gradient g_i = 2 sum_k J_ki . (p_k - y_k) over the weighted sites:
      dg <= 2 sum_k [Jmax (dp + eps (|p_k| + |y_k|)) + |p_k - y_k| dJ] + 2 K eps sum_k Jmax |p_k - y_k|   (per coordinate)
    with dp, da, dax the f32 errors of site positions, joint anchors and axes, Jmax = c (1 + lever) and dJ = c (dax lever + dp + da)
    (c = 2 / |q| of the least-normalised quaternion coordinate: d R(q / |q|) v / dq <= 2 |v| / |q|; 1 without quaternions); then the
    float32 evaluation of clip(x - g) - x (one rounding of x - g, one of the difference) and of its norm, and the float64
    gradient's own rounding to float32 on output."""
    from stac_mjx_amd.mjcf import JNT_BALL, JNT_FREE

    r32, r64 = orc.fk(x.copy()), o64.fk(x.copy())
    sx, sx64 = r32["site_xpos"].astype(np.float64), r64["site_xpos"].astype(np.float64)
    an, an64 = r32["xanchor"].astype(np.float64), r64["xanchor"].astype(np.float64)
    ax, ax64 = r32["xaxis"].astype(np.float64), r64["xaxis"].astype(np.float64)
    dp = np.abs(sx - sx64).max() + EPS * np.abs(sx64).max()
    da = (np.abs(an - an64).max() + EPS * np.abs(an64).max()) if len(an) else 0.0
    dax = (np.abs(ax - ax64).max() + EPS) if len(ax) else 0.0
    lever = np.abs(sx64).max() * np.sqrt(3) + (np.abs(an64).max() * np.sqrt(3) if len(an) else 0.0)
    c = 1.0
    for j in range(t.njnt):
        a, ty = int(t.jnt_qposadr[j]), int(t.jnt_type[j])
        if ty in (JNT_FREE, JNT_BALL):
            qa = a + 3 if ty == JNT_FREE else a
            c = max(c, 2.0 / np.linalg.norm(x[qa:qa + 4].astype(np.float64)))
    w = ks[::3].astype(bool)
    y = kp.reshape(-1, 3).astype(np.float64)
    e = np.linalg.norm(sx64 - y, axis=1)[w]
    mag = (np.linalg.norm(sx64, axis=1) + np.linalg.norm(y, axis=1))[w]
    Jmax, dJ = c * (1.0 + lever), c * (dax * lever + dp + da)
    dg = 2 * (Jmax * (dp + EPS * mag) + e * dJ).sum() + 2 * w.sum() * EPS * (Jmax * e).sum()
    m = qs.astype(bool)
    n = int(m.sum())
    xm, gm = x[m].astype(np.float64), g32[m].astype(np.float64)
    return np.sqrt(n) * (dg + EPS * np.abs(gm).max(initial=0.0)) + 2 * EPS * (np.linalg.norm(xm) + np.linalg.norm(gm)) + \
        (np.log2(max(n, 1)) + 3) * EPS * QS_TOL


def _check_q_solve(eng, orc, o64, t, lb, ub, q, kp, rng):
    """The q_solve seam with a random coordinate mask, once with a random site mask and once with every site, == the oracle bit for
    bit (iterates, state, counters); every solve that stopped before the bound has, at the point it returned, a float64 stopping
    residual -- the gradient of the SAME masked objective, ||clip(x - g) - x|| in float64 -- within _residual64_slack of the float32
    one, hence within QS_TOL + slack.  (With sites masked, some solves stall above the tolerance in both implementations: the run
    with every site is the one that must reach it.)  Returns how many solves were checked; at least one of every-site run."""
    from oracle import Oracle

    nq, K = t.nq, t.nsite
    qs = (rng.random(nq) < 0.6).astype(np.uint8)
    qs[rng.integers(nq)] = 1
    ks = (rng.random(3 * K) < 0.8).astype(np.uint8)
    ks[:3] = 1
    ks = np.repeat(ks[::3], 3)  # (whole sites: what the solver's callers pass)
    n = len(q)
    eng.params.tol, eng.params.maxiter = QS_TOL, QS_MAXITER
    orc_s = Oracle(t, tol=QS_TOL, maxiter=QS_MAXITER)
    checked = [_q_solve_residuals(eng, orc_s, o64, t, lb, ub, q, kp, qs, k) for k in (ks, np.ones(3 * K, np.uint8))]
    assert checked[1] >= 1, "no solve stopped before the bound: the float64 residual check did not run"
    return sum(checked)


def _q_solve_residuals(eng, orc_s, o64, t, lb, ub, q, kp, qs, ks):
    n = len(q)
    par, st, cn = (_np(v) for v in eng.q_solve(kp[:n], q, qs, ks))
    checked = 0
    for i in range(n):
        xr, sr = orc_s.q_opt(kp[i], qs, ks, q[i], lb, ub)
        np.testing.assert_array_equal(par[i], xr)
        assert cn[i].tolist() == [sr["iter_num"], sr["ls_evals"], sr["grad_evals"], 1]
        np.testing.assert_array_equal(st[i], np.array([sr["error"], sr["stepsize"], sr["t"], sr["loss"]], np.float32))
        if sr["iter_num"] < QS_MAXITER:
            assert sr["error"] <= QS_TOL
            x = par[i]
            _, g32 = orc_s.q_loss(x, kp[i], qs, ks, q[i])
            _, g64 = o64.q_loss(x, kp[i], qs, ks, q[i])
            x64 = x.astype(np.float64)
            r64 = float(np.linalg.norm((np.clip(x64 - g64.astype(np.float64), lb, ub) - x64)[qs.astype(bool)]))
            slack = _residual64_slack(orc_s, o64, t, x, q[i], kp[i], qs, ks, g32)
            assert abs(r64 - float(st[i, 0])) <= slack, (i, r64, float(st[i, 0]), slack)
            assert r64 <= QS_TOL + slack
            checked += 1
    return checked


def _expect_capacity(exc):
    assert "error -3" in str(exc), exc


@pytest.mark.gpu
@pytest.mark.parametrize("case", _EDGE_CASES, ids=[c[0] for c in _EDGE_CASES])
def test_capacity_edge(case, monkeypatch):
    from oracle import Oracle
    from stac_mjx_amd.engine import Engine, StacHipError

    name, nq, K, flags, lanes, env, P, expect = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(sum(map(ord, name)))
    t, lb, ub, kw = _setup(nq, K, flags, P, rng)
    maxiter, tol = 8, 1e-5
    if expect == REFUSE_CREATE:
        with pytest.raises(StacHipError) as ei:
            Engine(t, lb, ub, tol=tol, maxiter=maxiter, lanes_per_chain=lanes)
        _expect_capacity(ei.value)
        return
    eng = Engine(t, lb, ub, tol=tol, maxiter=maxiter, lanes_per_chain=lanes)
    orc, o64 = Oracle(t, tol=tol, maxiter=maxiter), Oracle(t, precision="f64", tol=tol, maxiter=maxiter)
    q, kp = _poses(t, lb, ub, orc, 6, rng)
    _check_fk(eng, orc, o64, t, q[:3])
    _check_m_phase(eng, orc, o64, t, q, kp, rng)
    if expect == REFUSE_LAUNCH:
        with pytest.raises(StacHipError) as ei:
            eng.q_phase(kp.reshape(3, 2, 3 * K), **kw)
        _expect_capacity(ei.value)
        eng.close()
        return
    ref = orc.ik_clips(kp.reshape(3, 2, 3 * K), lb, ub, kw["part_masks"], kw["trunk_kps"], 0, kw["root_dims"], do_root_opt=kw["do_root_opt"])
    try:
        res = _q_phase_twice(eng, kp.reshape(3, 2, 3 * K), **kw)
    except StacHipError as e:
        assert expect == FIT_OR_CAPACITY, (name, e)
        _expect_capacity(e)
        res = None
    if res is not None:
        _compare_phase(res, ref)
        if expect != FIT_OR_CAPACITY:
            assert _last_q_kernel(eng) == expect, (name, _last_q_kernel(eng), expect)
    if res is not None:
        _check_q_solve(eng, orc, o64, t, lb, ub, q[:4], kp, rng)
    eng.close()
    if nq <= 192 and K <= 256:  # the LM solver on the same model, against its oracle statement
        lm = Engine(t, lb, ub, tol=1e-4, solver="lm", lm_maxiter=8)
        a, b = lm.q_phase(kp.reshape(3, 2, 3 * K), **kw), lm.q_phase(kp.reshape(3, 2, 3 * K), **kw)
        ref_lm = Oracle(t, tol=1e-4).ik_clips_lm(kp.reshape(3, 2, 3 * K), lb, ub, kw["part_masks"], kw["trunk_kps"], 0, kw["root_dims"],
                                                 do_root_opt=kw["do_root_opt"], maxiter=8)
        for k in ("qpos", "frame_error", "counters"):
            assert (a[k] == b[k]).all(), k
        np.testing.assert_array_equal(_np(a["qpos"]).view(np.uint32), ref_lm["qpos"].view(np.uint32))
        np.testing.assert_array_equal(_np(a["frame_error"]).view(np.uint32), ref_lm["frame_error"].view(np.uint32))
        np.testing.assert_array_equal(_np(a["counters"]).astype(np.uint32), ref_lm["counters"])
        lm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", _LM_EDGE_CASES, ids=[c[0] for c in _LM_EDGE_CASES])
def test_lm_capacity_edge(case):
    from oracle import Oracle
    from stac_mjx_amd.engine import Engine, StacHipError

    name, nq, K, flags, lanes, expect = case
    rng = np.random.default_rng(sum(map(ord, name)))
    t, lb, ub, kw = _setup(nq, K, flags, 1, rng)
    kw["part_masks"] = np.ones((1, nq), np.uint8)  # (the full pass and the part pass: n = nq)
    orc = Oracle(t, tol=1e-4)
    _, kp = _poses(t, lb, ub, orc, 2, rng)
    kp = kp.reshape(2, 1, 3 * K)
    eng = Engine(t, lb, ub, tol=1e-4, solver="lm", lm_maxiter=6, lanes_per_chain=lanes)
    if expect == REFUSE_LAUNCH:
        with pytest.raises(StacHipError) as ei:
            eng.q_phase(kp, **kw)
        _expect_capacity(ei.value)
        assert "more than 192 optimised coordinates" in str(ei.value), ei.value
        return
    assert expect == LM_FITS, name
    res = eng.q_phase(kp, **kw)
    ref = orc.ik_clips_lm(kp, lb, ub, kw["part_masks"], kw["trunk_kps"], 0, 7, do_root_opt=False, maxiter=6)
    np.testing.assert_array_equal(_np(res["qpos"]).view(np.uint32), ref["qpos"].view(np.uint32))
    np.testing.assert_array_equal(_np(res["frame_error"]).view(np.uint32), ref["frame_error"].view(np.uint32))
    np.testing.assert_array_equal(_np(res["counters"]).astype(np.uint32), ref["counters"])


# ---- CPU: the builder and the table ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _EDGE_CASES + [c[:4] + (0, {}, None, c[5]) for c in _LM_EDGE_CASES], ids=lambda c: c[0])
def test_edge_builder_has_the_requested_shape(case):
    """_edge_tables gives exactly the nq and K the case names, and every joint is an ancestor of a fit site (what the host counts as
    the model's shape); a case on the lean side has a model the lean kernels take (free root, hinges below it)."""
    from stac_mjx_amd.mjcf import JNT_FREE, JNT_HINGE

    name, nq, K, flags = case[:4]
    t = _edge_tables(nq, K, **flags)
    assert (t.nq, t.nsite) == (nq, K), name
    active = set()
    for b in t.site_bodyid:
        b = int(b)
        while b > 0:
            active.add(b)
            b = int(t.body_parentid[b])
    assert active == set(range(1, t.nbody)), name
    exp = case[7]
    if isinstance(exp, tuple) and exp[3] & 1:
        assert int(t.jnt_type[0]) == JNT_FREE and all(int(x) == JNT_HINGE for x in t.jnt_type[1:]), name


def _shape_tables():
    """The shipped (not STAC_INST_SUBSET) STAC_Q_*SHAPES tables of stac_shapes.hpp: {list name: [(G, NQR, third), ...]}."""
    src = (ROOT / "stac_mjx_amd" / "csrc" / "stac_shapes.hpp").read_text()
    shipped = src.split("#ifdef STAC_INST_SUBSET", 1)[1].split("#else", 1)[1].split("#endif", 1)[0]
    out = {}
    for m in re.finditer(r"#define (STAC_Q_\w*SHAPES)\(X\)((?:[^\n]*\\\n)*[^\n]*)", shipped):
        out[m.group(1)] = [tuple(int(v) for v in x) for x in re.findall(r"X\((\d+),\s*(\d+),\s*(\d+)\)", m.group(2))]
    return out


# Latency shapes whose nq edge (256) no model of 256 coordinates reaches in latency mode: the latency layout of such a model (257
# bodies here) exceeds the LDS of a workgroup, so the host falls back to the throughput kernel (pinned by the nq = 256 cases above).
# The shapes themselves run on the mouse (nq = 230) in test_gpu_parity.py::_SHAPE_CASES: q<32,8,2,9>, q<32,8,2,8>, q<64,4,2,8>.
_LDS_LIMITED_EDGES = {("STAC_Q_SPEC_LEAN_SHAPES", 32, 8, 8), ("STAC_Q_SPEC_SHAPES", 32, 8, 8), ("STAC_Q_SPEC_SHAPES", 64, 4, 8)}


def _thr(c):
    return c[5].get("STAC_HIP_SPEC") != "1"


def test_every_shape_edge_has_cases():
    """Every shape of the shipped tables has its own edge in the case table: a case whose expected instantiation IS that shape
    (G, NQR, register cap or role count, lean or generic) at nq = G * NQR, and a case with the same model kind, lane width and
    switches at G * NQR + 1 (the next shape, or a refusal) -- so that a shape added to the tables without both cases, or a case
    deleted, fails here, on the CPU."""
    tabs = _shape_tables()
    assert set(tabs) == {"STAC_Q_LEAN_SHAPES", "STAC_Q_SPEC_LEAN_SHAPES", "STAC_Q_SHAPES", "STAC_Q_SPEC_SHAPES"}, set(tabs)
    assert all(tabs.values())
    missing = []
    for name, shapes in tabs.items():
        lean, spec = "LEAN" in name, "SPEC" in name
        for G, nqr, third in shapes:
            e = G * nqr
            want = (G, nqr, 2, third | int(lean)) if spec else (G, nqr, third, int(lean))
            if (name, G, nqr, third) in _LDS_LIMITED_EDGES:  # (a case at each side of the edge all the same: fallback | refusal)
                fits = [c for c in _EDGE_CASES if c[1] == e and not _thr(c) and c[5].get("STAC_HIP_SPECG") == str(G) and
                        isinstance(c[7], tuple) and c[3] == ({} if "LEAN" in name else FIXED)]
            else:
                fits = [c for c in _EDGE_CASES if c[1] == e and c[7] == want and _thr(c) != spec]
            over = [c for c in _EDGE_CASES for f in fits if c[1] == e + 1 and c[3:7] == f[3:7] and c[2] == f[2]]
            if not fits or not over:
                missing.append((name, G, nqr, third, e, bool(fits), bool(over)))
    assert not missing, missing
    all_nq = {c[1] for c in _EDGE_CASES}
    # the refusals beyond the widest shape, and the other edges of the host
    assert max(G * r for s in tabs.values() for G, r, _ in s) == 256
    assert any(c[1] == 257 and c[7] == REFUSE_LAUNCH for c in _EDGE_CASES)
    assert {1, 2, 4096, 4097} <= {c[2] for c in _EDGE_CASES}
    assert {0, "false1", 37, 38} <= {c[6] for c in _EDGE_CASES}
    assert {nq % 4 for nq in all_nq} == {0, 1, 2, 3}
    assert [(c[1], c[5]) for c in _LM_EDGE_CASES] == [(192, LM_FITS), (193, REFUSE_LAUNCH)]
