"""Shared by tests/test_gpu_transition.py: the cases of the solver transition of the lean throughput kernels -- models on the register
and lane edges of the nq-sums, line searches whose first candidate is accepted, steps taken without evaluation (small `maxls`), poses
outside the box -- with their keypoints and the oracle's answer, computed once per case and never changed, and what the oracle's
counters say about each case (asked on the host, before any launch).  No device is needed to build a case."""

from __future__ import annotations

import numpy as np

from fk3_cases import fk3_program, lean_box
from side_by_side_cases import MAXITER, TOL, hinge_model, trunk_sites

# free root + hinges -> nq = 8, 16, 17, 32, 48, 49, 80: a last register partly filled (8, 17, 49), whole padding registers (8, 16, 17,
# 32, 49 at five registers), the boundary between the three- and the five-register kernels (48 / 49), every lane holding a coordinate
# in every register (48 at three registers, 80 at five)
EDGE_HINGES = (1, 9, 10, 25, 41, 42, 73)
_REF = {}


def edge_model(hinges):
    return hinge_model(hinges, 6 if hinges < 9 else 12, seed=11)


def trans_case(key, t, trunk, chains=5, frames=2, tol=TOL, maxls=15, spread=0.15, outside=False, data=None, root_in_parts=True):
    """-> (lb, ub, keypoints [chains, frames, 3 K], part masks, the oracle's answer, the oracle).  As side_by_side_cases.case, with the
    oracle's `maxls`; `outside`: the poses that generate the keypoints are NOT clipped into the box and lie beyond both of its sides, so
    the projection binds below and above in the candidates and in the stopping residual; `data`: the key that seeds the keypoints, for
    cases that solve the same keypoints under different parameters (default: the case's own key)."""
    if key not in _REF:
        from oracle import Oracle

        lb, ub = lean_box(t)
        assert fk3_program(t, lb, ub)[0]["fk3"], "not a model of the lean kernels"
        rng = np.random.default_rng(6160 + sum(map(ord, str(key if data is None else data))))
        orc = Oracle(t, tol=tol, maxiter=MAXITER, maxls=maxls)
        n = chains * frames
        far = np.repeat(np.resize(np.array([1.0, 0.0, 0.3, 0.05], np.float32), chains), frames)[:, None]
        if outside:
            far = np.maximum(far, 0.7)
        q = np.tile(t.qpos0, (n, 1)) + far * rng.normal(0, spread, (n, t.nq)).astype(np.float32)
        lo, hi = np.where(np.isfinite(lb), lb, -3), np.where(np.isfinite(ub), ub, 3)
        if outside:
            q[:, 7:] += far * rng.choice(np.array([-2.4, 0.0, 2.6], np.float32), (n, t.nq - 7))
            assert (q[:, 7:] < lo[7:]).any() and (q[:, 7:] > hi[7:]).any()
        else:
            q = np.clip(q, lo, hi)
        q = q.astype(np.float32)
        kp = np.stack([orc.fk(x.copy())["site_xpos"].reshape(-1) for x in q]).astype(np.float32)
        noisy = np.repeat(np.resize(np.array([1.0, 0.0, 1.0, 0.0], np.float32), chains), frames)[:, None]
        kp = (kp + noisy * rng.normal(0, 2e-3, kp.shape)).astype(np.float32).reshape(chains, frames, 3 * t.nsite)
        part = np.zeros((2, t.nq), np.uint8)
        part[0] = rng.random(t.nq) < 0.5
        part[1] = rng.random(t.nq) < 0.15
        if not root_in_parts:
            part[:, :7] = 0
        ref = orc.ik_clips(kp, lb, ub, part, trunk, 0, 7, do_root_opt=True)
        _REF[key] = (lb, ub, kp, part, ref, orc)
    return _REF[key]


def single_evaluation_iterations(counters):
    """Frames [chains, frames] of the oracle's counters {iterations, line-search evaluations, gradients, solves} in which some solve has
    an iteration whose line search took its FIRST candidate: every iteration evaluates at least one, so fewer than two per iteration
    on the frame's sum means one with exactly one."""
    c = counters.astype(np.int64)
    return c[..., 1] < 2 * c[..., 0]


def forced_frames(counters_free, maxls):
    """Frames in which a line search limited to `maxls` evaluations takes a step without evaluation, read from the counters of the
    SAME keypoints solved with the default limit: a limited chain without such a step would be the free chain, evaluation for
    evaluation, and a frame whose free solves spent more than `maxls` evaluations per iteration has an iteration that rejected `maxls`
    candidates -- so every chain with such a frame takes at least one step without evaluation."""
    c = counters_free.astype(np.int64)
    return c[..., 1] > maxls * c[..., 0]
