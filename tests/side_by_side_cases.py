"""Shared by tests/test_gpu_side_by_side_rounds.py: lean models built directly -- a free root with only hinges below it, an exact
number of hinges and of sites, a chosen set of trunk keypoints -- with their keypoints and the oracle's answer, computed once per case
and never changed.  Building a model and asking the host for its split-kinematics program needs no device."""

from __future__ import annotations

import numpy as np

from fk3_cases import fk3_program, lean_box

MAXITER, TOL = 30, 1e-4
_REF = {}


def hinge_model(n_hinges, n_sites, seed, one_body=False):
    """World, a root body with a free joint, and below it bodies of one or two hinges each (`n_hinges` in all) in depth-first order with
    random parents; `n_sites` sites on random bodies in (body, site) order -- or all on one body in the middle of the tree (one_body).
    Identity body orientations, some body and joint offsets exactly zero: what the lean kernels take (tests/test_gpu_parity._random_tables)."""
    from stac_mjx_amd.mjcf import JNT_FREE, JNT_HINGE, ModelTables

    rng = np.random.default_rng(909000 + 1000 * n_hinges + 10 * n_sites + seed)
    per_body = []
    left = n_hinges
    while left:
        n = min(left, 2 if rng.random() < 0.3 else 1)
        per_body.append(n)
        left -= n
    nbody = 2 + len(per_body)
    parent = [0] * nbody
    for b in range(2, nbody):  # depth-first numbering: the parent is on the path from the root to body b - 1
        path = [b - 1]
        while path[-1] > 1:
            path.append(parent[path[-1]])
        parent[b] = path[0] if rng.random() < 0.6 else int(rng.choice(path))
    depth = [0] * nbody
    for b in range(1, nbody):
        depth[b] = depth[parent[b]] + 1
    body_pos = rng.normal(0, 0.05, (nbody, 3))
    for b in range(2, nbody):
        if rng.random() < 0.15:
            body_pos[b] = 0.0
    body_quat = np.tile([1.0, 0, 0, 0], (nbody, 1))
    jt, jadr, jbody, jpos, jaxis, jrange, qpos0 = [JNT_FREE], [0], [1], [np.zeros(3)], [np.eye(3)[2]], [[0, 0]], [0, 0, 0.1, 1, 0, 0, 0]
    body_jntadr, body_jntnum = [-1] * nbody, [0] * nbody
    body_jntadr[1], body_jntnum[1] = 0, 1
    nq = 7
    for b in range(2, nbody):
        body_jntadr[b], body_jntnum[b] = len(jt), per_body[b - 2]
        for _ in range(per_body[b - 2]):
            v = rng.normal(0, 1, 3)
            jt.append(JNT_HINGE)
            jadr.append(nq)
            jbody.append(b)
            jpos.append(np.zeros(3) if rng.random() < 0.4 else rng.normal(0, 0.02, 3))
            jaxis.append(v / np.linalg.norm(v) if rng.random() < 0.5 else np.eye(3)[rng.integers(3)])
            jrange.append([-1.0, 1.2])
            qpos0.append(float(rng.normal(0, 0.05)) if rng.random() < 0.3 else 0.0)
            nq += 1
    if one_body:
        site_body = np.full(n_sites, 1 + nbody // 2, np.int32)
    else:
        site_body = np.sort(rng.integers(1, nbody, n_sites)).astype(np.int32)
    t = ModelTables(
        nbody=nbody, njnt=len(jt), nq=nq, nsite=n_sites, body_parentid=np.array(parent, np.int32),
        body_pos=body_pos.astype(np.float32), body_quat=body_quat.astype(np.float32),
        body_jntadr=np.array(body_jntadr, np.int32), body_jntnum=np.array(body_jntnum, np.int32),
        body_depth=np.array(depth, np.int32), jnt_type=np.array(jt, np.int32), jnt_qposadr=np.array(jadr, np.int32),
        jnt_bodyid=np.array(jbody, np.int32), jnt_pos=np.array(jpos, np.float32).reshape(-1, 3),
        jnt_axis=np.array(jaxis, np.float32).reshape(-1, 3), jnt_range=np.array(jrange, np.float32).reshape(-1, 2),
        qpos0=np.array(qpos0, np.float32), site_bodyid=site_body, site_pos=rng.normal(0, 0.01, (n_sites, 3)).astype(np.float32),
        body_names=[f"b{i}" for i in range(nbody)], jnt_names=[f"j{i}" for i in range(len(jt))],
        site_names=[f"s{i}" for i in range(n_sites)])
    assert t.njnt == n_hinges + 1 and t.nq == n_hinges + 7 and t.nsite == n_sites
    return t


def trunk_sites(n_sites, count, seed=0):
    """`count` trunk keypoints of `n_sites`, site 0 and site n_sites - 1 always among them (count 1 on one site: that site)."""
    trunk = np.zeros(n_sites, np.uint8)
    trunk[0] = trunk[n_sites - 1] = 1
    rest = [k for k in range(1, n_sites - 1)]
    need = count - int(trunk.sum())
    assert 0 <= need <= len(rest), (n_sites, count)
    if need:
        trunk[np.random.default_rng(31 + seed).choice(rest, need, replace=False)] = 1
    assert int(trunk.sum()) == count
    return trunk


def case(key, t, trunk, chains=5, frames=2, do_root_opt=True, tol=TOL):
    """-> (lb, ub, keypoints [chains, frames, 3 K], part masks, the oracle's answer, the oracle) of a model: poses around the rest pose
    (the root's position and raw quaternion as well), by a different amount per clip and with noise on the keypoints of every other clip,
    so that the solves of the chains of a wavefront differ in length; two part groups.  The model must be one the lean kernels take (asked of the host's plan construction, no device)."""
    if key not in _REF:
        from oracle import Oracle

        lb, ub = lean_box(t)
        assert fk3_program(t, lb, ub)[0]["fk3"], "not a model of the lean kernels"
        rng = np.random.default_rng(5150 + sum(map(ord, str(key))))
        orc = Oracle(t, tol=tol, maxiter=MAXITER)
        n = chains * frames
        # (clips at different distances from the rest pose, the second one on it: their solves take different numbers of iterations)
        far = np.repeat(np.resize(np.array([1.0, 0.0, 0.3, 0.05], np.float32), chains), frames)[:, None]
        q = np.tile(t.qpos0, (n, 1)) + far * rng.normal(0, 0.15, (n, t.nq)).astype(np.float32)
        q = np.clip(q, np.where(np.isfinite(lb), lb, -3), np.where(np.isfinite(ub), ub, 3)).astype(np.float32)
        kp = np.stack([orc.fk(x.copy())["site_xpos"].reshape(-1) for x in q]).astype(np.float32)
        noisy = np.repeat(np.resize(np.array([1.0, 0.0, 1.0, 0.0], np.float32), chains), frames)[:, None]  # (every other clip can be fitted exactly)
        kp = (kp + noisy * rng.normal(0, 2e-3, kp.shape)).astype(np.float32).reshape(chains, frames, 3 * t.nsite)
        part = np.zeros((2, t.nq), np.uint8)
        part[0] = rng.random(t.nq) < 0.5
        part[1] = rng.random(t.nq) < 0.15
        ref = orc.ik_clips(kp, lb, ub, part, trunk, 0, 7, do_root_opt=do_root_opt)
        _REF[key] = (lb, ub, kp, part, ref, orc)
    return _REF[key]


def root_solve_lengths(orc, t, lb, ub, kp, trunk, chains):
    """Evaluations (line-search candidates + gradients) of the root solve of each of the first `chains` clips, on the host."""
    out = []
    for c in range(chains):
        st = orc.root_optimization(kp[c], t.qpos0, lb, ub, trunk, 0, 7)[1]
        out.append(st["ls_evals"] + st["grad_evals"])
    return out
