"""Test-side restatements of the reference's host sequencing, driven by the CPU oracle.

Shared by the CPU pins (tests/test_pin_demo_viz.py) and the GPU parity tests: the GPU path must equal these
bit for bit, and these are pinned -- in marker space -- to the reference's own stored fit (demos/demo_viz.p).
Also the deterministic model builder of the capacity-edge tests (_edge_tables), which the CPU gradient checks share.
"""

from __future__ import annotations

import numpy as np


def oracle_chain_passes(orc, fs, kp, n_passes, q0=None):
    """stac.py:277-311 with fixed offsets: root optimisation on frame 0, then ``n_passes`` warm-started
    ``pose_optimization`` passes over the same frames, the carried qpos crossing the passes (stac.py:300-301).
    Returns the list of per-pass outputs."""
    q = fs.tables.qpos0 if q0 is None else q0
    if fs.do_root_opt:
        q, _ = orc.root_optimization(kp, q, fs.lb, fs.ub, fs.trunk_kps, fs.root_kp_idx, fs.root_dims)
    outs = []
    for _ in range(n_passes):
        out = orc.pose_optimization(kp, q, fs.lb, fs.ub, fs.part_masks)
        q = out["carry_qpos"]
        outs.append(out)
    return outs


def oracle_fit_offsets(fs, cfgm, kp, n_iters, time_indices=None, history=None):
    """Stac.fit_offsets (stac.py:253-354) driven by the CPU oracle: root optimisation, then ``n_iters`` x
    (pose pass, closed-form offsets regularised toward the previous iterate), then the final pose pass."""
    from oracle import Oracle
    from stac_mjx_amd.prng import sample_time_indices

    orc = Oracle(fs.tables, tol=float(cfgm["FTOL"]), maxiter=int(cfgm["N_ITER_Q"]))
    offsets = fs.tables.site_pos.copy()
    q = fs.tables.qpos0
    if fs.do_root_opt:
        q, _ = orc.root_optimization(kp, q, fs.lb, fs.ub, fs.trunk_kps, fs.root_kp_idx, fs.root_dims)
    idx = sample_time_indices(kp.shape[0], int(cfgm["N_SAMPLE_FRAMES"])) if time_indices is None else np.asarray(time_indices)
    for _ in range(n_iters):
        out = orc.pose_optimization(kp, q, fs.lb, fs.ub, fs.part_masks)
        q = out["carry_qpos"]
        offsets, _ = orc.m_opt(kp[idx], out["qpos"][idx], offsets, fs.is_regularized, float(cfgm["M_REG_COEF"]))
        orc.set_site_pos(offsets)
        if history is not None:
            history.append((out, offsets.copy()))
    out = orc.pose_optimization(kp, q, fs.lb, fs.ub, fs.part_masks)
    return offsets, out


def marker_error_mm(marker_sites, kp):
    """Mean marker-to-keypoint distance in millimetres."""
    m = np.asarray(marker_sites)
    return float(np.linalg.norm(m.reshape(-1, m.shape[-2], 3) - np.asarray(kp).reshape(-1, m.shape[-2], 3), axis=-1).mean() * 1e3)


def pg_residual(orc, fs, q, kp, mask):
    """The stopping residual of jaxopt's ProjectedGradient at q for the coordinates in ``mask``:
    || clip(q - grad) - q ||_2 over the masked coordinates."""
    m = np.asarray(mask).astype(np.uint8)
    _, g = orc.q_loss(q, kp, m, np.ones(3 * fs.tables.nsite, np.uint8), q)
    r = (np.clip(q - g * m, fs.lb, fs.ub) - q) * m
    return float(np.linalg.norm(r))


def _edge_tables(nq, K, *, free_root=True, oriented=False, ball=False, slide_root=False, oriented_root=False, seed=0):
    """A model with exactly nq coordinates and K fit sites: body 1 carries the root (a free joint: 7 coordinates; a slide root:
    three slides and a hinge, root_dims = 4; else the first hinge), every other coordinate is a hinge of its own body (ball=True:
    the first one below the root is a ball joint, 4 coordinates).  The bodies below the root hang in min(K, n) branches of equal
    length; site k < #branches sits on the last body of branch k (so every body is an ancestor of a site: all joints active), the
    others are spread over all bodies.  oriented: every other body below the root has a body_quat; oriented_root: body 1 has one."""
    from stac_mjx_amd.mjcf import JNT_BALL, JNT_FREE, JNT_HINGE, JNT_SLIDE, ModelTables

    rng = np.random.default_rng(1_000_003 * nq + 1009 * K + seed)
    root = [JNT_FREE] if free_root else ([JNT_SLIDE] * 3 + [JNT_HINGE] if slide_root else [JNT_HINGE])
    root_q = {JNT_FREE: 7, JNT_BALL: 4}
    nroot = sum(root_q.get(j, 1) for j in root)
    rest = nq - nroot
    assert rest >= 0, (nq, nroot)
    below = []
    if ball and rest >= 4:
        below.append(JNT_BALL)
        rest -= 4
    below += [JNT_HINGE] * rest
    nb_below = len(below)
    nbody = 2 + nb_below
    nbr = max(1, min(K, nb_below)) if nb_below else 0
    lens = [nb_below // nbr + (1 if i < nb_below % nbr else 0) for i in range(nbr)] if nbr else []
    parent, last = [0, 0], []
    b = 2
    for L in lens:
        for i in range(L):
            parent.append(1 if i == 0 else b - 1)
            b += 1
        last.append(b - 1)
    depth = [0] * nbody
    for i in range(1, nbody):
        depth[i] = depth[parent[i]] + 1

    def unit(v):
        return v / np.linalg.norm(v)

    body_pos = rng.normal(0, 0.05, (nbody, 3))
    body_pos[1] = [0.0, 0.0, 0.1]
    body_quat = np.tile([1.0, 0, 0, 0], (nbody, 1))
    if oriented_root:
        body_quat[1] = unit(rng.normal(0, 1, 4))
    if oriented:
        for i in range(2, nbody, 2):
            body_quat[i] = unit(rng.normal(0, 1, 4))
    jt, jadr, jbody, jpos, jaxis, jrange, qpos0 = [], [], [], [], [], [], []
    body_jntadr, body_jntnum = [-1] * nbody, [0] * nbody
    q = 0

    def add(ty, bd, axis):
        nonlocal q
        if body_jntadr[bd] < 0:
            body_jntadr[bd] = len(jt)
        body_jntnum[bd] += 1
        jt.append(ty)
        jadr.append(q)
        jbody.append(bd)
        jpos.append(np.zeros(3) if rng.random() < 0.4 else rng.normal(0, 0.02, 3))
        jaxis.append(axis)
        if ty == JNT_FREE:
            qpos0.extend([0, 0, 0.1, 1, 0, 0, 0])
            jrange.append([0, 0])
        elif ty == JNT_BALL:
            qpos0.extend([1, 0, 0, 0])
            jrange.append([0, 0])
        else:
            qpos0.append(0.0)
            jrange.append([-1.0, 1.2] if ty == JNT_HINGE else [-0.05, 0.05])
        q += root_q.get(ty, 1)

    for i, ty in enumerate(root):
        add(ty, 1, np.eye(3)[i % 3] if ty == JNT_SLIDE else unit(rng.normal(0, 1, 3)))
    for i, ty in enumerate(below):
        add(ty, 2 + i, unit(rng.normal(0, 1, 3)))
    assert q == nq
    site_body = [last[k] if k < len(last) else 1 + (k * (nbody - 1)) // K for k in range(K)]
    site_body = np.sort(np.array(site_body, np.int32))
    t = ModelTables(
        nbody=nbody, njnt=len(jt), nq=nq, nsite=K, body_parentid=np.array(parent, np.int32),
        body_pos=body_pos.astype(np.float32), body_quat=body_quat.astype(np.float32),
        body_jntadr=np.array(body_jntadr, np.int32), body_jntnum=np.array(body_jntnum, np.int32),
        body_depth=np.array(depth, np.int32), jnt_type=np.array(jt, np.int32), jnt_qposadr=np.array(jadr, np.int32),
        jnt_bodyid=np.array(jbody, np.int32), jnt_pos=np.array(jpos, np.float32).reshape(-1, 3),
        jnt_axis=np.array(jaxis, np.float32).reshape(-1, 3), jnt_range=np.array(jrange, np.float32).reshape(-1, 2),
        qpos0=np.array(qpos0, np.float32), site_bodyid=site_body, site_pos=rng.normal(0, 0.01, (K, 3)).astype(np.float32),
        body_names=[f"b{i}" for i in range(nbody)], jnt_names=[f"j{i}" for i in range(len(jt))],
        site_names=[f"s{i}" for i in range(K)])
    return t
