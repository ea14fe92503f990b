"""Shared by tests/test_tree_shapes_host.py and tests/test_gpu_tree_shapes.py: hand-built trees whose DEPTH and WIDTH sit on the
limits the host planner decides by (stac_planner.hip, build_fk3_program: n1 <= 254, n3 <= 252 in PlanHeader::fk3_n; stac_q.hip /
stac_device.hpp fk_chain: 4 * max_width <= G, max_width <= G), plain Python restatements of the facts the cases are chosen by, and the
keypoints of a case.  The trees are built on test_gpu_offsets_fk._tree_tables (random body offsets, anchors and axes from a seed)."""

from __future__ import annotations

import numpy as np

from fk3_cases import lean_box  # noqa: F401  (the box of every case here)
from test_gpu_offsets_fk import _tree_tables

TOL, MAXITER = 1e-5, 10
CHAINS, FRAMES = 8, 2
IDENTITY = np.array([1, 0, 0, 0], np.float32)


# ---- builders --------------------------------------------------------------------------------------------------------------------
def _finish(t, *, oriented=(), zero_jnt_pos=False, zero_body_pos=False, keep_body_pos=()):
    """_tree_tables orients every body and draws every offset: keep the orientation of `oriented` bodies only (body 1 never: the
    root's own orientation is another path, test_gpu_boundaries "oriented-root"), and zero what the case wants zero."""
    quat = np.tile(IDENTITY, (t.nbody, 1))
    for b in oriented:
        quat[b] = t.body_quat[b]
    t.body_quat = quat.astype(np.float32)
    if zero_jnt_pos:
        t.jnt_pos = np.zeros_like(t.jnt_pos)
    if zero_body_pos:
        keep = t.body_pos.copy()
        t.body_pos = np.zeros_like(t.body_pos)
        for b in keep_body_pos:
            t.body_pos[b] = keep[b]
    return t


def _root(free_root):
    from stac_mjx_amd.mjcf import JNT_FREE, JNT_HINGE

    return [JNT_FREE] if free_root else [JNT_HINGE]


def chain(D, *, oriented=False, zero_jnt_pos=False, zero_body_pos=False, spacers=0, free_root=True):
    """Body 1 with the root joint, below it a serial chain of D hinge bodies; `spacers` jointless bodies with body_pos != 0 are spread
    evenly between them (each adds one P3 rotation and no coordinate).  Sites on the root body, the middle and the last body."""
    from stac_mjx_amd.mjcf import JNT_HINGE

    n = D + spacers
    is_spacer = [False] * n
    for i in range(spacers):  # evenly, never the last body (which carries a site and keeps its hinge)
        is_spacer[(i * n) // max(spacers, 1)] = True
    assert sum(is_spacer) == spacers and (n == 0 or spacers == 0 or not is_spacer[-1])
    parent = [0] + list(range(n + 1))
    joints = {1: _root(free_root)}
    hinge_bodies = [2 + i for i in range(n) if not is_spacer[i]]
    for b in hinge_bodies:
        joints[b] = [JNT_HINGE]
    last = n + 1
    t = _tree_tables(parent, joints, [1, 1 + (n + 1) // 2, last], 5000 + 7 * D + spacers + (1 << 12) * oriented)
    return _finish(t, oriented=hinge_bodies if oriented else (), zero_jnt_pos=zero_jnt_pos, zero_body_pos=zero_body_pos,
                   keep_body_pos=[2 + i for i in range(n) if is_spacer[i]])


def star(W, *, tail=0, oriented=False, free_root=True, idle=0):
    """Body 1 with the root joint, a hub (body 2, a hinge) below it, W hinge leaves under the hub and `tail` further hinge bodies in a
    chain under the first leaf.  Sites on the root body, on every leaf but the first and at the end of the first leaf's chain.
    `idle` further hinge leaves carry no site: bodies of the model that are no active bodies of the plan."""
    from stac_mjx_amd.mjcf import JNT_HINGE

    parent = [0, 0, 1] + [2] * (W + idle)
    for i in range(tail):
        parent.append(3 if i == 0 else len(parent) - 1)
    nbody = len(parent)
    joints = {b: [JNT_HINGE] for b in range(2, nbody)}
    joints[1] = _root(free_root)
    sites = [1] + list(range(4, 3 + W)) + [nbody - 1 if tail else 3]
    t = _tree_tables(parent, joints, sites, 6000 + 11 * W + tail + 101 * idle + (1 << 12) * oriented + (1 << 13) * free_root)
    return _finish(t, oriented=range(3, 3 + W) if oriented else ())


def fixed_star(W, *, oriented=False, idle=0):
    """star(W) under a fixed root (body 1 carries a hinge): never lean."""
    return star(W, oriented=oriented, free_root=False, idle=idle)


def broom(D, W):
    """A chain of D hinge bodies under the free root, the last of them carrying W hinge leaves.  Sites on the root body and every leaf."""
    from stac_mjx_amd.mjcf import JNT_FREE, JNT_HINGE

    parent = [0] + list(range(D + 1)) + [D + 1] * W
    joints = {b: [JNT_HINGE] for b in range(2, len(parent))}
    joints[1] = [JNT_FREE]
    return _finish(_tree_tables(parent, joints, [1] + list(range(D + 2, D + 2 + W)), 7000 + 13 * D + W))


# ---- the facts the cases are chosen by ---------------------------------------------------------------------------------------------
def active_bodies(t, all_bodies=False):
    """The bodies that are ancestors of a fit site (build_plan: the only ones the q_phase kernels evaluate)."""
    if all_bodies:
        return set(range(1, t.nbody))
    act = set()
    for b in t.site_bodyid:
        b = int(b)
        while b > 0 and b not in act:
            act.add(b)
            b = int(t.body_parentid[b])
    return act


def body_depths(t):
    d = [0] * t.nbody
    for b in range(1, t.nbody):
        d[b] = d[int(t.body_parentid[b])] + 1
    return d


def active_depths(t):
    """{active body: its depth} (the root body: 1)."""
    d = body_depths(t)
    return {b: d[b] for b in sorted(active_bodies(t))}


def max_width(t, all_bodies=False):
    """PlanHeader::max_width: the largest number of ACTIVE bodies at one depth (stac_planner.hip: lev_adr[l + 1] - lev_adr[l] over the
    levels of the active bodies)."""
    d = body_depths(t)
    count = {}
    for b in active_bodies(t, all_bodies):
        count[d[b]] = count.get(d[b], 0) + 1
    return max(count.values())


def path_depth(t):
    return max(active_depths(t).values())


# ---- a case: keypoints, part groups and the oracle's answer ------------------------------------------------------------------------
_REF = {}


def case(key, t, lb, ub, trunk, *, do_root_opt, chains=CHAINS, frames=FRAMES, tol=TOL, maxiter=MAXITER):
    """As test_gpu_fk3_rounds._case: qpos0 + N(0, 0.15) clipped to the box, the oracle's sites plus N(0, 2e-3), two random part
    groups; computed once per (key, do_root_opt) and shared by the launches that check it.  -> (kp, part, oracle result)"""
    k = (key, bool(do_root_opt))
    if k not in _REF:
        from oracle import Oracle

        rng = np.random.default_rng(4242 + sum(map(ord, str(key))))
        orc = Oracle(t, tol=tol, maxiter=maxiter)
        n = chains * frames
        q = np.tile(t.qpos0, (n, 1)) + rng.normal(0, 0.15, (n, t.nq)).astype(np.float32)
        q = np.clip(q, np.where(np.isfinite(lb), lb, -3), np.where(np.isfinite(ub), ub, 3)).astype(np.float32)
        kp = np.stack([orc.fk(x.copy())["site_xpos"].reshape(-1) for x in q]).astype(np.float32)
        kp = (kp + rng.normal(0, 2e-3, kp.shape)).astype(np.float32).reshape(chains, frames, 3 * t.nsite)
        part = np.zeros((2, t.nq), np.uint8)
        part[0] = rng.random(t.nq) < 0.5
        part[1] = rng.random(t.nq) < 0.15
        ref = orc.ik_clips(kp, lb, ub, part, trunk, 0, 7, do_root_opt=do_root_opt)
        _REF[k] = (kp, part, ref)
    return _REF[k]


def trunk_two(t):
    """The trunk of the depth cases: the first and the last site."""
    trunk = np.zeros(t.nsite, np.uint8)
    trunk[[0, -1]] = 1
    return trunk


# ---- the models the host and the GPU module share ----------------------------------------------------------------------------------
# (what, builder) of the program-size table: serial chains under a free root
PROGRAM_ROWS = [
    # id, builder, nq, (fk3, n1, n2, n3, nrot)
    ("chain24", lambda: chain(24), 31, (1, 24, 80, 72, 72)),
    ("chain83", lambda: chain(83), 90, (1, 84, 256, 252, 249)),
    ("chain84", lambda: chain(84), 91, (1, 84, 256, 252, 252)),
    ("chain85", lambda: chain(85), 92, (0,)),
    ("chain249-nojp", lambda: chain(249, zero_jnt_pos=True), 256, (1, 250, 256, 252, 249)),
    ("chain249-nojp-nobp", lambda: chain(249, zero_jnt_pos=True, zero_body_pos=True), 256, (1, 250, 0, 0, 0)),
    ("chain127-or", lambda: chain(127, oriented=True, zero_jnt_pos=True), 134, (1, 254, 128, 128, 127)),
    ("chain128-or", lambda: chain(128, oriented=True, zero_jnt_pos=True), 135, (0,)),
]
SPACER_D = 73  # nq = 80: the most coordinates a 16-lane lean shape holds


def spacer_chain_full_p3():
    """(spacers, tables) of the chain of SPACER_D hinges with the most spacers the lean kernels still take (n3 = 252), by search."""
    from fk3_cases import fk3_program

    best = None
    for s in range(0, 64):
        t = chain(SPACER_D, spacers=s)
        info, _ = fk3_program(t, *lean_box(t))
        if info["fk3"]:
            best = (s, t, info)
        elif best is not None:
            return best
    raise AssertionError("no spacer count at which the program falls out")
