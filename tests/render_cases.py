"""Scenes of the render tests (tests/test_render_host.py, tests/test_gpu_render.py): the rodent of the reference's fixtures
with the stored demo_viz fit, the synth model, and seeded random scenes of every primitive type."""

from __future__ import annotations

import math

import numpy as np

from conftest import GOLDEN

GEOM_TYPES = (0, 2, 3, 4, 5, 6)  # plane, sphere, capsule, ellipsoid, cylinder, box


def kp_rgba(cfg) -> list:
    cp = cfg["KEYPOINT_COLOR_PAIRS"]
    return [[float(c) for c in cp[k].split()] if isinstance(cp[k], str) else [float(c) for c in cp[k]]
            for k in cfg["KEYPOINT_MODEL_PAIRS"]]


def rodent_scene(reference_dir, cfg):
    from stac_mjx_amd.mjcf import compile_render_scene

    return compile_render_scene(reference_dir / "models" / "rodent.xml", scale=float(cfg["SCALE_FACTOR"]), log=lambda *a: None)


def rodent_frames(tables, demo_viz, idx):
    """xpos, xquat, markers of the stored fit's frames ``idx`` (oracle FK at the stored offsets), and its keypoints."""
    from oracle import Oracle

    o = Oracle(tables)
    o.set_site_pos(demo_viz["offsets"])
    fr = [o.fk(demo_viz["qpos"][i]) for i in idx]
    return (np.stack([f["xpos"] for f in fr]), np.stack([f["xquat"] for f in fr]), np.stack([f["site_xpos"] for f in fr]),
            np.ascontiguousarray(demo_viz["kp_data"][list(idx)], dtype=np.float32))


def qpos0_pose(tables):
    from oracle import Oracle

    f = Oracle(tables).fk(tables.qpos0)
    return f["xpos"], f["xquat"]


def look_at(pos, target, up=(0.0, 0.0, 1.0)):
    """cam[12] of a camera at ``pos`` looking at ``target``."""
    pos, target, up = (np.asarray(v, np.float64) for v in (pos, target, up))
    f = target - pos
    f /= np.linalg.norm(f)
    x = np.cross(f, up)
    x /= np.linalg.norm(x)
    z = -f
    y = np.cross(z, x)
    return np.concatenate([pos, np.stack([x, y, z], 1).reshape(9)]).astype(np.float32)


def _unit_quat(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def random_scene(seed, nbody, K, n_static=60, n_frames=2, layered=True, near=True):
    """Random tables (the ``render_tables`` dict layout), body poses, keypoints, markers and cameras.

    Every primitive type with random sizes, poses and colours; about half of the moving-body primitives transparent;
    planes with checkers; ``layered``: a stack of 12 transparent spheres on the camera axis (more than the 8 layers a pixel
    keeps); ``near``: primitives behind the camera and crossing its near side.  Positions are continuous random draws, so no
    two primitives coincide."""
    rng = np.random.default_rng(seed)
    P = n_static
    types = rng.choice(GEOM_TYPES, size=P)
    body = rng.integers(0, nbody, size=P).astype(np.int32)
    size = rng.uniform(0.01, 0.12, size=(P, 3))
    size[types == 0, :2] = rng.uniform(0.2, 1.0, size=((types == 0).sum(), 2))
    pos = rng.uniform(-0.15, 0.15, size=(P, 3))
    quat = _unit_quat(rng, P)
    rgba = np.concatenate([rng.uniform(0.05, 1.0, size=(P, 3)), np.ones((P, 1))], 1)
    flags = np.where((body != 0) & (rng.random(P) < 0.5), 1, 0).astype(np.int32)
    checker = (types == 0) & (rng.random(P) < 0.7)
    flags |= np.where(checker, 2, 0).astype(np.int32)
    flags |= np.where(checker & (rng.random(P) < 0.5), 4, 0).astype(np.int32)
    xpos = rng.uniform(-0.5, 0.5, size=(n_frames, nbody, 3))
    xquat = _unit_quat(rng, n_frames * nbody).reshape(n_frames, nbody, 4)
    xpos[:, 0], xquat[:, 0] = 0.0, [1.0, 0.0, 0.0, 0.0]
    cams = np.stack([look_at(rng.uniform(-1, 1, 3) * [1, 1, 0.5] + [0, 0, 0.6] + np.sign(rng.uniform(-1, 1, 3)) * [1.2, 1.2, 0],
                             rng.uniform(-0.1, 0.1, 3)) for _ in range(n_frames)])
    if layered:  # 12 transparent spheres in a row along the first camera's axis, on the world body
        c0 = cams[0].astype(np.float64)
        fwd = -c0[3:].reshape(3, 3)[:, 2]
        for j in range(12):
            types = np.append(types, 2)
            body = np.append(body, 0).astype(np.int32)
            size = np.vstack([size, [0.05 + 0.003 * j, 0, 0]])
            pos = np.vstack([pos, c0[:3] + fwd * (0.4 + 0.11 * j) + rng.normal(scale=0.003, size=3)])
            quat = np.vstack([quat, [1, 0, 0, 0]])
            rgba = np.vstack([rgba, np.append(rng.uniform(0.1, 1, 3), 1)])
            flags = np.append(flags, 1).astype(np.int32)
            checker = np.append(checker, False)
    if near:  # behind the first camera, and straddling its position
        c0 = cams[0].astype(np.float64)
        fwd = -c0[3:].reshape(3, 3)[:, 2]
        for off, r in ((-0.3, 0.1), (0.02, 0.05), (-0.01, 0.2)):
            types = np.append(types, 6 if r == 0.2 else 2)
            body = np.append(body, 0).astype(np.int32)
            size = np.vstack([size, [r, r * 0.8, r * 0.6]])
            pos = np.vstack([pos, c0[:3] + fwd * off + rng.normal(scale=0.01, size=3)])
            quat = np.vstack([quat, _unit_quat(rng, 1)])
            rgba = np.vstack([rgba, np.append(rng.uniform(0.1, 1, 3), 1)])
            flags = np.append(flags, 0).astype(np.int32)
            checker = np.append(checker, False)
    P = len(types)
    kp = rng.uniform(-0.3, 0.3, size=(n_frames, K, 3))
    markers = kp + rng.normal(scale=0.01, size=(n_frames, K, 3))
    kp[0, 0] = np.nan  # one missing keypoint
    kp[-1, 1, 2] = np.nan
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    t = dict(
        prim_type=np.ascontiguousarray(types, dtype=np.int32), prim_body=body, prim_flags=np.ascontiguousarray(flags, np.int32),
        prim_size=f32(size), prim_pos=f32(pos), prim_quat=f32(quat), prim_rgba=f32(rgba),
        prim_rgb2=f32(rng.uniform(0, 1, size=(P, 3))), prim_texrepeat=f32(rng.uniform(0.5, 4, size=(P, 2))),
        kp_rgba=f32(np.concatenate([rng.uniform(0, 1, (K, 3)), np.ones((K, 1))], 1)),
        marker_rgba=f32([0, 0, 0, 1]), segment_rgba=f32([1, 0, 0, 1]), marker_radius=np.float32(0.01), segment_radius=np.float32(0.002),
        light_dir=f32([[0, 0, -1], [0.6, 0, -0.8]]), light_diffuse=f32([[0.5, 0.5, 0.5], [0.3, 0.2, 0.1]]),
        head_ambient=f32([0.1, 0.1, 0.1]), head_diffuse=f32([0.4, 0.4, 0.4]), alpha=np.float32(0.3),
        background=f32([0.1, 0.1, 0.12]), names=[f"p{i}" for i in range(P)],
    )
    return t, f32(xpos), f32(xquat), f32(kp), f32(markers), cams, math.tan(math.radians(45) / 2)


def load_demo_viz():
    with np.load(GOLDEN / "demo_viz_golden.npz") as d:
        return {k: d[k] for k in d.files}
