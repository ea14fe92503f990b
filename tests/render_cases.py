"""Scenes and shared helpers of the render tests (tests/test_render_host.py, tests/test_gpu_render.py and their mesh
siblings): the rodent of the reference's fixtures with the stored demo_viz fit, the synth model, seeded random scenes of
every primitive type, the scenes whose pictures are pinned, the checker (tests/tools/build_render_ref.py) and the
comparisons against it."""

from __future__ import annotations

import hashlib
import math
import sys

import numpy as np
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, str(ROOT / "tests" / "tools"))
from build_render_ref import RenderRef  # noqa: E402,F401

GEOM_TYPES = (0, 2, 3, 4, 5, 6)  # plane, sphere, capsule, ellipsoid, cylinder, box
AMB_CAP = 0.01  # at most 1 % of an image's pixels may be flagged ambiguous by the double build (a condition, not a tolerance)
SENTINEL = 0xAB


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


def rodent_render_args(scene, cfg, camera, idx=(0, 25, 49), W=480, H=300):
    """The argument list of ``RenderRef.render`` for the stored fit's frames ``idx`` of the rodent through ``camera``,
    error segments on."""
    from stac_mjx_amd.mjcf import ModelTables
    from stac_mjx_amd.render import camera_frames, render_tables

    tables = ModelTables.load(GOLDEN / "rodent_tables_legacy.npz")
    xpos, xquat, mk, kp = rodent_frames(tables, load_demo_viz(), list(idx))
    x0, q0 = qpos0_pose(tables)
    cam, tanh = camera_frames(scene, tables.body_parentid, camera, torch.tensor(xpos), torch.tensor(xquat), x0, q0)
    t = render_tables(scene, kp_rgba(cfg), float(cfg["MARKER_SIZE"]))
    return t, tables.nbody, xpos, xquat, kp, mk, True, cam.float().numpy(), tanh, W, H


def pinned_scenes(rodent, cfg):
    """(name, RenderRef.render arguments) of the mesh-free scenes whose pictures tests/golden/render_ref_digests.json pins."""
    for seed in (0, 1, 2, 3):
        t, xpos, xquat, kp, markers, cams, tanh = random_scene(seed, 67, 23, n_frames=2)
        for W, H in ((160, 120), (97, 61)):
            for show in (False, True):
                yield f"random{seed}/{W}x{H}/show_error={int(show)}", (t, 67, xpos, xquat, kp, markers, show, cams, tanh, W, H)
    for camera in (0, 2, 4, 5, -1):
        yield f"rodent_camera{camera}/480x300/show_error=1", rodent_render_args(rodent, cfg, camera)


def picture_digests(rodent, cfg) -> dict:
    """SHA-256 of the raw bytes of rgb, seg, depth and amb of every pinned scene, float and double build."""
    out = {}
    for real in ("float", "double"):
        ref = RenderRef(real)
        for name, args in pinned_scenes(rodent, cfg):
            for what, a in zip(("rgb", "seg", "depth", "amb"), ref.render(*args)):
                out[f"{name}/{real}/{what}"] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return out


def compare_builds(refs, args):
    """The f32 build against the f64 build on every pixel the f64 build does not flag as ambiguous.

    Ambiguous pixels.  Each decision of a pixel is a sign test of a computed quantity whose float32 evaluation carries a
    relative error of a few units of 2^-24 of the inputs it is formed from.  For a quadric (sphere, ellipsoid after its
    map to the unit sphere, the side of a capsule or cylinder), the test is h2 = r^2 - |p|^2 >= 0 with p the closest point
    of the ray to the axis or centre: p is formed from o - c, so its error is about eps |o - c|, and that of h2 about
    2 r eps |o - c|.  The margin |h2| / r^2 is therefore compared with 64 x 2^-24 times the condition number |o - c| / r.
    The linear tests (slab overlap and face choice of a box, |z| <= half length, a plane's extent, the checker edges) use
    the same factor on their absolute margin against |o - c|.  Depth ties (the two nearest opaque hits, the order of
    transparent hits and their order against the opaque one) use the relative gap.  64 leaves room for the dozen
    roundings on the path of each quantity.

    Bounds on the other pixels.  seg is exact.  RGB may differ by one quantisation step, where a colour lies within float32
    noise of a rounding boundary.  Depth: the entry distance t = tca - sqrt(h2 / a) of the closest-approach form has an
    absolute error of a few ulp of |o - c|; relative to t this stays near 1e-7 where t is comparable to |o - c| and grows
    only for primitives that reach close to the camera, so 1e-5 is the bound (measured: at most 5e-6 on the random scenes
    with primitives crossing the camera's near side, below 1.2e-6 on the rodent)."""
    r32, r64 = refs
    a = r32.render(*args)
    b = r64.render(*args)
    amb = b[3].astype(bool)
    frac = amb.mean(axis=(1, 2))
    print("ambiguous fraction per image:", frac)
    assert (frac <= AMB_CAP).all(), frac
    ok = ~amb
    np.testing.assert_array_equal(a[1][ok], b[1][ok])
    assert np.abs(a[0].astype(int) - b[0].astype(int))[ok].max() <= 1
    fin = ok & np.isfinite(b[2])
    assert (np.isinf(a[2]) == np.isinf(b[2]))[ok].all()
    rel = np.abs(a[2][fin].astype(np.float64) - b[2][fin]) / np.abs(b[2][fin])
    print("max relative depth difference:", rel.max() if rel.size else 0.0)
    assert rel.size == 0 or rel.max() <= 1e-5
    return a, b


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda:0", dtype=dtype) if a is not None else None


def gpu_render(handle, xpos, xquat, kp, markers, show_error, cam, tanh, W, H, want_seg=True, want_depth=True):
    """stac_render on outputs prefilled with a sentinel byte; returns numpy rgb, seg, depth."""
    N = cam.shape[0]
    rgb = torch.full((N, H, W, 3), SENTINEL, dtype=torch.uint8, device="cuda:0")
    seg = torch.full((N * H * W * 4,), SENTINEL, dtype=torch.uint8, device="cuda:0").view(torch.int32).view(N, H, W) if want_seg else None
    depth = torch.full((N * H * W * 4,), SENTINEL, dtype=torch.uint8, device="cuda:0").view(torch.float32).view(N, H, W) if want_depth else None
    handle.render(_dev(xpos), _dev(xquat), _dev(kp), _dev(markers), show_error, _dev(cam), tanh, W, H, rgb, seg, depth)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), seg.cpu().numpy() if want_seg else None, depth.cpu().numpy() if want_depth else None


def assert_same(got, want, what=""):
    for name, g, w in zip(("rgb", "seg", "depth"), got, want):
        if g is None:
            continue
        if name == "depth":
            g, w = g.view(np.uint32), w.view(np.uint32)  # bit for bit, +inf included
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what} {name}: {len(bad)} values differ, first at {bad[:3].tolist()}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}"
