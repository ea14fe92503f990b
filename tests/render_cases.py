"""Scenes and shared helpers of the render tests (tests/test_render_host.py, tests/test_gpu_render.py and their mesh
siblings): the rodent of the reference's fixtures with the stored demo_viz fit, the synth model, seeded random scenes of
every primitive type, the scenes whose pictures are pinned, the checker (tests/tools/build_render_ref.py) and the
comparisons against it; and the constructed scenes on which checker and kernel are held to tests/render_rule.py
(``rule_cases``: every type from outside and from inside, ties, degenerate segments, lights) with that comparison."""

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


# ---- the scenes held to tests/render_rule.py (tests/test_render_rule_host.py, tests/test_gpu_render_rule.py) ---------------
RULE_SIZES = ((96, 64), (97, 61))  # a partial last tile in both directions
RULE_NBODY = 67  # the rodent's body count: the GPU tests create their scenes on its engine
TAN45 = math.tan(math.radians(45) / 2)
_f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)


class RuleCase:
    """One scene of the rule tests: ``args`` is the argument list of ``RenderRef.render`` up to ``tan_half_fovy`` (W and H
    follow).  ``single``: every image shows one primitive (the cap on excluded pixels then counts hit pixels); ``hidden``:
    per frame the id of the solid that holds the camera and must not be seen (the other frames: None)."""

    def __init__(self, name, t, xpos, xquat, kp, markers, show, cams, single=False, hidden=None, tanh=TAN45):
        self.name, self.single, self.hidden = name, single, hidden
        self.args = (t, xpos.shape[1], _f32(xpos), _f32(xquat), kp, markers, show, _f32(cams), tanh)


def rule_tables(types, body, size, pos, quat, rgb, flags, rgb2=None, tex=None, kp_rgb=(), lights=((0, 0, -1),),
                diffuse=((0.7, 0.7, 0.7),), marker_radius=0.01, segment_radius=0.002):
    P = len(types)
    one = lambda a: np.concatenate([np.reshape(a, (-1, 3)), np.ones((len(a), 1))], 1) if len(a) else np.zeros((0, 4))
    return dict(
        prim_type=np.ascontiguousarray(types, np.int32), prim_body=np.ascontiguousarray(body, np.int32),
        prim_flags=np.ascontiguousarray(flags, np.int32), prim_size=_f32(np.reshape(size, (P, 3))),
        prim_pos=_f32(np.reshape(pos, (P, 3))), prim_quat=_f32(np.reshape(quat, (P, 4))), prim_rgba=_f32(one(rgb)),
        prim_rgb2=_f32(np.zeros((P, 3)) if rgb2 is None else rgb2), prim_texrepeat=_f32(np.ones((P, 2)) if tex is None else tex),
        kp_rgba=_f32(one(kp_rgb)), marker_rgba=_f32([0, 0, 0, 1]), segment_rgba=_f32([1, 0, 0, 1]),
        marker_radius=np.float32(marker_radius), segment_radius=np.float32(segment_radius),
        light_dir=_f32(np.reshape(lights, (-1, 3))), light_diffuse=_f32(np.reshape(diffuse, (-1, 3))),
        head_ambient=_f32([0.1, 0.1, 0.1]), head_diffuse=_f32([0.4, 0.4, 0.4]), alpha=np.float32(0.3),
        background=_f32([0.1, 0.1, 0.12]), names=[f"p{i}" for i in range(P)],
    )


def _rot(q):
    from render_rule import quat_matrix

    return quat_matrix(np.asarray(q, np.float32))


def _still_bodies(n_frames, nbody):
    xquat = np.zeros((n_frames, nbody, 4))
    xquat[..., 0] = 1.0
    return np.zeros((n_frames, nbody, 3)), xquat


OUTSIDE_KINDS = ("plane", "plane_checker", "plane_checker_texuniform", "sphere", "capsule", "ellipsoid", "cylinder", "box")


def outside_case(kind, nbody=RULE_NBODY):
    """Eight primitives of one type with anisotropic sizes, primitive k on body k + 1; frame f shows primitive f at a random
    pose from a random side (a plane from its +z side) and has the others behind the camera.  Capsule and cylinder: frame 6
    looks along the axis of a turned solid, frame 7 along the axis of an axis-aligned one, where the centre pixel of an
    odd-sized image has a direction exactly parallel to the axis (the side term's a == 0)."""
    rng = np.random.default_rng(100 + OUTSIDE_KINDS.index(kind))
    n = 8
    ty = {"plane": 0, "plane_checker": 0, "plane_checker_texuniform": 0, "sphere": 2, "capsule": 3, "ellipsoid": 4,
          "cylinder": 5, "box": 6}[kind]
    size = rng.uniform(0.04, 0.15, size=(n, 3))
    if ty == 0:
        size[:, :2] = rng.uniform(0.2, 0.6, size=(n, 2))
    if ty in (3, 5):
        size[:, 1] = rng.uniform(0.05, 0.2, size=n)
    flags = np.full(n, {"plane_checker": 2, "plane_checker_texuniform": 6}.get(kind, 0))
    pos, quat = rng.uniform(-0.05, 0.05, size=(n, 3)), _unit_quat(rng, n)
    xpos, xquat = _still_bodies(n, nbody)
    cams = np.zeros((n, 12), np.float32)
    axis_view = ty in (3, 5)
    if axis_view:
        pos[7], quat[7] = 0.0, [1, 0, 0, 0]
    for f in range(n):
        xpos[f, f + 1], xquat[f, f + 1] = rng.uniform(-0.1, 0.1, 3), _unit_quat(rng, 1)[0]
        if axis_view and f == 7:
            xpos[f, f + 1], xquat[f, f + 1] = 0.0, [1, 0, 0, 0]
        Rb = _rot(xquat[f, f + 1])
        R = Rb @ _rot(quat[f])
        c = _f32(xpos[f, f + 1]).astype(np.float64) + Rb @ _f32(pos[f]).astype(np.float64)
        brad = {0: np.hypot(*size[f, :2]), 2: size[f, 0], 3: size[f, 0] + size[f, 1], 4: size[f].max(),
                5: np.hypot(*size[f, :2]), 6: np.linalg.norm(size[f])}[ty]
        D = brad / rng.uniform(0.22, 0.32)
        side = rng.normal(size=3)
        if ty == 0:  # within 60 degrees of the plane's normal
            nz = R[:, 2] / np.linalg.norm(R[:, 2])
            tang = np.cross(nz, side)
            a = rng.uniform(0.0, math.radians(60))
            side = nz * math.cos(a) + tang / np.linalg.norm(tang) * math.sin(a)
        side /= np.linalg.norm(side)
        if axis_view and f == 7:
            cams[f] = np.concatenate([[0, 0, D], np.eye(3).reshape(9)])
        else:
            if axis_view and f == 6:
                side = R[:, 2] / np.linalg.norm(R[:, 2])
            cams[f] = look_at(c + D * side, c, up=(0.2, 0.3, 0.9))
        back = cams[f, 3:].astype(np.float64).reshape(3, 3)[:, 2]
        for k in range(n):
            if k != f:
                xpos[f, k + 1] = cams[f, :3] + back * (20.0 + 2.0 * k)
    t = rule_tables([ty] * n, np.arange(1, n + 1), size, pos, quat, rng.uniform(0.2, 1.0, (n, 3)), flags,
                    rgb2=rng.uniform(0.0, 1.0, (n, 3)), tex=rng.uniform(1.0, 4.0, (n, 2)),
                    lights=((0, 0, -1), (0.6, 0, -0.8)), diffuse=((0.5, 0.5, 0.5), (0.3, 0.2, 0.1)))
    return RuleCase(f"outside_{kind}", t, xpos, xquat, None, None, False, cams, single=True)


INSIDE_KINDS = ("sphere", "capsule", "ellipsoid", "cylinder", "box")
CAPSULE_INSIDE_VIEWS = {  # frame -> what the view is (r = 0.05, hl = 0.2)
    0: "centre, along the axis", 1: "centre, across the axis",
    2: "cylindrical part outside both cap spheres, along the axis", 3: "cylindrical part outside both cap spheres, across the axis",
    4: "inside a cap sphere beyond the segment's end, towards the other end", 5: "inside a cap sphere beyond the segment's end, outwards",
    6: "inside a cap sphere within the segment, towards the other end",
}


def inside_views(kind):
    """(size, [(origin, direction)]) in the solid's own frame: the camera inside the solid."""
    if kind == "sphere":
        r = 0.11
        return [r, 0, 0], [((0, 0, 0), (0.3, -0.5, 0.8)), ((0.9 * r, 0, 0), (1, 0.1, 0)), ((0, -0.9 * r, 0), (0.1, 1, 0.2))]
    if kind == "capsule":
        r, hl = 0.05, 0.2
        return [r, hl, 0], [((0, 0, 0), (0, 0, 1)), ((0, 0, 0), (1, 0, 0)), ((0.5 * r, 0, 0.3 * hl), (0, 0, 1)),
                            ((0.5 * r, 0, 0.3 * hl), (0, 1, 0.1)), ((0, 0, hl + 0.5 * r), (0, 0, -1)),
                            ((0, 0, hl + 0.5 * r), (0.3, 0, 1)), ((0, 0.3 * r, hl - 0.5 * r), (0, 0, -1))]
    if kind == "ellipsoid":
        s = (0.06, 0.1, 0.18)
        return list(s), [((0, 0, 0), (0.5, 0.5, 0.7)), ((0, 0, 0.9 * s[2]), (0, 0, 1)), ((0, 0, 0.9 * s[2]), (0, 0.1, -1)),
                         ((0.9 * s[0], 0, 0), (1, 0, 0))]
    if kind == "cylinder":
        r, hl = 0.06, 0.15
        return [r, hl, 0], [((0, 0, 0), (0, 0, 1)), ((0, 0, 0), (1, 0, 0)), ((0.3 * r, 0, 0.9 * hl), (0, 0, 1)),
                            ((0.3 * r, 0, 0.9 * hl), (0.1, 0, -1)), ((0.9 * r, 0, 0), (1, 0, 0.2))]
    s = (0.05, 0.09, 0.16)
    return list(s), [((0, 0, 0), (0.4, 0.5, 0.7)), ((0.9 * s[0], 0, 0), (1, 0, 0)), ((0.9 * s[0], 0, 0), (-1, 0.1, 0)),
                     ((0.9 * s[0], 0.9 * s[1], 0.9 * s[2]), (1, 1, 1))]


def inside_case(kind, transparent, nbody=RULE_NBODY):
    """The camera inside solid 0 (body 1, a random pose per frame), an opaque sphere (id 1, body 2) 0.8 ahead of it: the
    solid must not be seen and the sphere must."""
    rng = np.random.default_rng(200 + INSIDE_KINDS.index(kind))
    ty = {"sphere": 2, "capsule": 3, "ellipsoid": 4, "cylinder": 5, "box": 6}[kind]
    size, views = inside_views(kind)
    n = len(views)
    pos, quat = _f32(rng.uniform(-0.05, 0.05, (2, 3))), _f32(_unit_quat(rng, 2))
    pos[1] = 0.0
    xpos, xquat = _still_bodies(n, nbody)
    cams = np.zeros((n, 12), np.float32)
    for f, (o, d) in enumerate(views):
        xpos[f, 1], xquat[f, 1] = rng.uniform(-0.2, 0.2, 3), _unit_quat(rng, 1)[0]
        Rb = _rot(xquat[f, 1])
        R = Rb @ _rot(quat[0])
        c = _f32(xpos[f, 1]).astype(np.float64) + Rb @ pos[0].astype(np.float64)
        ow, dw = c + R @ np.asarray(o, np.float64), R @ (np.asarray(d, np.float64) / np.linalg.norm(d))
        cams[f] = look_at(ow, ow + dw, up=(0.3, 0.5, 0.8))
        xpos[f, 2] = ow + 0.8 * dw
    t = rule_tables([ty, 2], [1, 2], [size, [0.3, 0, 0]], pos, quat, [[0.9, 0.5, 0.2], [0.3, 0.7, 0.9]],
                    [1 if transparent else 0, 0])
    return RuleCase(f"inside_{kind}_{'transparent' if transparent else 'opaque'}", t, xpos, xquat, None, None, False, cams,
                    hidden=[0] * n)


def beyond_end_case(nbody=RULE_NBODY):
    """An origin beyond the end of a capsule (id 0) or cylinder (id 1) but inside the infinite cylinder sees the cap: frames
    0, 1 from beyond the +z ends, frames 2, 3 from beyond the -z ends."""
    rng = np.random.default_rng(300)
    size = [[0.05, 0.2, 0], [0.06, 0.15, 0]]
    pos, quat = _f32(rng.uniform(-0.05, 0.05, (2, 3))), _f32(_unit_quat(rng, 2))
    xpos, xquat = _still_bodies(4, nbody)
    cams = np.zeros((4, 12), np.float32)
    for f in range(4):
        xpos[f, 1], xpos[f, 2] = rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.1, 0.1, 3) + [1.5, 0, 0]
        xquat[f, 1], xquat[f, 2] = _unit_quat(rng, 2)
        i, sgn = f % 2, 1.0 if f < 2 else -1.0
        Rb = _rot(xquat[f, 1 + i])
        R = Rb @ _rot(quat[i])
        c = _f32(xpos[f, 1 + i]).astype(np.float64) + Rb @ pos[i].astype(np.float64)
        r, hl = size[i][0], size[i][1]
        ow = c + R @ np.array([0.3 * r, 0.0, sgn * (hl + (r if i == 0 else 0.0) + 0.15)])
        cams[f] = look_at(ow, ow - sgn * R[:, 2], up=(0.3, 0.5, 0.8))
    t = rule_tables([3, 5], [1, 2], size, pos, quat, [[0.9, 0.5, 0.2], [0.3, 0.7, 0.9]], [0, 0])
    return RuleCase("beyond_end", t, xpos, xquat, None, None, False, cams)


TIE_CLEAR, TIE_OPAQUE = (14, 15), (17, 18)  # the two pairs of equal records in transparency_case


def transparency_case(nbody=RULE_NBODY):
    """Camera at the origin looking along +x.  Ids 0-11: twelve transparent spheres in a row (more than the 8 layers) in front
    of the opaque sphere 12; 13: an opaque box; 14, 15: two transparent spheres with one and the same record (an exactly
    equal entry depth; the tie goes by id) in front of it; 16: a transparent ellipsoid behind the box, showing beside it;
    17, 18: two opaque spheres with the same record."""
    rng = np.random.default_rng(400)
    ty, size, pos, flags = [], [], [], []
    row = np.array([1.0, 0.15, 0.05]) / np.linalg.norm([1.0, 0.15, 0.05])  # a ray of the camera
    for j in range(12):
        ty.append(2), size.append([0.05 + 0.004 * j, 0, 0]), flags.append(1)
        pos.append((0.5 + 0.12 * j) * row + rng.normal(scale=0.004, size=3))
    ty.append(2), size.append([0.3, 0, 0]), pos.append(2.4 * row), flags.append(0)
    ty.append(6), size.append([0.05, 0.2, 0.25]), pos.append([1.6, -0.3, 0.1]), flags.append(0)
    for _ in range(2):
        ty.append(2), size.append([0.032, 0, 0]), pos.append([1.0, -0.25, 0.2]), flags.append(1)
    ty.append(4), size.append([0.2, 0.3, 0.15]), pos.append([2.1, -0.45, 0.1]), flags.append(1)
    for _ in range(2):
        ty.append(2), size.append([0.032, 0, 0]), pos.append([1.0, -0.25, -0.25]), flags.append(0)
    P = len(ty)
    quat = _unit_quat(rng, P)
    for a, b in (TIE_CLEAR, TIE_OPAQUE):
        quat[b] = quat[a]
    xpos, xquat = _still_bodies(1, nbody)
    cams = look_at((0, 0, 0), (1, 0, 0.02))[None]
    rgb = rng.uniform(0.1, 1.0, (P, 3))
    rgb[[14, 17]], rgb[[15, 18]] = [0.9, 0.2, 0.1], [0.1, 0.3, 0.9]  # far apart: the order within a tie shows
    t = rule_tables(ty, [0] * P, size, pos, quat, rgb, flags)
    return RuleCase("transparency", t, xpos, xquat, None, None, False, cams)


def error_segment_case(nbody=RULE_NBODY):
    """Error segments (radius 0.012, wider than the 0.005 keypoint and marker spheres) seen from 0.25 away: keypoint 0 and its
    marker coincide (a segment of length 0), 1: 1e-6 apart (these two, flagged ambiguous all over, from 0.45 away), 2: a NaN in the keypoint, 3: a NaN in the marker, 4 and 5:
    ordinary segments; behind them an opaque plane facing the camera."""
    rng = np.random.default_rng(500)
    K = 6
    kp = np.array([[0.45, -0.18, 0.09], [0.45, -0.09, -0.09], [0.25, 0.0, 0.06], [0.25, 0.04, -0.05], [0.25, 0.08, 0.03],
                   [0.27, -0.02, 0.0]])
    step = rng.normal(size=3)
    mk = kp.copy()
    mk[1] += 1e-6 * step / np.linalg.norm(step)
    mk[2] += [0.0, 0.01, 0.02]
    mk[3] += [0.0, 0.01, -0.02]
    mk[4] += [0.02, 0.03, -0.07]
    mk[5] += [-0.06, -0.03, 0.05]
    kp[2, 1] = np.nan
    mk[3, 2] = np.nan
    h = math.sqrt(0.5)
    t = rule_tables([0], [0], [[0.4, 0.4, 0.01]], [[0.5, 0, 0]], [[h, 0, -h, 0]], [[0.6, 0.6, 0.5]], [0],
                    kp_rgb=rng.uniform(0.2, 1.0, (K, 3)), marker_radius=0.005, segment_radius=0.012)
    xpos, xquat = _still_bodies(1, nbody)
    cams = look_at((0, 0, 0), (1, 0, 0))[None]
    return RuleCase("error_segments", t, xpos, xquat, _f32(kp[None]), _f32(mk[None]), True, cams)


def lights_case(lit, nbody=RULE_NBODY):
    """A sphere, an ellipsoid, a box and a cylinder over a plane, from above and from below.  ``lit`` False: no <light>, the
    headlight alone; True: two lights whose sum with the headlight exceeds 1 on the upper sides, while every normal of the
    undersides seen from below faces away from both."""
    rng = np.random.default_rng(600)
    ty = [0, 2, 4, 6, 5]
    size = [[0.6, 0.6, 0.01], [0.1, 0, 0], [0.08, 0.14, 0.05], [0.07, 0.1, 0.05], [0.06, 0.09, 0]]
    pos = [[0, 0, -0.2], [-0.2, 0.15, 0], [0.15, 0.2, 0.02], [0.2, -0.15, 0], [-0.15, -0.2, 0.03]]
    quat = _unit_quat(rng, 5)
    quat[0] = [1, 0, 0, 0]
    lights = ((0, 0, -1), (0.6, 0, -0.8)) if lit else np.zeros((0, 3))
    diffuse = ((0.8, 0.8, 0.8), (0.7, 0.6, 0.5)) if lit else np.zeros((0, 3))
    t = rule_tables(ty, [0] * 5, size, pos, quat, rng.uniform(0.3, 1.0, (5, 3)), [0] * 5, lights=lights, diffuse=diffuse)
    xpos, xquat = _still_bodies(2, nbody)
    cams = np.stack([look_at((0.5, -0.6, 0.7), (0, 0, 0)), look_at((0.3, 0.4, -0.9), (0, 0, 0))])
    return RuleCase(f"lights_{'two' if lit else 'none'}", t, xpos, xquat, None, None, False, cams)


def rule_cases(nbody=RULE_NBODY) -> dict:
    """name -> RuleCase: every constructed scene of the rule tests (the random scenes and the rodent are added by the tests)."""
    cases = [outside_case(k, nbody) for k in OUTSIDE_KINDS]
    cases += [inside_case(k, tr, nbody) for k in INSIDE_KINDS for tr in (False, True)]
    cases += [beyond_end_case(nbody), transparency_case(nbody), error_segment_case(nbody), lights_case(False, nbody),
              lights_case(True, nbody)]
    return {c.name: c for c in cases}


_RULE_PICTURES = {}


def rule_picture(name, args, W, H):
    """``render_rule.render`` of a scene, computed once per (name, size) and shared by the tests of a run (read only)."""
    import render_rule

    if (name, W, H) not in _RULE_PICTURES:
        out = render_rule.render(*args, W, H)
        for a in out:
            a.setflags(write=False)
        _RULE_PICTURES[(name, W, H)] = out
    return _RULE_PICTURES[(name, W, H)]


def excluded_share(mask, hit, single):
    """Share of an image's pixels that ``mask`` takes out of a comparison; for a single-primitive image of which fewer than
    20 % of the pixels hit anything, the share of the hit pixels (the cap would otherwise hide a thin primitive entirely)."""
    if single and hit.mean() < 0.2:
        return (mask & hit).sum() / max(int(hit.sum()), 1)
    return mask.mean()


def eroded(m):
    """The pixels of a mask whose four neighbours are in it too."""
    out = m.copy()
    out[1:] &= m[:-1]
    out[:-1] &= m[1:]
    out[:, 1:] &= m[:, :-1]
    out[:, :-1] &= m[:, 1:]
    out[0] = out[-1] = False
    out[:, 0] = out[:, -1] = False
    return out


def compare_with_rule(got, rule, amb, single=False, depth_rtol=1e-5, what=""):
    """rgb, seg, depth of a build (or of the kernel) against ``render_rule`` on every pixel that neither the double build's
    ``amb`` nor the rule's ``edge`` marks: seg and hit / no-hit equal, rgb within one quantisation step, depth within
    ``depth_rtol`` relative.  The excluded pixels are at most AMB_CAP of each image (``excluded_share``).  Returns the
    largest relative depth difference and the largest excluded share."""
    rgb, seg, depth = got[:3]
    r_rgb, r_seg, r_depth, edge = rule
    worst_rel, worst_share = 0.0, 0.0
    for f in range(len(seg)):
        mask = amb[f].astype(bool) | edge[f]
        share = excluded_share(mask, r_seg[f] >= 0, single)
        worst_share = max(worst_share, share)
        assert share <= AMB_CAP, f"{what} frame {f}: {share:.4f} of the pixels are excluded"
        ok = ~mask
        bad = np.argwhere((seg[f] != r_seg[f]) & ok)
        first = tuple(bad[0]) if bad.size else None
        assert bad.size == 0, f"{what} frame {f} seg: {len(bad)} pixels differ, first (y, x) {first}: {seg[f][first]} vs rule {r_seg[f][first]}"
        assert (np.isinf(depth[f]) == np.isinf(r_depth[f]))[ok].all(), f"{what} frame {f}: hit / no hit differs"
        diff = np.abs(rgb[f].astype(int) - r_rgb[f].astype(int)).max(-1)
        bad = np.argwhere((diff > 1) & ok)
        first = tuple(bad[0]) if bad.size else None
        assert bad.size == 0, f"{what} frame {f} rgb: {len(bad)} pixels off by more than 1, first (y, x) {first}: {rgb[f][first]} vs rule {r_rgb[f][first]}"
        fin = ok & np.isfinite(r_depth[f])
        if fin.any():
            rel = np.abs(depth[f][fin].astype(np.float64) - r_depth[f][fin]) / r_depth[f][fin]
            worst_rel = max(worst_rel, float(rel.max()))
            assert rel.max() <= depth_rtol, f"{what} frame {f} depth: relative difference {rel.max():.3e} > {depth_rtol:.1e}"
    return worst_rel, worst_share
