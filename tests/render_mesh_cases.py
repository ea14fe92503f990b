"""Mesh scenes of the render tests (tests/test_render_mesh_host.py, tests/test_gpu_render_mesh.py): procedural meshes
(icosphere, torus, open sheet, triangle-soup cube), writers of the three file formats, seeded random scenes that mix every
primitive type with mesh instances, and the hand-made scene of the awkward cases."""

from __future__ import annotations

import math
import struct

import numpy as np

from render_cases import _unit_quat, look_at, random_scene


# ---- procedural meshes: [T, 3, 3] float32 ---------------------------------------------------------------------------------
def icosphere(subdiv: int, radius: float = 1.0) -> np.ndarray:
    """20 x 4^subdiv triangles with their vertices on the sphere of ``radius`` (outward winding)."""
    p = (1.0 + math.sqrt(5.0)) / 2.0
    v = np.array([[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p],
                  [p, 0, -1], [p, 0, 1], [-p, 0, -1], [-p, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10],
                  [8, 6, 7], [9, 8, 1]])
    t = v[f]
    t /= np.linalg.norm(t, axis=2, keepdims=True)
    for _ in range(subdiv):
        a, b, c = t[:, 0], t[:, 1], t[:, 2]
        ab, bc, ca = (a + b), (b + c), (c + a)
        ab, bc, ca = (m / np.linalg.norm(m, axis=1, keepdims=True) for m in (ab, bc, ca))
        t = np.concatenate([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1), np.stack([c, ca, bc], 1), np.stack([ab, bc, ca], 1)])
    return np.ascontiguousarray(t * radius, dtype=np.float32)


def _grid(P: np.ndarray, wrap_u: bool, wrap_v: bool) -> np.ndarray:
    nu, nv = P.shape[:2]
    tris = []
    for i in range(nu if wrap_u else nu - 1):
        for j in range(nv if wrap_v else nv - 1):
            a, b = P[i, j], P[(i + 1) % nu, j]
            c, d = P[(i + 1) % nu, (j + 1) % nv], P[i, (j + 1) % nv]
            tris += [[a, b, c], [a, c, d]]
    return np.asarray(tris, np.float32)


def torus(R: float = 0.1, r: float = 0.03, nu: int = 24, nv: int = 12) -> np.ndarray:
    u, v = np.meshgrid(np.linspace(0, 2 * np.pi, nu, endpoint=False), np.linspace(0, 2 * np.pi, nv, endpoint=False), indexing="ij")
    P = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1)
    return _grid(P, True, True)


def sheet(a: float = 0.1, b: float = 0.07, n: int = 6, bump: float = 0.01) -> np.ndarray:
    """An open, slightly bumpy rectangle in the xy plane: both of its sides can be seen."""
    x, y = np.meshgrid(np.linspace(-a, a, n + 1), np.linspace(-b, b, n + 1), indexing="ij")
    P = np.stack([x, y, bump * np.sin(9 * x / a) * np.cos(7 * y / b)], -1)
    return _grid(P, False, False)


def cube_soup(h=(1.0, 1.0, 1.0), centre=(0.0, 0.0, 0.0)) -> np.ndarray:
    """12 triangles of the box with half sizes ``h`` around ``centre`` (outward winding)."""
    s = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], np.float64)
    q = [[0, 3, 2, 1], [4, 5, 6, 7], [0, 1, 5, 4], [2, 3, 7, 6], [1, 2, 6, 5], [0, 4, 7, 3]]
    f = [[a, b, c] for a, b, c, d in q] + [[a, c, d] for a, b, c, d in q]
    return np.ascontiguousarray(s[np.asarray(f)] * np.asarray(h) + np.asarray(centre), dtype=np.float32)


def with_degenerates(tri: np.ndarray) -> np.ndarray:
    """``tri`` with zero-area triangles mixed in: repeated vertices, and three equal ones, lying across the mesh."""
    t = np.asarray(tri, np.float32)
    a, b = t[0, 0], t[-1, 2]
    extra = np.array([[a, a, b], [a, b, b], [b, a, b], [a, a, a]], np.float32)
    return np.ascontiguousarray(np.concatenate([extra[:2], t, extra[2:]]))


# ---- file writers -----------------------------------------------------------------------------------------------------------
def write_stl_binary(path, tri):
    tri = np.asarray(tri, np.float32)
    with open(path, "wb") as fh:
        fh.write(b"binary stl written by the tests".ljust(80, b" "))
        fh.write(struct.pack("<I", len(tri)))
        for t in tri:
            n = np.cross(t[1] - t[0], t[2] - t[0])
            fh.write(struct.pack("<12fH", *n, *t.reshape(-1), 0))


def write_stl_ascii(path, tri):
    with open(path, "w") as fh:
        fh.write("solid test\n")
        for t in np.asarray(tri, np.float32):
            fh.write(" facet normal 0 0 0\n  outer loop\n")
            for v in t:
                fh.write(f"   vertex {float(v[0])!r} {float(v[1])!r} {float(v[2])!r}\n")
            fh.write("  endloop\n endfacet\n")
        fh.write("endsolid test\n")


def write_obj(path, tri, negative=False, extras=True):
    """One ``v`` per corner, faces ``i/j/k`` (or negative indices), with ``vt`` / ``vn`` / comment / group lines between."""
    tri = np.asarray(tri, np.float32)
    with open(path, "w") as fh:
        fh.write("# written by the tests\no thing\n")
        for k, t in enumerate(tri):
            for v in t:
                fh.write(f"v {float(v[0])!r} {float(v[1])!r} {float(v[2])!r}\n")
            if extras:
                fh.write("vt 0.5 0.5\nvn 0 0 1\ns off\n")
            if negative:
                fh.write("f -3//1 -2//1 -1//1\n" if extras else "f -3 -2 -1\n")
            else:
                i = 3 * k + 1
                fh.write(f"f {i}/1/1 {i + 1}/1/1 {i + 2}/1/1\n" if extras else f"f {i} {i + 1}/1 {i + 2}\n")


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def library(subdivs=(0, 1, 2, 3), rng=None) -> list:
    """stac_mjx_amd.mesh.Mesh objects: icospheres of the given subdivisions, a torus, an open sheet, a cube with
    zero-area triangles in it."""
    from stac_mjx_amd.mesh import make_mesh

    rng = rng or np.random.default_rng(0)
    out = [make_mesh(f"ico{s}", icosphere(s, float(rng.uniform(0.04, 0.12)))) for s in subdivs]
    out.append(make_mesh("torus", torus()))
    out.append(make_mesh("sheet", sheet()))
    out.append(make_mesh("cube", with_degenerates(cube_soup((0.05, 0.04, 0.03), (0.02, 0.0, -0.01)))))
    return out


def add_meshes(t: dict, meshes: list, prim_mesh, body, pos, quat, rgba, flags) -> dict:
    """The tables ``t`` (render_tables layout) with mesh instances appended as static primitives, and its ``meshes`` entry."""
    from stac_mjx_amd.mesh import pack_meshes

    n = len(prim_mesh)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    P0 = len(t["prim_type"])
    out = dict(t)
    out["prim_type"] = np.ascontiguousarray(np.concatenate([t["prim_type"], np.full(n, 7)]), dtype=np.int32)
    out["prim_body"] = np.ascontiguousarray(np.concatenate([t["prim_body"], body]), dtype=np.int32)
    out["prim_flags"] = np.ascontiguousarray(np.concatenate([t["prim_flags"], flags]), dtype=np.int32)
    out["prim_size"] = f32(np.concatenate([t["prim_size"], np.zeros((n, 3))]))
    out["prim_pos"] = f32(np.concatenate([t["prim_pos"], np.reshape(pos, (n, 3))]))
    out["prim_quat"] = f32(np.concatenate([t["prim_quat"], np.reshape(quat, (n, 4))]))
    out["prim_rgba"] = f32(np.concatenate([t["prim_rgba"], np.reshape(rgba, (n, 4))]))
    out["prim_rgb2"] = f32(np.concatenate([t["prim_rgb2"], np.zeros((n, 3))]))
    out["prim_texrepeat"] = f32(np.concatenate([t["prim_texrepeat"], np.ones((n, 2))]))
    out["names"] = list(t["names"]) + [f"mesh{i}" for i in range(n)]
    m = pack_meshes(meshes)
    m["prim_mesh"] = np.ascontiguousarray(np.concatenate([np.full(P0, -1), prim_mesh]), dtype=np.int32)
    out["meshes"] = m
    return out


def random_mesh_scene(seed, nbody, K, n_mesh=12, subdivs=(0, 1, 2, 3), n_static=40, n_frames=2, layered=True, near=True):
    """``random_scene`` plus ``n_mesh`` mesh instances: meshes drawn from :func:`library` (fewer meshes than instances, so
    meshes are shared by geoms with different poses), random bodies and poses, about half of those on moving bodies
    see-through (instance 0: opaque and in view of the first camera); with ``layered`` also five see-through instances
    stacked behind the twelve see-through spheres on the first camera's axis (more than 8 layers on those rays, meshes
    among them)."""
    t, xpos, xquat, kp, markers, cams, tanh = random_scene(seed, nbody, K, n_static=n_static, n_frames=n_frames, layered=layered, near=near)
    rng = np.random.default_rng(1000 + seed)
    lib = library(subdivs, rng)
    pm = rng.integers(0, len(lib), size=n_mesh)
    body = rng.integers(0, nbody, size=n_mesh)
    pos = rng.uniform(-0.15, 0.15, size=(n_mesh, 3))
    quat = _unit_quat(rng, n_mesh)
    rgba = np.concatenate([rng.uniform(0.05, 1.0, size=(n_mesh, 3)), np.ones((n_mesh, 1))], 1)
    flags = np.where((body != 0) & (rng.random(n_mesh) < 0.5), 1, 0)
    # instance 0 is opaque, on the world body, in front of the first camera and off its axis (clear of the see-through
    # stack): whatever the draws above, a mesh is the nearest opaque hit of some pixels of frame 0
    c0 = cams[0].astype(np.float64)
    Rc = c0[3:].reshape(3, 3)
    body[0], flags[0] = 0, 0
    pos[0] = c0[:3] - Rc[:, 2] * 0.35 + Rc[:, 0] * 0.12 + Rc[:, 1] * 0.08
    if layered:
        c0 = cams[0].astype(np.float64)
        fwd = -c0[3:].reshape(3, 3)[:, 2]
        for j in range(5):
            pm = np.append(pm, j % len(lib))
            body = np.append(body, 0)
            pos = np.vstack([pos, c0[:3] + fwd * (0.45 + 0.2 * j) + rng.normal(scale=0.003, size=3)])
            quat = np.vstack([quat, _unit_quat(rng, 1)])
            rgba = np.vstack([rgba, np.append(rng.uniform(0.1, 1, 3), 1)])
            flags = np.append(flags, 1)
    return add_meshes(t, lib, pm, body, pos, quat, rgba, flags), xpos, xquat, kp, markers, cams, tanh


def _empty_tables(K=1):
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(
        prim_type=np.zeros(0, np.int32), prim_body=np.zeros(0, np.int32), prim_flags=np.zeros(0, np.int32),
        prim_size=f32(np.zeros((0, 3))), prim_pos=f32(np.zeros((0, 3))), prim_quat=f32(np.zeros((0, 4))),
        prim_rgba=f32(np.zeros((0, 4))), prim_rgb2=f32(np.zeros((0, 3))), prim_texrepeat=f32(np.zeros((0, 2))),
        kp_rgba=f32(np.ones((K, 4))), marker_rgba=f32([0, 0, 0, 1]), segment_rgba=f32([1, 0, 0, 1]),
        marker_radius=np.float32(0.01), segment_radius=np.float32(0.002),
        light_dir=f32([[0, 0, -1], [0.6, 0, -0.8]]), light_diffuse=f32([[0.5, 0.5, 0.5], [0.3, 0.2, 0.1]]),
        head_ambient=f32([0.1, 0.1, 0.1]), head_diffuse=f32([0.4, 0.4, 0.4]), alpha=np.float32(0.3),
        background=f32([0.1, 0.1, 0.12]), names=[],
    )


def static_scene(meshes, inst, cams, nbody=1, K=1, extra=None):
    """Tables of mesh instances ``inst`` = [(mesh index, pos, quat, rgba, flags)] on the world body (plus the primitives of
    ``extra``, a tables dict), seen by the cameras ``cams`` (one frame each); no keypoints."""
    t = extra if extra is not None else _empty_tables(K)
    n = len(inst)
    t = add_meshes(t, meshes, [i[0] for i in inst], np.zeros(n, np.int32), [i[1] for i in inst], [i[2] for i in inst],
                   [i[3] for i in inst], [i[4] for i in inst])
    N = len(cams)
    xpos = np.zeros((N, nbody, 3), np.float32)
    xquat = np.zeros((N, nbody, 4), np.float32)
    xquat[..., 0] = 1
    kp = np.full((N, K, 3), np.nan, np.float32)
    return t, xpos, xquat, kp, kp.copy(), np.stack(cams).astype(np.float32), math.tan(math.radians(45) / 2)


def pad_bodies(scene, nbody):
    """A scene made for one body, for an engine with ``nbody`` bodies (the others at the origin, unused)."""
    t, xpos, xquat, kp, markers, cams, tanh = scene
    N = xpos.shape[0]
    xp = np.zeros((N, nbody, 3), np.float32)
    xq = np.zeros((N, nbody, 4), np.float32)
    xq[..., 0] = 1
    xp[:, : xpos.shape[1]], xq[:, : xquat.shape[1]] = xpos, xquat
    return t, xp, xq, kp, markers, cams, tanh


def big_sphere_scene(eng, subdiv):
    from stac_mjx_amd.mesh import make_mesh

    m = make_mesh("big", icosphere(subdiv, 0.5))
    cams = [look_at([1.3, 0.2, 0.9], [0, 0, 0.6]), look_at([0.0, 0.0, 0.6], [1.0, 0.2, 0.7])]  # outside, filling the frame; inside
    sc = static_scene([m], [(0, [0, 0, 0.6], [1, 0, 0, 0], [0.7, 0.7, 0.9, 1], 0)], cams, K=eng.K)
    t = dict(sc[0])
    t["kp_rgba"] = np.ones((eng.K, 4), np.float32)
    return pad_bodies((t,) + sc[1:], eng.nbody)


def awkward_scene(subdiv=3):
    """Grazing rays, a camera inside a mesh, an open sheet seen from both sides, coincident faces of two instances (opaque
    and see-through: ties by id) and zero-area triangles."""
    from stac_mjx_amd.mesh import make_mesh

    meshes = [make_mesh("shell", icosphere(subdiv, 0.5)), make_mesh("sheet", sheet(0.3, 0.2, 8, 0.0)),
              make_mesh("cube", with_degenerates(cube_soup((0.05, 0.05, 0.05)))), make_mesh("bumpy", sheet(0.2, 0.2, 10, 0.02))]
    I = [1.0, 0.0, 0.0, 0.0]
    inst = [
        (0, [0, 0, 0.6], I, [0.8, 0.3, 0.2, 1], 0),          # the shell around the first camera
        (2, [0.1, 0, 0.6], I, [0.2, 0.8, 0.2, 1], 0),        # a cube inside it
        (1, [2, 0, 0.5], I, [0.2, 0.3, 0.9, 1], 0),          # flat sheet: seen from above, from below, and along its plane
        (2, [0, 2, 0.3], I, [0.9, 0.9, 0.1, 1], 0),          # two opaque cubes in the same place
        (2, [0, 2, 0.3], I, [0.1, 0.9, 0.9, 1], 0),
        (2, [0.2, 2, 0.3], I, [0.9, 0.1, 0.9, 1], 1),        # two see-through cubes in the same place
        (2, [0.2, 2, 0.3], I, [0.1, 0.1, 0.9, 1], 1),
        (3, [-2, 0, 0.3], I, [0.6, 0.6, 0.6, 1], 1),         # a bumpy see-through sheet seen at a shallow angle
    ]
    cams = [look_at([0.0, 0.0, 0.6], [0.1, 0.0, 0.6]), look_at([2.0, 0.1, 1.2], [2.0, 0.0, 0.5]), look_at([2.0, 0.1, -0.2], [2.0, 0.0, 0.5]),
            look_at([2.0, -1.0, 0.5], [2.0, 0.0, 0.5]), look_at([0.1, 1.2, 0.5], [0.1, 2.0, 0.3]), look_at([-2.0, -1.0, 0.32], [-2.0, 0.0, 0.3]),
            look_at([0.1, 2.0, 1.0], [0.1, 2.0, 0.3], up=(0, 1, 0))]
    return static_scene(meshes, inst, cams)
