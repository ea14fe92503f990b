"""Cases and checkers of the ground clearance (stac.ground), shared by tests/test_ground_host.py and tests/test_gpu_ground.py:
``cpu_rule``, a CPU build of the rule of csrc/ground/stac_ground.hpp (ground_reference, through host_scaffold.build_cpu_library);
``judge``, a numpy float32 judge that shares none of its code (whole-array operations, one rounding each, argmin and boolean masks
instead of the serial pass); the shapes; and ``reference_fit``, the reference's stored fit as xpos / xquat with the rodent's scene."""

import ctypes as C

import numpy as np

import host_scaffold as hs

DRIVER = r"""
#include "ground/stac_ground.hpp"
extern "C" void ground_rule(const float *xpos, const float *xquat, long long N, int nbody, const int *meta, const float *data, int G,
                            const float *verts, int S, float z_ref, float *low_z, int *low_geom, float *track_z, float *geom_min,
                            long long *geom_below) {
    stac::ground_reference(xpos, xquat, N, nbody, (const int32_t *)meta, data, G, verts, S, z_ref, low_z, (int32_t *)low_geom, track_z,
                           geom_min, (int64_t *)geom_below);
}
extern "C" int ground_check(const int *m, int nbody, int S, int V) { return stac::ground_check_geom((const int32_t *)m, nbody, S, V); }
extern "C" long long ground_tiles(long long n) { return stac::ground_tiles_per_group(n); }
"""

OUTPUTS = ("low_z", "low_geom", "track_z", "geom_min", "geom_below")
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX, MESH = 2, 3, 4, 5, 6, 7
TYPES = (SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX, MESH)
KEY_INF = np.uint32(0xFF800000)
KEY_NONE = np.uint32(0xFFFFFFFF)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def cpu_rule(tmp_path_factory):
    """-> (clearance(xpos, xquat, meta, data, verts, S, z_ref) -> dict of the five outputs (numpy), the library)"""
    lib = hs.build_cpu_library(tmp_path_factory, "ground", DRIVER)
    lib.ground_rule.restype = None
    lib.ground_rule.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float] + [C.c_void_p] * 5
    lib.ground_check.restype = C.c_int
    lib.ground_check.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.ground_tiles.restype = C.c_longlong
    lib.ground_tiles.argtypes = [C.c_longlong]

    def clearance(xpos, xquat, meta, data, verts, S, z_ref=0.0):
        p, q = _f32(xpos), _f32(xquat)
        N, nbody = p.shape[:2]
        meta, data, verts = np.ascontiguousarray(meta, dtype=np.int32), _f32(data), _f32(verts).reshape(-1, 3)
        G = meta.shape[0]
        out = {"low_z": np.full(N, -7.0, np.float32), "low_geom": np.full(N, -7, np.int32), "track_z": np.full((N, S), -7.0, np.float32),
               "geom_min": np.full(G, -7.0, np.float32), "geom_below": np.full(G, -7, np.int64)}
        lib.ground_rule(p.ctypes.data, q.ctypes.data, N, nbody, meta.ctypes.data, data.ctypes.data, G, verts.ctypes.data if verts.size else None, S,
                        float(z_ref), *[out[k].ctypes.data if out[k].size else None for k in OUTPUTS])
        return out

    return clearance, lib


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, label=""):
    """Tolerance 0 on every word of the five outputs"""
    for k in OUTPUTS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (label, k, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(bits(g), bits(w)):
            i = np.argwhere(bits(g) != bits(w))[0]
            raise AssertionError((label, k, tuple(i), g[tuple(i)], w[tuple(i)], int((bits(g) != bits(w)).sum())))


# ---- the numpy float32 judge -------------------------------------------------------------------------------------------------------
def _key(a):
    """The order of the floats as unsigned integers, -0 below +0"""
    b = _f32(a).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def judge_z(xpos, xquat, meta, data, verts):
    """z_g [N, G] as whole-array float32 operations"""
    p, q, data, verts = _f32(xpos), _f32(xquat), _f32(data), _f32(verts).reshape(-1, 3)
    body, typ = meta[:, 1], meta[:, 0]
    one, two = np.float32(1), np.float32(2)
    with np.errstate(all="ignore"):
        w, x, y, z = (q[:, body, i] for i in range(4))
        b0, b1, b2 = two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)
        s0, s1, s2, p0, p1, p2 = (data[None, :, i] for i in range(6))
        R = data[:, 6:].reshape(-1, 3, 3)
        cz = p[:, body, 2] + ((b0 * p0 + b1 * p1) + b2 * p2)
        r0, r1, r2 = ((b0 * R[None, :, 0, j] + b1 * R[None, :, 1, j]) + b2 * R[None, :, 2, j] for j in range(3))
        h = {SPHERE: s0 + np.zeros_like(cz), CAPSULE: s0 + np.abs(r2) * s1,
             ELLIPSOID: np.sqrt(((r0 * s0) * (r0 * s0) + (r1 * s1) * (r1 * s1)) + (r2 * s2) * (r2 * s2)),
             CYLINDER: np.abs(r2) * s1 + s0 * np.sqrt(r0 * r0 + r1 * r1), BOX: (np.abs(r0) * s0 + np.abs(r1) * s1) + np.abs(r2) * s2}
        zg = np.full(cz.shape, np.float32(0), np.float32)
        for t, ht in h.items():
            zg = np.where(typ[None, :] == t, cz - ht, zg)
        for g in np.flatnonzero(typ == MESH):
            v = verts[meta[g, 4]: meta[g, 4] + meta[g, 5]]
            d = (r0[:, g, None] * v[None, :, 0] + r1[:, g, None] * v[None, :, 1]) + r2[:, g, None] * v[None, :, 2]
            lowest = _unkey(_key(d).min(axis=1))
            zg[:, g] = np.where(np.isfinite(d).all(axis=1), cz[:, g] + lowest, QNAN)
    return zg.astype(np.float32)


def judge(xpos, xquat, meta, data, verts, S, z_ref=0.0):
    """The rule as whole-array float32 operations -> the five outputs"""
    meta = np.asarray(meta, np.int32)
    zg = judge_z(xpos, xquat, meta, data, verts)
    N, G = zg.shape
    fin = np.isfinite(zg)
    key = np.where(fin, _key(zg), KEY_NONE)
    inc = meta[:, 2] != 0
    out = {}
    ki = np.where(inc[None, :], key, KEY_NONE)
    best = np.minimum(ki.min(axis=1), KEY_INF)
    bad = (~fin & inc[None, :]).any(axis=1)
    out["low_z"] = np.where(bad, QNAN, _unkey(best)).astype(np.float32)
    out["low_geom"] = np.where(bad | (best == KEY_INF), -1, ki.argmin(axis=1)).astype(np.int32)  # (argmin: the first of equals)
    out["track_z"] = np.empty((N, S), np.float32)
    for s in range(S):
        cols = meta[:, 3] == s
        ks = np.minimum(np.where(cols[None, :], key, KEY_NONE).min(axis=1), KEY_INF)
        out["track_z"][:, s] = np.where((~fin & cols[None, :]).any(axis=1), QNAN, _unkey(ks))
    out["geom_min"] = _unkey(np.minimum(key.min(axis=0), KEY_INF)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        out["geom_below"] = (fin & (zg < np.float32(z_ref))).sum(axis=0).astype(np.int64)
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------
NS = (1, 2, 63, 64, 65, 130)
GS = (1, 63, 64, 65, 101)
NBODIES = (2, 5, 67)
AXIS_QUATS = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [-1, 0, 0, 0]], np.float32)


def _unit(rng, shape):
    v = rng.normal(0.0, 1.0, shape + (4,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def poses(N, nbody, seed, aligned=False):
    """xpos, xquat of N frames: random unit quaternions, or (``aligned``) the axis-aligned ones, whose rotation rows are exact 0 / +-1"""
    rng = np.random.default_rng(seed)
    xpos = rng.normal(0.0, 0.1, (N, nbody, 3))
    xquat = AXIS_QUATS[rng.integers(0, len(AXIS_QUATS), (N, nbody))] if aligned else _unit(rng, (N, nbody))
    return _f32(xpos), _f32(xquat)


def table(G, nbody, seed, S=2, mesh_counts=(1, 63), share=False, aligned=False, include=None, quantised=False):
    """A random table of G geoms that cycles through the six types; the meshes take their vertex counts from ``mesh_counts`` in turn
    (``share``: all meshes of one count use one range).  ``aligned``: axis-aligned geom frames.  ``quantised``: sizes, positions and
    vertices are multiples of 1 / 64, so that with aligned poses z_g is exact and ties are common.  -> meta, data, verts"""
    rng = np.random.default_rng(seed)
    meta = np.zeros((G, 6), np.int32)
    data = np.zeros((G, 15), np.float64)
    verts, ranges, n_mesh = [], {}, 0
    for g in range(G):
        t = TYPES[(g + seed) % 6]
        meta[g, 0], meta[g, 1] = t, rng.integers(1, nbody)
        meta[g, 2] = rng.integers(0, 2) if include is None else include
        meta[g, 3] = rng.integers(-1, S) if S else -1
        size, pos = rng.uniform(0.01, 0.1, 3), rng.normal(0.0, 0.05, 3)
        if quantised:
            size, pos = np.ceil(size * 64) / 64, np.round(pos * 64) / 64
        data[g, :3], data[g, 3:6] = size, pos
        data[g, 6:] = _rot(AXIS_QUATS[rng.integers(0, 4)].astype(np.float64) if aligned else _unit(rng, ())).reshape(-1)
        if t == MESH:
            cnt = mesh_counts[n_mesh % len(mesh_counts)]
            n_mesh += 1
            if not (share and cnt in ranges):
                v = rng.normal(0.0, 0.05, (cnt, 3))
                ranges[cnt] = (sum(len(a) for a in verts), cnt)
                verts.append(np.round(v * 64) / 64 if quantised else v)
            meta[g, 4:] = ranges[cnt]
    return meta, _f32(data), _f32(np.concatenate(verts) if verts else np.zeros((0, 3)))


def cases(nbody, ns=NS, gs=GS):
    """(label, xpos, xquat, meta, data, verts, S, z_ref) over N x G of one nbody; even seeds are axis-aligned and quantised"""
    out = []
    for N in ns:
        for G in gs:
            seed = 31 * N + 7 * G + nbody
            aligned = seed % 2 == 0
            S = (0, 1, 2, 32)[seed % 4]
            xpos, xquat = poses(N, nbody, seed, aligned)
            if aligned:
                xpos = _f32(np.round(xpos * 64) / 64)
            meta, data, verts = table(G, nbody, seed, S, mesh_counts=(1, 63, 64, 65), share=seed % 3 == 0, aligned=aligned, quantised=aligned)
            out.append((f"N{N}_G{G}_nbody{nbody}_S{S}_{'aligned' if aligned else 'random'}", xpos, xquat, meta, data, verts, S, 0.0))
    return out


def special_cases():
    """Two identical included geoms; nothing included; S in {0, 1, 32} with slots of non-included geoms; meshes of 1, 63, 64, 65 and
    1000 vertices, sharing and not sharing verts; z_ref equal to a z_g exactly"""
    out = []
    xpos, xquat = poses(70, 5, 1)
    meta, data, verts = table(12, 5, 1, S=1, include=1)
    meta[7], data[7] = meta[3], data[3]  # (two identical geoms: the smaller index wins wherever they are the lowest)
    meta[:, 2] = 0
    meta[[3, 7], 2] = 1
    out.append(("twins", xpos, xquat, meta, data, verts, 1, 0.0))
    meta, data, verts = table(9, 5, 2, S=2, include=0)
    meta[:, 3] = np.arange(9) % 3 - 1
    out.append(("nothing_included", xpos, xquat, meta, data, verts, 2, 0.0))
    for S in (0, 1, 32):
        meta, data, verts = table(70, 5, 3 + S, S=S)
        if S:
            meta[::2, 2] = 0  # (slots that hold geoms which are not included)
            meta[:S, 3] = np.arange(S)
        out.append((f"slots{S}", xpos, xquat, meta, data, verts, S, 0.0))
    for share in (False, True):
        meta, data, verts = table(30, 5, 5, S=2, mesh_counts=(1, 63, 64, 65, 1000), share=share)
        meta[:, 0] = MESH
        meta, data, verts = _all_meshes(meta, data, (1, 63, 64, 65, 1000), share)
        out.append((f"meshes_{'shared' if share else 'own'}", xpos, xquat, meta, data, verts, 2, 0.0))
    # z_ref equal to a z_g exactly: an aligned, quantised scene, z_ref the lowest z of frame 0
    xp, xq = poses(66, 5, 8, aligned=True)
    xp = _f32(np.round(xp * 64) / 64)
    meta, data, verts = table(20, 5, 8, S=1, aligned=True, quantised=True, include=1)
    z = judge_z(xp, xq, meta, data, verts)
    out.append(("z_ref_hit", xp, xq, meta, data, verts, 1, float(z[0].min())))
    return out


def _all_meshes(meta, data, counts, share):
    rng = np.random.default_rng(99)
    verts, ranges = [], {}
    for g in range(meta.shape[0]):
        cnt = counts[g % len(counts)]
        if not (share and cnt in ranges):
            ranges[cnt] = (sum(len(a) for a in verts), cnt)
            verts.append(rng.normal(0.0, 0.05, (cnt, 3)))
        meta[g, 4:] = ranges[cnt]
    return meta, data, _f32(np.concatenate(verts))


POISONS = [(v, where, body) for v in (np.nan, np.inf, -np.inf) for where in ("xpos", "xquat") for body in ("included", "tracked", "untouched")]


def poisoned(value, where, body, N=130, rows=(1, 70)):
    """Five bodies: body 1 carries included geoms (slot 0), body 2 geoms that are tracked (slot 1) but not included, body 3 geoms that
    are neither, body 4 no geom.  ``value`` goes into the z of xpos or into the x of the quaternion of one of them (``untouched``: body
    4) in the frames ``rows``"""
    xpos, xquat = poses(N, 5, 77)
    meta, data, verts = table(18, 5, 77, S=2, mesh_counts=(5,))
    meta[:, 1] = 1 + np.arange(18) % 3
    meta[:, 2] = meta[:, 1] == 1
    meta[:, 3] = np.where(meta[:, 1] == 1, 0, np.where(meta[:, 1] == 2, 1, -1))
    b = {"included": 1, "tracked": 2, "untouched": 4}[body]
    for t in rows:
        if where == "xpos":
            xpos[t, b, 2] = value
        else:
            xquat[t, b, 1] = value
    return f"{value}_{where}_{body}", xpos, xquat, meta, data, verts, 2, 0.0


# ---- the reference's stored fit ------------------------------------------------------------------------------------------------------
def reference_fit(reference_dir, demo_viz, scale=0.9):
    """The reference's own stored fit (tests/golden/demo_viz_golden.npz, 50 frames) as xpos / xquat by the oracle's forward kinematics
    over rodent_tables_legacy.npz, with the rodent's scene compiled at ``scale`` -> (scene, tables, xpos, xquat)"""
    from conftest import GOLDEN
    from oracle import Oracle
    from stac_mjx_amd.mjcf import ModelTables, compile_render_scene

    tables = ModelTables.load(GOLDEN / "rodent_tables_legacy.npz")
    orc = Oracle(tables)
    orc.set_site_pos(demo_viz["offsets"])
    fk = [orc.fk(q) for q in demo_viz["qpos"]]
    scene = compile_render_scene(reference_dir / "models" / "rodent.xml", scale=scale, log=lambda *a: None)
    return scene, tables, np.stack([f["xpos"] for f in fk]), np.stack([f["xquat"] for f in fk])
