"""The frame rule of DESIGN.md section 8 "What a frame shows", stated from solid membership in numpy float64 (test
infrastructure only).  It shares no program text with tests/tools/render_ref.c or the kernel: where those solve a quadratic
or walk slabs, this file only asks of a point whether it is inside a solid.

Every solid has a convex level function g(x), negative inside:
    sphere      |x - c| - r
    capsule     (distance from x to the segment) - r
    ellipsoid   |S^-1 R^T (x - c)| - 1
    cylinder    max(rho - r, |z| - hl)          rho, z: the cylindrical coordinates of R^T (x - c)
    box         max_k(|l_k| - s_k)              l = R^T (x - c)
Along a ray, g is convex.  A ray whose origin has g <= 0 does not hit that solid (a camera inside a solid does not see it).
Otherwise golden-section search looks for a point of the ray with g <= 0 between the near and far side of the solid's
bounding sphere; from the ray's last point known to be outside to that point g changes sign once, and bisection finds where:
the entry.  The normal is the gradient of g by central differences; the two one-sided differences disagree where the
surface has an edge within the step, and such a pixel is marked ``edge``: it has no normal to compare.  Planes are linear and
are intersected as such.  The rest (camera, ids, missing keypoints, error segments, the nearest opaque hit, the transparent
layers, lights, checker, quantisation) follows the text line by line.

Inputs are what the C ABI carries (float32 arrays, ``tan_half_fovy`` rounded to float32), widened to float64.  A quaternion is
used as it is given, in the homogeneous form of its matrix: one of norm 1 + e gives (1 + e)^2 times a rotation.

``render`` returns rgb uint8 [N,H,W,3], seg int32 [N,H,W], depth float64 [N,H,W] and edge bool [N,H,W].  A type-7 (mesh)
primitive raises: meshes have their own brute-force check."""

from __future__ import annotations

import numpy as np

PLANE, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX, MESH = 0, 2, 3, 4, 5, 6, 7
TRANSPARENT, CHECKER, TEXUNIFORM = 1, 2, 4
LAYERS = 8
GOLDEN_STEPS = 48  # the bracket shrinks to 0.618^48 = 1e-10 of the bounding sphere's diameter
BISECT_STEPS = 60  # the entry to 2^-60 of it
DIFF_STEP = 1e-5  # finite-difference step of the normal, in units of the solid's smallest size
EDGE_TOL = 1e-3  # one-sided unit normals further apart than this: an edge


def quat_matrix(q):
    """[..., 4] (w, x, y, z), used as given -> [..., 3, 3] whose columns are the rotated frame's axes."""
    q = np.asarray(q, np.float64)
    w, x, y, z = (q[..., k] for k in range(4))
    return np.stack([
        w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
        2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
        2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z,
    ], -1).reshape(q.shape[:-1] + (3, 3))  # fmt: skip


class Prims:
    """The primitives of one frame, id = row.  kind -1: not drawn.  c, R, sz: world centre, axes (columns), sizes; a, b: the
    two ends of a capsule's segment; brad: radius of a sphere about c that holds the solid; step: DIFF_STEP x smallest size."""

    def __init__(self, n):
        self.kind = np.full(n, -1, np.int64)
        self.flags = np.zeros(n, np.int64)
        self.c = np.zeros((n, 3))
        self.R = np.tile(np.eye(3), (n, 1, 1))
        self.sz = np.zeros((n, 3))
        self.a = np.zeros((n, 3))
        self.b = np.zeros((n, 3))
        self.brad = np.zeros(n)
        self.step = np.ones(n)
        self.rgb = np.zeros((n, 3))
        self.rgb2 = np.zeros((n, 3))
        self.tex = np.ones((n, 2))


def frame_prims(t, f, xpos, xquat, kp, markers, show_error) -> Prims:
    P, K = len(t["prim_type"]), len(t["kp_rgba"])
    p = Prims(P + 3 * K)
    ty = np.asarray(t["prim_type"], np.int64)
    if (ty == MESH).any():
        raise ValueError("render_rule does not draw mesh primitives")
    body = np.asarray(t["prim_body"], np.int64)
    Rb = quat_matrix(xquat[f])[body]
    p.kind[:P] = ty
    p.flags[:P] = np.asarray(t["prim_flags"], np.int64)
    p.R[:P] = Rb @ quat_matrix(t["prim_quat"])
    p.c[:P] = np.asarray(xpos[f], np.float64)[body] + np.einsum("pij,pj->pi", Rb, np.asarray(t["prim_pos"], np.float64))
    p.sz[:P] = np.asarray(t["prim_size"], np.float64)
    p.rgb[:P] = np.asarray(t["prim_rgba"], np.float64)[:, :3]
    p.rgb2[:P] = np.asarray(t["prim_rgb2"], np.float64)
    p.tex[:P] = np.asarray(t["prim_texrepeat"], np.float64)
    axis = p.R[:P, :, 2]
    p.a[:P] = p.c[:P] - axis * p.sz[:P, 1:2]
    p.b[:P] = p.c[:P] + axis * p.sz[:P, 1:2]
    kpf = np.asarray(kp[f], np.float64).reshape(K, 3) if kp is not None else np.full((K, 3), np.nan)
    mkf = np.asarray(markers[f], np.float64).reshape(K, 3) if markers is not None else np.full((K, 3), np.nan)
    mr, sr = float(t["marker_radius"]), float(t["segment_radius"])
    for k in range(K):
        has_kp, has_mk = np.isfinite(kpf[k]).all(), np.isfinite(mkf[k]).all()
        if has_kp:
            i = P + k
            p.kind[i], p.c[i], p.sz[i, 0], p.rgb[i] = SPHERE, kpf[k], mr, np.asarray(t["kp_rgba"], np.float64)[k, :3]
        if has_mk:
            i = P + K + k
            p.kind[i], p.c[i], p.sz[i, 0], p.rgb[i] = SPHERE, mkf[k], mr, np.asarray(t["marker_rgba"], np.float64)[:3]
        if show_error and has_kp and has_mk:
            i = P + 2 * K + k
            p.kind[i], p.a[i], p.b[i], p.c[i] = CAPSULE, kpf[k], mkf[k], 0.5 * (kpf[k] + mkf[k])
            p.sz[i, 0], p.sz[i, 1] = sr, 0.5 * np.linalg.norm(mkf[k] - kpf[k])
            p.rgb[i] = np.asarray(t["segment_rgba"], np.float64)[:3]
    s = p.sz
    k = p.kind
    p.brad = np.select([k == SPHERE, k == CAPSULE, k == ELLIPSOID, (k == CYLINDER) | (k == PLANE), k == BOX],
                       [s[:, 0], s[:, 0] + s[:, 1], s.max(1), np.hypot(s[:, 0], s[:, 1]), np.linalg.norm(s, axis=1)], 0.0)
    p.step = DIFF_STEP * np.select([(k == SPHERE) | (k == CAPSULE), k == CYLINDER], [s[:, 0], s[:, :2].min(1)], s.min(1))
    return p


def level(kind, p: Prims, idx, x):
    """g of the solids ``idx`` (all of one kind) at the points x [M, 3]."""
    if kind == SPHERE:
        return np.linalg.norm(x - p.c[idx], axis=1) - p.sz[idx, 0]
    if kind == CAPSULE:
        a = p.a[idx]
        ab = p.b[idx] - a
        l2 = (ab * ab).sum(1)
        s = np.clip(((x - a) * ab).sum(1) / np.where(l2 > 0, l2, 1.0), 0.0, 1.0)
        return np.linalg.norm(x - a - s[:, None] * ab, axis=1) - p.sz[idx, 0]
    l = np.einsum("mji,mj->mi", p.R[idx], x - p.c[idx])  # R^T (x - c)
    sz = p.sz[idx]
    if kind == ELLIPSOID:
        return np.linalg.norm(l / sz, axis=1) - 1.0
    if kind == CYLINDER:
        return np.maximum(np.hypot(l[:, 0], l[:, 1]) - sz[:, 0], np.abs(l[:, 2]) - sz[:, 1])
    if kind == BOX:
        return (np.abs(l) - sz).max(1)
    raise ValueError(kind)


def solid_entries(kind, p: Prims, ids, o, d, T):
    """Entry distances of the rays o + t d [Npix, 3] into the solids ``ids`` of one kind, written into T[:, ids]."""
    ids = ids[level(kind, p, ids, np.broadcast_to(o, (len(ids), 3))) > 0]  # the inside rule
    if not len(ids):
        return
    w = p.c[ids] - o
    br = p.brad[ids] * 1.01 + 1e-9
    tc = d @ w.T  # [Npix, n] closest approach to the centre
    miss2 = (w * w).sum(1)[None] - tc * tc
    pix, k = np.nonzero((miss2 <= (br * br)[None]) & (tc >= -br[None]))  # bounding-sphere prefilter
    if not len(pix):
        return
    idx, tc, br = ids[k], tc[pix, k], br[k]
    lo, hi = np.maximum(tc - br, 0.0), tc + br  # g(lo) > 0: the origin, or a point outside the bounding sphere
    g = lambda sel, tt: level(kind, p, idx[sel], o + tt[:, None] * d[pix[sel]])
    # golden-section search for a point with g <= 0; a pair leaves the search as soon as it has one
    inv = (np.sqrt(5.0) - 1.0) / 2.0
    tin = np.full(len(pix), np.inf)
    act = np.arange(len(pix))
    a, b = lo.copy(), hi.copy()
    x1, x2 = b - inv * (b - a), a + inv * (b - a)
    f1, f2 = g(act, x1), g(act, x2)
    for _ in range(GOLDEN_STEPS):
        found = np.minimum(f1, f2) <= 0
        tin[act[found]] = np.where(f1 <= 0, x1, x2)[found]
        keep = ~found
        act, a, b, x1, x2, f1, f2 = act[keep], a[keep], b[keep], x1[keep], x2[keep], f1[keep], f2[keep]
        if not len(act):
            break
        left = f1 <= f2  # the minimum is in [a, x2], else in [x1, b]
        a, b = np.where(left, a, x1), np.where(left, x2, b)
        xn = np.where(left, b - inv * (b - a), a + inv * (b - a))
        fn = g(act, xn)
        x1, f1, x2, f2 = np.where(left, xn, x2), np.where(left, fn, f2), np.where(left, x1, xn), np.where(left, f1, fn)
    if len(act):
        found = np.minimum(f1, f2) <= 0
        tin[act[found]] = np.where(f1 <= 0, x1, x2)[found]
    hit = np.flatnonzero(np.isfinite(tin))
    if not len(hit):
        return
    a, b = lo[hit], tin[hit]  # g(a) > 0 >= g(b), one sign change between them
    for _ in range(BISECT_STEPS):
        m = 0.5 * (a + b)
        inside = g(hit, m) <= 0
        a, b = np.where(inside, a, m), np.where(inside, m, b)
    T[pix[hit], idx[hit]] = b


def plane_entries(p: Prims, ids, o, d, T):
    """One-sided finite planes: the ray comes from the +z side and meets l_z = 0 within the half extents."""
    for i in ids:
        R, c, sz = p.R[i], p.c[i], p.sz[i]
        ol, dl = R.T @ (o - c), d @ R
        if not ol[2] > 0:
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(dl[:, 2] < 0, -ol[2] / dl[:, 2], np.inf)
            x, y = ol[0] + dl[:, 0] * t, ol[1] + dl[:, 1] * t
            ok = np.isfinite(t) & (t > 0) & (np.abs(x) <= sz[0]) & (np.abs(y) <= sz[1])
        T[ok, i] = t[ok]


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def shade(t, p: Prims, ids, x, zc):
    """Colour [M, 3] and edge [M] of the hits at the points x of the primitives ids; zc: the camera's z axis."""
    n = np.zeros((len(ids), 3))
    edge = np.zeros(len(ids), bool)
    kinds = p.kind[ids]
    for kind in np.unique(kinds):
        m = np.flatnonzero(kinds == kind)
        if kind == PLANE:
            n[m] = _unit(p.R[ids[m]][:, :, 2])
            continue
        h = p.step[ids[m]]
        g0 = level(kind, p, ids[m], x[m])
        fwd, bwd = np.zeros((len(m), 3)), np.zeros((len(m), 3))
        for k in range(3):
            e = np.zeros(3)
            e[k] = 1.0
            fwd[:, k] = (level(kind, p, ids[m], x[m] + h[:, None] * e) - g0) / h
            bwd[:, k] = (g0 - level(kind, p, ids[m], x[m] - h[:, None] * e)) / h
        n[m] = _unit(fwd + bwd)
        edge[m] = np.linalg.norm(_unit(fwd) - _unit(bwd), axis=1) > EDGE_TOL
    rgb = p.rgb[ids].copy()
    ck = np.flatnonzero((p.flags[ids] & CHECKER) != 0)
    if len(ck):
        i = ids[ck]
        l = np.einsum("mji,mj->mi", p.R[i], x[ck] - p.c[i])
        uni = ((p.flags[i] & TEXUNIFORM) != 0)[:, None]
        uv = l[:, :2] * p.tex[i] / np.where(uni, 1.0, 2.0 * p.sz[i, :2])
        cell = np.floor(2.0 * uv[:, 0]) + np.floor(2.0 * uv[:, 1])
        odd = np.mod(cell, 2.0) == 1.0
        rgb[ck[odd]] = p.rgb2[i[odd]]
    L = np.asarray(t["head_ambient"], np.float64)[None] + np.asarray(t["head_diffuse"], np.float64)[None] * np.maximum(n @ zc, 0.0)[:, None]
    for ldir, ldiff in zip(np.asarray(t["light_dir"], np.float64).reshape(-1, 3), np.asarray(t["light_diffuse"], np.float64).reshape(-1, 3)):
        L = L + ldiff[None] * np.maximum(-(n @ ldir), 0.0)[:, None]
    return rgb * np.minimum(L, 1.0), edge


def entries(p: Prims, o, d):
    """T [Npix, Ptot]: the entry distance of every ray into every primitive, +inf where it does not hit."""
    T = np.full((len(d), len(p.kind)), np.inf)
    for kind in (SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX):
        ids = np.flatnonzero(p.kind == kind)
        if len(ids):
            solid_entries(kind, p, ids, o, d, T)
    plane_entries(p, np.flatnonzero(p.kind == PLANE), o, d, T)
    return T


def pixel_rays(cam_f, tan_half_fovy, W, H):
    """Origin [3], unit directions [H * W, 3] (row 0 at the top) and rotation of one camera cam_f[12]."""
    cam_f = np.asarray(cam_f, np.float32).astype(np.float64)
    tv = float(np.float32(tan_half_fovy))
    tu = tv * (W / H)
    u = ((np.arange(W) + 0.5) * 2.0 / W - 1.0) * tu
    v = (1.0 - (np.arange(H) + 0.5) * 2.0 / H) * tv
    uu, vv = (a.reshape(-1) for a in np.meshgrid(u, v))
    Rc = cam_f[3:].reshape(3, 3)
    return cam_f[:3], _unit(uu[:, None] * Rc[:, 0] + vv[:, None] * Rc[:, 1] - Rc[:, 2]), Rc


def hit_table(t, nbody, xpos, xquat, kp, markers, show_error, cam, tan_half_fovy, W, H, frame=0):
    """[H, W, P + 3K]: the entry distance of every pixel's ray into every primitive of one frame (+inf: no hit)."""
    cam = np.asarray(cam, np.float32).reshape(-1, 12)
    N = len(cam)
    xpos, xquat = np.asarray(xpos, np.float32).reshape(N, nbody, 3), np.asarray(xquat, np.float32).reshape(N, nbody, 4)
    o, d, _ = pixel_rays(cam[frame], tan_half_fovy, W, H)
    return entries(frame_prims(t, frame, xpos, xquat, kp, markers, show_error), o, d).reshape(H, W, -1)


def render(t, nbody, xpos, xquat, kp, markers, show_error, cam, tan_half_fovy, W, H):
    cam = np.asarray(cam, np.float32).reshape(-1, 12)
    N = len(cam)
    xpos = np.asarray(xpos, np.float32).reshape(N, nbody, 3)
    xquat = np.asarray(xquat, np.float32).reshape(N, nbody, 4)
    alpha = float(np.float32(t["alpha"]))
    rgb = np.zeros((N, H, W, 3), np.uint8)
    seg = np.full((N, H, W), -1, np.int32)
    depth = np.full((N, H, W), np.inf)
    edge = np.zeros((N, H, W), bool)
    for f in range(N):
        o, d, Rc = pixel_rays(cam[f], tan_half_fovy, W, H)
        p = frame_prims(t, f, xpos, xquat, kp, markers, show_error)
        T = entries(p, o, d)
        drawn = p.kind >= 0
        opaque = np.flatnonzero(drawn & ((p.flags & TRANSPARENT) == 0))
        clear = np.flatnonzero(drawn & ((p.flags & TRANSPARENT) != 0))
        npix = len(d)
        to, io = np.full(npix, np.inf), np.full(npix, -1)
        if len(opaque):
            j = T[:, opaque].argmin(1)  # the first of equal minima: the lower id
            to = T[np.arange(npix), opaque[j]]
            io = np.where(np.isfinite(to), opaque[j], -1)
        col = np.tile(np.asarray(t["background"], np.float64), (npix, 1))
        e = np.zeros(npix, bool)
        hit = np.flatnonzero(io >= 0)
        if len(hit):
            col[hit], e[hit] = shade(t, p, io[hit], o + to[hit, None] * d[hit], Rc[:, 2])
        if len(clear):
            Tc = T[:, clear]
            order = np.argsort(Tc, axis=1, kind="stable")[:, :LAYERS]  # by (t, id)
            tt = np.take_along_axis(Tc, order, 1)
            for k in range(order.shape[1] - 1, -1, -1):  # back to front
                m = np.flatnonzero(tt[:, k] < to)
                if len(m):
                    s, ek = shade(t, p, clear[order[m, k]], o + tt[m, k, None] * d[m], Rc[:, 2])
                    col[m] = col[m] * (1.0 - alpha) + s * alpha
                    e[m] |= ek
        rgb[f] = np.floor(np.clip(col, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8).reshape(H, W, 3)
        seg[f], depth[f], edge[f] = io.reshape(H, W), to.reshape(H, W), e.reshape(H, W)
    return rgb, seg, depth, edge
