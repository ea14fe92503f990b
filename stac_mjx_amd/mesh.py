"""Triangle-mesh assets of the renderer: loaders (numpy only), the bounding-volume hierarchy and mass properties.

A mesh geom is one more primitive of the ray caster (DESIGN.md "Rendering").  This module reads ``.stl`` (binary and
ASCII) and ``.obj`` files into float32 triangle soups, places them in the geom frame, and builds the hierarchy the kernel
walks: nodes in depth-first order with a skip link, so that the walk needs no stack (csrc/stac_render.hip).
"""

from __future__ import annotations

import struct
from dataclasses import dataclass
from pathlib import Path

import numpy as np

LEAF_TRIS = 4  # triangles per leaf (at most)
MAX_TRIS = 1 << 20  # include/stac_hip.h: STAC_RENDER_MAX_MESH_TRIS (the triangle index travels in the pixel's hit key)
SUFFIXES = (".stl", ".obj")


class MeshError(ValueError):
    """A mesh file that cannot be read: the geom is skipped (``n_skipped``), the scene still compiles."""


# ---- loaders: [T, 3, 3] float32 triangle vertices exactly as the file has them ---------------------------------------------
def _stl_binary(data: bytes) -> np.ndarray | None:
    if len(data) < 84:
        return None
    (n,) = struct.unpack_from("<I", data, 80)
    if len(data) != 84 + 50 * n:
        return None
    rec = np.frombuffer(data, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]), count=n, offset=84)
    return np.ascontiguousarray(rec["v"], dtype=np.float32)


def _stl_ascii(text: str) -> np.ndarray:
    verts = []
    tok = text.split()
    if not tok or tok[0].lower() != "solid":
        raise MeshError("not an STL file (neither a binary header with a matching size nor 'solid')")
    i, closed = 0, False
    while i < len(tok):
        w = tok[i].lower()
        if w == "vertex":
            try:
                verts.append([float(tok[i + 1]), float(tok[i + 2]), float(tok[i + 3])])
            except (IndexError, ValueError) as exc:
                raise MeshError("ASCII STL: a vertex line without three numbers") from exc
            i += 4
            continue
        if w == "endsolid":
            closed = True
        i += 1
    if not closed:
        raise MeshError("ASCII STL: truncated (no 'endsolid')")
    if len(verts) % 3:
        raise MeshError(f"ASCII STL: {len(verts)} vertices are not a whole number of triangles")
    return np.asarray(verts, np.float32).reshape(-1, 3, 3)


def load_stl(path) -> np.ndarray:
    """Binary STL when the 80-byte header's count matches the file size, else ASCII."""
    data = Path(path).read_bytes()
    tri = _stl_binary(data)
    if tri is not None:
        return tri
    try:
        text = data.decode("ascii")
    except UnicodeDecodeError as exc:
        raise MeshError("binary STL whose size does not match its triangle count (truncated?)") from exc
    return _stl_ascii(text)


def load_obj(path) -> np.ndarray:
    """``v`` and ``f`` lines only; ``i``, ``i/j``, ``i/j/k``, ``i//k``; negative indices count back from the vertices read
    so far; polygons are fan-triangulated."""
    verts: list = []
    faces: list = []
    with open(path, "r", errors="replace") as fh:
        for ln, line in enumerate(fh, 1):
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                try:
                    verts.append((float(p[1]), float(p[2]), float(p[3])))
                except (IndexError, ValueError) as exc:
                    raise MeshError(f"OBJ line {ln}: a vertex without three numbers") from exc
            elif p[0] == "f":
                idx = []
                for w in p[1:]:
                    try:
                        k = int(w.split("/")[0])
                    except ValueError as exc:
                        raise MeshError(f"OBJ line {ln}: bad face index {w!r}") from exc
                    k = k - 1 if k > 0 else len(verts) + k
                    if k < 0 or k >= len(verts) or w.split("/")[0] in ("0", "-0"):
                        raise MeshError(f"OBJ line {ln}: face index {w!r} outside the {len(verts)} vertices read so far")
                    idx.append(k)
                if len(idx) < 3:
                    raise MeshError(f"OBJ line {ln}: a face with {len(idx)} vertices")
                for j in range(1, len(idx) - 1):
                    faces.append((idx[0], idx[j], idx[j + 1]))
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.ascontiguousarray(v[f], dtype=np.float32)


def load_mesh(path) -> np.ndarray:
    """[T, 3, 3] float32.  Raises :class:`MeshError` for another suffix, an unreadable or empty file, non-finite
    vertices, or more than MAX_TRIS triangles."""
    path = Path(path)
    suf = path.suffix.lower()
    if suf not in SUFFIXES:
        raise MeshError(f"{path.name}: mesh files of type {suf or '(none)'!r} are not read (only .stl and .obj)")
    try:
        tri = load_stl(path) if suf == ".stl" else load_obj(path)
    except OSError as exc:
        raise MeshError(f"{path.name}: {exc.strerror or exc}") from exc
    except MeshError as exc:
        raise MeshError(f"{path.name}: {exc}") from exc
    if tri.shape[0] == 0:
        raise MeshError(f"{path.name}: no triangles")
    if tri.shape[0] > MAX_TRIS:
        raise MeshError(f"{path.name}: {tri.shape[0]} triangles, more than the {MAX_TRIS} a mesh may have")
    if not np.isfinite(tri).all():
        raise MeshError(f"{path.name}: non-finite vertices")
    return tri


# ---- placement and mass ------------------------------------------------------------------------------------------------
def _quat_mat(q) -> np.ndarray:
    w, x, y, z = (float(c) for c in q)
    return np.array([
        [w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
        [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
        [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z],
    ])  # fmt: skip


def place(tri, scale=(1.0, 1.0, 1.0), refpos=(0.0, 0.0, 0.0), refquat=(1.0, 0.0, 0.0, 0.0)) -> np.ndarray:
    """Vertices in the geom frame: ``scale * rotate(conj(refquat), v - refpos)`` (float64 arithmetic, float32 result)."""
    q = np.asarray(refquat, np.float64)
    q = q / np.linalg.norm(q)
    R = _quat_mat(q)  # rotate(conj(q), x) = R^T x; for row vectors x: x @ R
    v = (np.asarray(tri, np.float64) - np.asarray(refpos, np.float64)) @ R
    return np.ascontiguousarray(v * np.asarray(scale, np.float64), dtype=np.float32)


def volume_centroid(tri) -> tuple[float, np.ndarray]:
    """|signed-tetrahedron volume| of a closed mesh and its volume centroid (the vertex mean when the volume is 0)."""
    t = np.asarray(tri, np.float64)
    six = np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2]))
    vol = six.sum() / 6.0
    if abs(vol) < 1e-300:
        return 0.0, t.reshape(-1, 3).mean(0)
    cen = (six[:, None] * (t[:, 0] + t[:, 1] + t[:, 2])).sum(0) / (24.0 * vol)
    return abs(float(vol)), cen


# ---- hierarchy -----------------------------------------------------------------------------------------------------------
@dataclass
class Mesh:
    """One mesh asset as the kernel gets it.  ``tris`` are in the hierarchy's order (Morton order of the centroids)."""

    name: str
    tris: np.ndarray  # [T,3,3] float32, geom frame
    node_box: np.ndarray  # [NN,6] float32: lo[3], hi[3]
    node_link: np.ndarray  # [NN,3] int32: skip, first triangle, triangle count (0 = inner node)
    volume: float = 0.0
    centroid: np.ndarray | None = None

    @property
    def n_tris(self) -> int:
        return int(self.tris.shape[0])


def _spread3(v: np.ndarray) -> np.ndarray:
    """10 bits -> every third bit of 30."""
    v = v.astype(np.uint64) & 0x3FF
    v = (v | (v << 16)) & 0x30000FF
    v = (v | (v << 8)) & 0x300F00F
    v = (v | (v << 4)) & 0x30C30C3
    v = (v | (v << 2)) & 0x9249249
    return v


def morton_order(tri: np.ndarray) -> np.ndarray:
    """Permutation that sorts the triangles by the 30-bit Morton code of their centroid (stable: ties keep file order)."""
    c = np.asarray(tri, np.float64).mean(1)
    lo, hi = c.min(0), c.max(0)
    ext = np.where(hi > lo, hi - lo, 1.0)
    g = np.clip(((c - lo) / ext * 1024.0).astype(np.int64), 0, 1023)
    code = (_spread3(g[:, 0]) << 2) | (_spread3(g[:, 1]) << 1) | _spread3(g[:, 2])
    return np.argsort(code, kind="stable")


def build_bvh(tri: np.ndarray, leaf_tris: int = LEAF_TRIS) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(tris_sorted, node_box, node_link)``: a balanced binary tree over halves of the Morton-sorted triangles, leaves of
    at most ``leaf_tris``, nodes in depth-first order.  ``node_link[n] = (skip, first, count)``: ``skip`` is the node to go
    to when the ray misses node ``n`` or is done with it as a leaf (``n + 1`` for a leaf, the end of the subtree otherwise;
    the number of nodes = stop), ``count`` = 0 for an inner node.  Boxes are the exact float32 bounds of the triangles
    below; the kernel pads them per ray.  Deterministic."""
    tri = np.ascontiguousarray(tri, dtype=np.float32)
    T = tri.shape[0]
    if T == 0:
        raise MeshError("a mesh without triangles")
    tri = tri[morton_order(tri)]
    # level by level: ranges [lo, hi) of the sorted triangles; a range longer than leaf_tris splits at its middle
    levels = [(np.array([0], np.int64), np.array([T], np.int64))]
    while True:
        lo, hi = levels[-1]
        split = (hi - lo) > leaf_tris
        if not split.any():
            break
        mid = (lo[split] + hi[split] + 1) // 2
        levels.append((np.stack([lo[split], mid], 1).reshape(-1), np.stack([mid, hi[split]], 1).reshape(-1)))
    # subtree sizes bottom-up, depth-first indices top-down
    size = [np.ones(len(l[0]), np.int64) for l in levels]
    for d in range(len(levels) - 2, -1, -1):
        split = (levels[d][1] - levels[d][0]) > leaf_tris
        size[d][split] += size[d + 1].reshape(-1, 2).sum(1)
    index = [np.zeros(1, np.int64)]
    for d in range(len(levels) - 1):
        split = (levels[d][1] - levels[d][0]) > leaf_tris
        left = index[d][split] + 1
        right = left + size[d + 1].reshape(-1, 2)[:, 0]
        index.append(np.stack([left, right], 1).reshape(-1))
    NN = int(size[0][0])
    box = np.zeros((NN, 6), np.float32)
    link = np.zeros((NN, 3), np.int32)
    tlo, thi = tri.min(1), tri.max(1)  # [T,3]
    below = None  # boxes of the level below, (lo, hi)
    for d in range(len(levels) - 1, -1, -1):
        lo, hi = levels[d]
        split = (hi - lo) > leaf_tris
        blo = np.empty((len(lo), 3), np.float32)
        bhi = np.empty((len(lo), 3), np.float32)
        leaf = ~split
        if leaf.any():
            # ranges are short: reduce by padding to leaf_tris columns
            k = lo[leaf, None] + np.arange(leaf_tris)[None]
            k = np.minimum(k, hi[leaf, None] - 1)
            blo[leaf], bhi[leaf] = tlo[k].min(1), thi[k].max(1)
        if split.any():
            clo, chi = below
            blo[split], bhi[split] = clo.reshape(-1, 2, 3).min(1), chi.reshape(-1, 2, 3).max(1)
        n = index[d]
        box[n, :3], box[n, 3:] = blo, bhi
        link[n, 0] = n + size[d]
        link[n[leaf], 1] = lo[leaf]
        link[n[leaf], 2] = (hi - lo)[leaf]
        below = (blo, bhi)
    return tri, box, link


def make_mesh(name: str, tri: np.ndarray) -> Mesh:
    """Hierarchy and mass properties of triangles already placed in the geom frame."""
    vol, cen = volume_centroid(tri)
    tris, box, link = build_bvh(tri)
    return Mesh(name=name, tris=tris, node_box=box, node_link=link, volume=vol, centroid=cen)


def pack_meshes(meshes) -> dict:
    """The concatenated arrays of ``stac_render_meshes`` (without ``prim_mesh``)."""
    node_off = np.zeros(len(meshes) + 1, np.int32)
    tri_off = np.zeros(len(meshes) + 1, np.int32)
    for i, m in enumerate(meshes):
        node_off[i + 1] = node_off[i] + len(m.node_box)
        tri_off[i + 1] = tri_off[i] + m.n_tris
    cat = lambda parts, shape, dt: (np.ascontiguousarray(np.concatenate(parts), dtype=dt) if parts else np.zeros(shape, dt))
    return dict(
        node_offset=node_off, tri_offset=tri_off,
        node_box=cat([m.node_box for m in meshes], (0, 6), np.float32),
        node_link=cat([m.node_link for m in meshes], (0, 3), np.int32),
        tri_vertex=cat([m.tris for m in meshes], (0, 3, 3), np.float32),
    )  # fmt: skip
