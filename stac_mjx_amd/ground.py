"""Ground clearance of fitted poses (``stac.ground``; DESIGN.md "Ground clearance"): ``ground_table``, the geoms of a compiled scene
as the table of ``csrc/ground/stac_ground.hpp``; ``ground_clearance`` over ``stac_ground_clearance`` of the companion library
``csrc/ground/libstac_ground.so`` -- per frame the lowest world z of the included geoms and the geom that has it, per track slot the
lowest z of a body's geoms, per geom its lowest z over the frames and the number of frames it spends below a reference height, one
fused pass over ``xpos`` / ``xquat`` on the GPU -- and ``summarize``, what ``<ik file>.ground.json`` holds.

The rule is stated once, in ``csrc/ground/stac_ground.hpp``.  There is no tensor-operation fallback: without the built library the
call raises.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from .abi import StacHipError, _ptr, stream_ptr
from .config import GROUND_MAX_TRACK
from .engine import load_ground_library

MAX_GEOMS = 4096     # csrc/ground/stac_ground.hpp: kGroundMaxGeoms
MAX_BODIES = 4096    # kGroundMaxBodies
MAX_VERTS = 1 << 20  # kGroundMaxVerts
MAX_SLOTS = GROUND_MAX_TRACK  # kGroundMaxSlots (config.py holds the one Python statement of it)
OUTPUTS = ("low_z", "low_geom", "track_z", "geom_min", "geom_below")


def _check(lib, what, rc):
    if rc < 0:
        raise StacHipError(f"{what}: libstac_ground error {rc}: {lib.stac_ground_last_error().decode('utf-8', 'replace')}")
    return rc


@dataclass
class GroundTable:
    """The geom table of a call: ``meta`` [G, 6] int32 (type, body, include, slot, vert_first, vert_count), ``data`` [G, 15] float32
    (size, pos, the rotation matrix row-major), ``verts`` [V, 3] float32, and what the rows are called.  The device copies are made
    on first use, per device."""

    meta: np.ndarray
    data: np.ndarray
    verts: np.ndarray
    nbody: int
    names: list = field(default_factory=list)        # [G] geom names (``geom<i>`` of the scene for a geom without one)
    body_names: list = field(default_factory=list)   # [G] the name of each geom's body
    track: list = field(default_factory=list)        # [S] the body name of each slot
    _device: dict = field(default_factory=dict, repr=False)

    @property
    def n_geoms(self) -> int:
        return int(self.meta.shape[0])

    @property
    def n_slots(self) -> int:
        return len(self.track)

    @property
    def include(self) -> np.ndarray:
        return self.meta[:, 2].astype(bool)

    def on(self, device):
        """(meta, data, verts) as tensors on ``device``"""
        key = str(torch.device(device))
        if key not in self._device:
            verts = self.verts if self.verts.size else np.zeros((1, 3), np.float32)  # (a table without meshes: never read)
            self._device[key] = tuple(torch.as_tensor(np.array(a)).to(device) for a in (self.meta, self.data, verts))
        return self._device[key]


def _rotation(quat) -> np.ndarray:
    """The rotation matrix of a quaternion (w, x, y, z), float64, normalised first."""
    w, x, y, z = np.asarray(quat, np.float64) / np.linalg.norm(np.asarray(quat, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def fitted_bodies(tables) -> np.ndarray:
    """[nbody] bool: the bodies that are ancestor-or-self of a body with a marker site (``site_bodyid``): what the fit can move."""
    parent = np.asarray(tables.body_parentid)
    out = np.zeros(int(tables.nbody), bool)
    for b in np.unique(np.asarray(tables.site_bodyid)):
        b = int(b)
        while b > 0 and not out[b]:
            out[b] = True
            b = int(parent[b])
    return out


def ground_table(scene, tables, geoms="fitted", geom_groups=None, track=()) -> GroundTable:
    """The table of the geoms of ``scene`` (``mjcf.compile_render_scene``) that hang on a body other than the world, planes left out
    (and ``geom_groups``: only those groups; None: all).  ``geoms`` says which of them are INCLUDED in ``low_z``: "fitted" -- those of
    ``fitted_bodies(tables)``; "all"; or a list of geom or body names (a body name stands for its geoms), each checked.  ``track``: up
    to 32 body names, one slot each over the body's geoms, included or not.  ``ValueError`` for an unknown name, a name that selects
    nothing, a table without geoms and more than 32 slots.  -> ``GroundTable`` (``.names``: the geom names in table order)."""
    from .mjcf import GEOM_MESH, GEOM_PLANE, GEOM_SPHERE

    gtype, gbody = np.asarray(scene.geom_type), np.asarray(scene.geom_body)
    keep = (gtype >= GEOM_SPHERE) & (gtype <= GEOM_MESH) & (gbody > 0) & (gtype != GEOM_PLANE)
    if geom_groups is not None:
        keep &= np.isin(np.asarray(scene.geom_group), [int(g) for g in geom_groups])
    rows = np.flatnonzero(keep)
    if rows.size == 0:
        raise ValueError("ground_table: the scene has no geom on a body other than the world" + ("" if geom_groups is None else f" in the groups {list(geom_groups)}"))
    names = [scene.geom_names[i] or f"geom{i}" for i in rows]
    body_names = [str(scene.body_names[gbody[i]]) for i in rows]
    if isinstance(geoms, str):
        if geoms not in ("fitted", "all"):
            raise ValueError(f"ground_table: geoms must be fitted, all or a list of geom or body names, not {geoms!r}")
        include = fitted_bodies(tables)[gbody[rows]] if geoms == "fitted" else np.ones(rows.size, bool)
    else:
        include = np.zeros(rows.size, bool)
        for n in geoms:
            hit = np.array([n == g or n == b for g, b in zip(names, body_names)], bool)
            if not hit.any():
                raise ValueError(f"ground_table: {n!r} is neither a geom nor a body with geoms of this table")
            include |= hit
    track = [str(b) for b in track]
    if len(track) > MAX_SLOTS:
        raise ValueError(f"ground_table: at most {MAX_SLOTS} bodies can be tracked, not {len(track)}")
    slot = np.full(rows.size, -1, np.int32)
    for s, b in enumerate(track):
        hit = np.array([bn == b for bn in body_names], bool)
        if not hit.any():
            raise ValueError(f"ground_table: track names {b!r}, which is not a body with geoms of this table")
        if track.index(b) != s:
            raise ValueError(f"ground_table: track names the body {b!r} twice")
        slot[hit] = s
    meta = np.zeros((rows.size, 6), np.int32)
    data = np.zeros((rows.size, 15), np.float32)
    verts, ranges = [], {}
    for r, i in enumerate(rows):
        meta[r, :4] = (gtype[i], gbody[i], include[r], slot[r])
        data[r, :3], data[r, 3:6] = scene.geom_size[i], scene.geom_pos[i]
        data[r, 6:] = _rotation(scene.geom_quat[i]).reshape(-1)  # (float64, rounded once)
        if gtype[i] == GEOM_MESH:
            mi = int(scene.geom_mesh[i])
            if mi not in ranges:  # (the geoms of one mesh asset share its vertices)
                v = np.unique(np.asarray(scene.meshes[mi].tris, np.float32).reshape(-1, 3), axis=0)
                ranges[mi] = (sum(a.shape[0] for a in verts), v.shape[0])
                verts.append(v)
            meta[r, 4:] = ranges[mi]
    verts = np.ascontiguousarray(np.concatenate(verts) if verts else np.zeros((0, 3)), dtype=np.float32)
    return GroundTable(meta=meta, data=data, verts=verts, nbody=int(scene.nbody), names=names, body_names=body_names, track=track)


def ground_clearance(xpos: torch.Tensor, xquat: torch.Tensor, table: GroundTable, z_ref: float = 0.0) -> dict:
    """Device tensors ``xpos`` [N, nbody, 3] and ``xquat`` [N, nbody, 4] -> ``{low_z [N], low_geom [N] int32, track_z [N, S], geom_min
    [G], geom_below [G] int64}``, device tensors, on the current stream of their device (``stac_ground_clearance``; the header states
    every word).  The inputs are made contiguous float32 first and are never written; no host synchronisation."""
    for name, a, last in (("xpos", xpos, 3), ("xquat", xquat, 4)):
        if not isinstance(a, torch.Tensor) or not a.is_cuda or a.dim() != 3 or a.shape[2] != last:
            raise ValueError(f"ground_clearance: {name} must be a CUDA tensor [frames, nbody, {last}]")
    if xpos.shape[:2] != xquat.shape[:2] or xpos.device != xquat.device:
        raise ValueError(f"ground_clearance: xpos {tuple(xpos.shape)} and xquat {tuple(xquat.shape)} are not of the same frames and bodies")
    p, q = xpos.to(torch.float32).contiguous(), xquat.to(torch.float32).contiguous()
    N, nbody = int(p.shape[0]), int(p.shape[1])
    G, S, V = table.n_geoms, table.n_slots, int(table.verts.shape[0])
    meta, data, verts = table.on(p.device)
    host = np.ascontiguousarray(table.meta, dtype=np.int32)
    lib = load_ground_library()
    mk = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=p.device)  # noqa: E731
    out = {"low_z": mk(N), "low_geom": mk(N, torch.int32), "track_z": mk((N, S)), "geom_min": mk(G), "geom_below": mk(G, torch.int64)}
    with torch.cuda.device(p.device):
        rc = lib.stac_ground_clearance(_ptr(p), _ptr(q), N, nbody, host.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(meta), _ptr(data), G,
                                       _ptr(verts) if V else None, V, S, float(z_ref), _ptr(out["low_z"]), _ptr(out["low_geom"]),
                                       _ptr(out["track_z"]) if S else None, _ptr(out["geom_min"]), _ptr(out["geom_below"]),
                                       stream_ptr(p.device))
    _check(lib, "stac_ground_clearance", rc)
    return out


def kth_rank(permille: int, n: int) -> int:
    """The 1-based rank of the ``permille`` quantile of n values: ceil(permille n / 1000), at least 1 (integer arithmetic)."""
    return max(1, -(-int(permille) * int(n) // 1000))


def floor_level(low_z: torch.Tensor, permille: int):
    """``floor_z``: the order statistic of rank ``kth_rank(permille, n)`` of the n finite values of ``low_z`` (``torch.kthvalue`` on
    its device), as a float32 tensor of one element; None without a finite value."""
    fin = low_z[torch.isfinite(low_z)]
    return torch.kthvalue(fin, kth_rank(permille, fin.numel())).values.reshape(1) if fin.numel() else None


def summarize(res: dict, table: GroundTable, z_ref: float = 0.0, permille: int = 50, contact: float = 0.002) -> dict:
    """The summary of ``ground_clearance``'s device tensors ``res``: ``floor_z`` (``floor_level``); the minimum, ``floor_z``, the median
    (rank ceil(n / 2)) and the maximum of the finite ``low_z``; per geom its name, body, whether it is included, ``min_z`` and
    ``frames_below`` (of ``z_ref``), and in how many frames it is the lowest; ``unfitted_below``, the geoms that are not included
    and lie below ``z_ref`` in more than half of the frames; and per track the fraction of its finite frames with ``track_z -
    floor_z < contact``.  A value that is not finite is written as null (JSON has no NaN)."""
    num = lambda v: None if v is None or not math.isfinite(float(v)) else float(v)  # noqa: E731
    low = res["low_z"]
    N, G = int(low.shape[0]), table.n_geoms
    fin = low[torch.isfinite(low)]
    floor = floor_level(low, permille)
    floor_z = None if floor is None else float(floor)
    stats = {"n_finite": int(fin.numel()), "min": num(fin.min()) if fin.numel() else None, "floor_z": floor_z,
             "median": float(torch.kthvalue(fin, kth_rank(500, fin.numel())).values) if fin.numel() else None,
             "max": num(fin.max()) if fin.numel() else None}
    lowest = torch.bincount(res["low_geom"][res["low_geom"] >= 0].to(torch.int64), minlength=G).cpu().numpy()
    gmin, below, inc = res["geom_min"].cpu().numpy(), res["geom_below"].cpu().numpy(), table.include
    geoms = [{"name": table.names[g], "body": table.body_names[g], "included": bool(inc[g]), "min_z": num(gmin[g]),
              "frames_below": int(below[g]), "frames_lowest": int(lowest[g])} for g in range(G)]
    tracks = []
    for s, body in enumerate(table.track):
        z = res["track_z"][:, s]
        z = z[torch.isfinite(z)]
        near = None if floor is None or not z.numel() else float(((z - floor) < float(contact)).sum()) / int(z.numel())
        tracks.append({"body": body, "n_finite": int(z.numel()), "min_z": num(z.min()) if z.numel() else None, "contact_fraction": near})
    return {"n_frames": N, "n_geoms": G, "n_included": int(inc.sum()), "z_ref": float(z_ref), "permille": int(permille), "contact": float(contact),
            "floor_z": floor_z, "low_z": stats, "geoms": geoms,
            "unfitted_below": [table.names[g] for g in range(G) if not inc[g] and 2 * int(below[g]) > N], "tracks": tracks}
