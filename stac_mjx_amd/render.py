"""GPU renderer of fitted poses: ``Renderer`` (FK + cameras + the ``stac_render`` kernel) behind ``Stac.render``.

What a frame shows is the rule of DESIGN.md "Rendering" (modelled on ``stac_mjx/stac.py:505-658``): model geoms of groups 0
and 2 (primitives and triangle meshes), model sites of groups 0-2, one sphere per keypoint and per fitted marker, and optionally a red segment from each
keypoint to its marker; Lambert shading from the headlight and the model's lights; model geoms of moving bodies drawn
see-through with opacity ``<visual><map alpha>``.  The pixels come from ``stac_render`` (csrc/stac_render.hip); this module
only prepares its inputs on the device.
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from .abi import StacRenderMeshes, StacRenderTables, _f32p, _i32p, _ptr, hip_error
from .engine import Engine
from .mjcf import RenderScene

MAX_PRIMS = 512  # include/stac_hip.h: STAC_RENDER_MAX_PRIMS
LAYERS = 8  # STAC_RENDER_LAYERS
FLAG_TRANSPARENT, FLAG_CHECKER, FLAG_TEXUNIFORM = 1, 2, 4
BACKGROUND = (0.0, 0.0, 0.0)  # colour of a pixel whose ray hits nothing
SEGMENT_RADIUS = 0.001  # the reference's tendon width (stac.py:555)
MARKER_RGBA = (0.0, 0.0, 0.0, 1.0)
SEGMENT_RGBA = (1.0, 0.0, 0.0, 1.0)
GEOM_GROUPS = (0, 2)  # stac.py:619-625: geomgroup 1 off, 2 on (0 on by default)
SITE_GROUPS = (0, 1, 2)  # sitegroup 0-2 on, 3 off
FREE_CAMERA_DISTANCE = 2.0  # free camera: distance = FREE_CAMERA_DISTANCE * spread / tan(fovy / 2)


def render_tables(scene: RenderScene, kp_rgba, marker_size: float, geom_groups=None) -> dict:
    """Host arrays of ``stac_render_tables`` (float32 / int32) and the static primitives' names: the geoms of ``geom_groups``
    (None: GEOM_GROUPS), mesh geoms among them, then the sites of SITE_GROUPS, in document order.  With mesh geoms the dict
    has a ``meshes`` entry: the arrays of ``stac_render_meshes`` (only the meshes that a drawn geom uses)."""
    g = np.flatnonzero(np.isin(scene.geom_group, GEOM_GROUPS if geom_groups is None else tuple(int(v) for v in geom_groups)))
    s = np.flatnonzero(np.isin(scene.site_group, SITE_GROUPS))
    f32 = lambda a, shape: np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape), dtype=np.float32)
    P = len(g) + len(s)
    flags = np.zeros(P, np.int32)
    moving = scene.geom_body[g] != 0
    flags[: len(g)] |= np.where(moving, FLAG_TRANSPARENT, 0).astype(np.int32)
    flags[: len(g)] |= np.where(scene.geom_checker[g], FLAG_CHECKER, 0).astype(np.int32)
    flags[: len(g)] |= np.where(scene.geom_texuniform[g] & scene.geom_checker[g], FLAG_TEXUNIFORM, 0).astype(np.int32)
    kp_rgba = f32(kp_rgba, (-1, 4))
    head_on = 1.0 if scene.head_active else 0.0
    meshes = None
    gm = scene.geom_mesh[g] if scene.geom_mesh is not None else np.full(len(g), -1, np.int32)
    if (gm >= 0).any():
        from .mesh import pack_meshes

        used = sorted(set(int(m) for m in gm if m >= 0))
        remap = {m: k for k, m in enumerate(used)}
        meshes = pack_meshes([scene.meshes[m] for m in used])
        meshes["prim_mesh"] = np.asarray([remap.get(int(m), -1) for m in gm] + [-1] * len(s), np.int32)
    out = dict(
        prim_type=np.ascontiguousarray(np.concatenate([scene.geom_type[g], scene.site_type[s]]), dtype=np.int32),
        prim_body=np.ascontiguousarray(np.concatenate([scene.geom_body[g], scene.site_body[s]]), dtype=np.int32),
        prim_flags=flags,
        prim_size=f32(np.concatenate([scene.geom_size[g], scene.site_size[s]]), (P, 3)),
        prim_pos=f32(np.concatenate([scene.geom_pos[g], scene.site_pos[s]]), (P, 3)),
        prim_quat=f32(np.concatenate([scene.geom_quat[g], scene.site_quat[s]]), (P, 4)),
        prim_rgba=f32(np.concatenate([scene.geom_rgba[g], scene.site_rgba[s]]), (P, 4)),
        prim_rgb2=f32(np.concatenate([scene.geom_rgb2[g], np.zeros((len(s), 3))]), (P, 3)),
        prim_texrepeat=f32(np.concatenate([scene.geom_texrepeat[g], np.ones((len(s), 2))]), (P, 2)),
        kp_rgba=kp_rgba,
        marker_rgba=f32(MARKER_RGBA, 4), segment_rgba=f32(SEGMENT_RGBA, 4),
        marker_radius=np.float32(marker_size), segment_radius=np.float32(SEGMENT_RADIUS),
        light_dir=f32(scene.light_dir, (-1, 3)), light_diffuse=f32(scene.light_diffuse, (-1, 3)),
        head_ambient=f32(scene.head_ambient * head_on, 3), head_diffuse=f32(scene.head_diffuse * head_on, 3),
        alpha=np.float32(scene.alpha), background=f32(BACKGROUND, 3),
        names=[scene.geom_names[i] for i in g] + [scene.site_names[i] for i in s],
    )
    if meshes is not None:
        out["meshes"] = meshes
    return out


def _ctables(t: dict):
    ct = StacRenderTables()
    ct.nprim = len(t["prim_type"])
    for k in ("prim_type", "prim_body", "prim_flags"):
        setattr(ct, k, t[k].ctypes.data_as(_i32p))
    for k in ("prim_size", "prim_pos", "prim_quat", "prim_rgba", "prim_rgb2", "prim_texrepeat", "kp_rgba", "light_dir", "light_diffuse"):
        setattr(ct, k, t[k].ctypes.data_as(_f32p))
    ct.nkp = len(t["kp_rgba"])
    ct.nlight = len(t["light_dir"])
    for k in ("marker_rgba", "segment_rgba", "head_ambient", "head_diffuse", "background"):
        getattr(ct, k)[:] = [float(v) for v in t[k]]
    ct.marker_radius, ct.segment_radius, ct.alpha = float(t["marker_radius"]), float(t["segment_radius"]), float(t["alpha"])
    return ct


def _cmeshes(m: dict):
    cm = StacRenderMeshes()
    cm.nmesh = len(m["node_offset"]) - 1
    for k in ("node_offset", "tri_offset", "node_link", "prim_mesh"):
        m[k] = np.ascontiguousarray(m[k], dtype=np.int32)
        setattr(cm, k, m[k].ctypes.data_as(_i32p))
    for k in ("node_box", "tri_vertex"):
        m[k] = np.ascontiguousarray(m[k], dtype=np.float32)
        setattr(cm, k, m[k].ctypes.data_as(_f32p))
    return cm


class RenderSceneHandle:
    """A ``stac_render_scene`` on the engine's device (uploaded once; no host upload per call)."""

    def __init__(self, engine: Engine, tables: dict):
        self.engine, self.lib = engine, engine.lib
        self.tables = tables
        self.P, self.K = len(tables["prim_type"]), len(tables["kp_rgba"])
        if tables.get("meshes") is not None:  # triangles and hierarchies go to device memory once, here
            self._h = self.lib.stac_render_scene_create_with_meshes(C.c_void_p(engine._h), C.byref(_ctables(tables)),
                                                                    C.byref(_cmeshes(tables["meshes"])))
        else:
            self._h = self.lib.stac_render_scene_create(C.c_void_p(engine._h), C.byref(_ctables(tables)))
        if not self._h:
            self.code = int(self.lib.stac_last_error_code())
            raise hip_error(self.lib, "stac_render_scene_create failed", self.code)

    def render(self, xpos, xquat, kp, markers, show_error, cam, tan_half_fovy, width, height, rgb=None, seg=None, depth=None):
        """Raw ``stac_render`` on device tensors (outputs preallocated by the caller, each may be None)."""
        N = int(cam.shape[0])
        self.engine._check(self.lib.stac_render(
            C.c_void_p(self._h), N, _ptr(xpos), _ptr(xquat), _ptr(kp), _ptr(markers), 1 if show_error else 0, _ptr(cam),
            C.c_float(float(tan_half_fovy)), int(width), int(height), _ptr(rgb), _ptr(seg), _ptr(depth), self.engine._stream()))

    def close(self):
        if getattr(self, "_h", None):
            self.lib.stac_render_scene_destroy(C.c_void_p(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- cameras (torch, float64, any device) --------------------------------------------------------------------------------
def quat_to_mat(q: torch.Tensor) -> torch.Tensor:
    """[..., 4] w,x,y,z -> [..., 3, 3] (columns = the rotated frame's axes)."""
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y),
    ], -1).reshape(q.shape[:-1] + (3, 3))  # fmt: skip


def subtree_com(xpos, xquat, body_mass, body_ipos, parent) -> torch.Tensor:
    """[N, nbody, 3] centre of mass of every body's subtree (MuJoCo's subtree_com; a massless subtree: its body's xpos)."""
    xpos = xpos.to(torch.float64)
    R = quat_to_mat(xquat.to(torch.float64))
    m = torch.as_tensor(body_mass, dtype=torch.float64, device=xpos.device)
    ip = torch.as_tensor(body_ipos, dtype=torch.float64, device=xpos.device)
    xipos = xpos + torch.einsum("nbij,bj->nbi", R, ip)
    mass = m.clone().expand(xpos.shape[0], -1).clone()
    acc = xipos * m[None, :, None]
    for b in range(len(parent) - 1, 0, -1):
        p = int(parent[b])
        acc[:, p] += acc[:, b]
        mass[:, p] += mass[:, b]
    com = acc / mass.clamp_min(1e-300)[..., None]
    return torch.where(mass[..., None] > 0, com, xpos)


def camera_frames(scene: RenderScene, parent, camera: int, xpos, xquat, xpos0=None, xquat0=None):
    """Per-frame cameras ``[N, 12]`` (position, row-major rotation whose columns are the camera axes) in float64 and
    ``tan(fovy / 2)``.  ``xpos0`` / ``xquat0`` ([nbody, 3] / [nbody, 4]): the bodies at qpos0 (track / trackcom).

    camera = -1 is the free camera: it looks at the centre c of the first frame's body positions (bodies 1..) from the
    model's ``<visual><global azimuth elevation>``, at distance FREE_CAMERA_DISTANCE * s / tan(fovy / 2), where s is the
    largest distance of those positions from c (at least 1 cm), and stays there for the whole call."""
    xpos = xpos.to(torch.float64)
    N = xpos.shape[0]
    dev = xpos.device
    if camera == -1:
        tanh = math.tan(math.radians(scene.fovy) / 2)
        pts = xpos[0, 1:] if xpos.shape[1] > 1 else xpos[0]
        c = pts.mean(0)
        s = max(float((pts - c).norm(dim=-1).max()), 0.01)
        az, el = math.radians(scene.azimuth), math.radians(scene.elevation)
        fwd = torch.tensor([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)], dtype=torch.float64, device=dev)
        pos = c - FREE_CAMERA_DISTANCE * s / tanh * fwd
        up = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=dev)
        xa = torch.linalg.cross(fwd, up)
        xa = xa / xa.norm()
        za = -fwd
        ya = torch.linalg.cross(za, xa)
        R = torch.stack([xa, ya, za], 1)
        return torch.cat([pos, R.reshape(9)])[None].expand(N, 12).contiguous(), tanh
    if not 0 <= camera < len(scene.cam_names):
        raise ValueError(f"camera {camera} out of range: the model has {len(scene.cam_names)} cameras {scene.cam_names}")
    b = int(scene.cam_body[camera])
    mode = scene.cam_mode[camera]
    lp = torch.as_tensor(scene.cam_pos[camera], dtype=torch.float64, device=dev)
    Rl = quat_to_mat(torch.as_tensor(scene.cam_quat[camera], dtype=torch.float64, device=dev))
    tanh = math.tan(math.radians(float(scene.cam_fovy[camera])) / 2)
    if mode == "fixed":
        Rb = quat_to_mat(xquat[:, b].to(torch.float64))
        pos = xpos[:, b] + Rb @ lp
        R = Rb @ Rl
    else:
        x0 = torch.as_tensor(xpos0, dtype=torch.float64, device=dev)
        Rb0 = quat_to_mat(torch.as_tensor(xquat0, dtype=torch.float64, device=dev)[b])
        cam0 = x0[b] + Rb0 @ lp
        R = (Rb0 @ Rl)[None].expand(N, 3, 3)
        if mode == "track":
            pos = xpos[:, b] + (cam0 - x0[b])
        else:
            q0 = torch.as_tensor(xquat0, dtype=torch.float64, device=dev)
            com0 = subtree_com(x0[None], q0[None], scene.body_mass, scene.body_ipos, parent)[0, b]
            com = subtree_com(xpos, xquat, scene.body_mass, scene.body_ipos, parent)[:, b]
            pos = com + (cam0 - com0)
    return torch.cat([pos, R.reshape(N, 9)], 1).contiguous(), tanh


class Renderer:
    """Renders poses of the engine's model with the scene's primitives (see the module docstring).

    ``kp_names`` / ``kp_body`` name the keypoints and the bodies their markers sit on (``KEYPOINT_MODEL_PAIRS``);
    ``kp_rgba`` [K, 4] colours the keypoints (``KEYPOINT_COLOR_PAIRS``); ``marker_size`` is ``MARKER_SIZE``;
    ``geom_groups``: the geom groups to draw (None = GEOM_GROUPS, the reference's rule; ``(0, 1, 2)`` shows the fruit fly's
    body meshes, which sit in group 1)."""

    def __init__(self, engine: Engine, scene: RenderScene, kp_names, kp_body, kp_rgba, marker_size=0.005,
                 memory_budget=1 << 30, *, geom_groups=None):
        if scene.nbody != engine.nbody:
            raise ValueError(f"scene has {scene.nbody} bodies, the engine's model {engine.nbody}")
        self.engine, self.scene = engine, scene
        self.tables = render_tables(scene, kp_rgba, marker_size, geom_groups)
        self.K = len(self.tables["kp_rgba"])
        if self.K != engine.K:
            raise ValueError(f"{self.K} keypoint colours for a model with {engine.K} markers")
        self.handle = RenderSceneHandle(engine, self.tables)
        self.memory_budget = int(memory_budget)
        kp_names, kp_body = list(kp_names), list(kp_body)
        self.names = (self.tables["names"] + [f"{k}_kp" for k in kp_names] + [f"{k}_new" for k in kp_names]
                      + [f"{k}-{b}" for k, b in zip(kp_names, kp_body)])
        self._parent = None
        self._pose0 = None

    @property
    def P(self):
        return self.handle.P

    def camera_index(self, camera) -> int:
        if isinstance(camera, str):
            if camera not in self.scene.cam_names:
                raise ValueError(f"unknown camera {camera!r}; the model's cameras: {self.scene.cam_names}")
            return self.scene.cam_names.index(camera)
        camera = int(camera)
        if camera != -1 and not 0 <= camera < len(self.scene.cam_names):
            raise ValueError(f"camera index {camera} out of range; the model's cameras: {self.scene.cam_names}")
        return camera

    def _qpos0_pose(self, qpos0):
        if self._pose0 is None:
            out = self.engine.fk(torch.as_tensor(np.asarray(qpos0, np.float32)[None]), want=("xpos", "xquat"))
            self._pose0 = (out["xpos"][0].double(), out["xquat"][0].double())
        return self._pose0

    def poses(self, qpos, offsets):
        """FK at ``offsets``: xpos, xquat and the marker positions; the engine's own site positions are restored."""
        eng = self.engine
        old = eng.get_site_pos()
        try:
            eng.set_site_pos(torch.as_tensor(np.asarray(offsets, np.float32)).reshape(-1, 3))
            out = eng.fk(qpos, want=("xpos", "xquat", "site_xpos"))
        finally:
            eng.set_site_pos(old)
        return out["xpos"], out["xquat"], out["site_xpos"]

    def cameras(self, camera, xpos, xquat, qpos0, parent):
        camera = self.camera_index(camera)
        x0 = q0 = None
        if camera >= 0 and self.scene.cam_mode[camera] != "fixed":
            x0, q0 = self._qpos0_pose(qpos0)
        cam, tanh = camera_frames(self.scene, parent, camera, xpos, xquat, x0, q0)
        return cam.to(torch.float32).contiguous(), tanh

    def render(self, qpos, kp, offsets, *, qpos0, parent, camera=0, width=1920, height=1200, show_marker_error=False,
               want_seg=False, want_depth=False, want_jpeg=False, want_rgb=True, jpeg_quality=None, restart_mcus=None):
        """qpos [N, nq], kp [N, 3K] (NaN = missing keypoint) -> {"rgb": [N,H,W,3] uint8, "seg", "depth"} (CPU tensors).

        ``want_jpeg``: every chunk is also encoded on the device (``stac_mjx_amd.jpeg``) and ``out["jpeg"]`` is the list of
        the frames' JPEG files (``jpeg_quality``: None = ``video.JPEG_QUALITY``; ``restart_mcus``: None = one MCU row).
        ``want_rgb=False``: the raw frames stay on the device and ``out`` has no ``"rgb"``."""
        dev = self.engine.device
        q = torch.as_tensor(np.asarray(qpos, np.float32)).to(dev).reshape(-1, self.engine.nq)
        N = q.shape[0]
        kpt = torch.as_tensor(np.asarray(kp, np.float32)).to(dev).reshape(N, self.K, 3)
        xpos, xquat, markers = self.poses(q, offsets)
        cam, tanh = self.cameras(camera, xpos, xquat, qpos0, parent)
        per_frame = height * width * (3 + 4 * want_seg + 4 * want_depth)
        if want_jpeg:  # the encoder's workspace and its output buffer share the budget
            from . import jpeg

            quality = jpeg.JPEG_QUALITY if jpeg_quality is None else int(jpeg_quality)
            R = jpeg.default_restart_mcus(width) if restart_mcus is None else int(restart_mcus)
            per_frame += jpeg.workspace_bytes(1, width, height, R) + jpeg.JpegEncoder.first_guess(1, width, height)
        chunk = int(max(1, min(N, self.memory_budget // max(per_frame, 1))))
        out = {}
        if want_rgb:
            out["rgb"] = torch.empty((N, height, width, 3), dtype=torch.uint8)
        if want_seg:
            out["seg"] = torch.empty((N, height, width), dtype=torch.int32)
        if want_depth:
            out["depth"] = torch.empty((N, height, width), dtype=torch.float32)
        dbuf = {k: torch.empty((chunk,) + v.shape[1:], dtype=v.dtype, device=dev) for k, v in out.items()}
        if want_jpeg:
            if not want_rgb:
                dbuf["rgb"] = torch.empty((chunk, height, width, 3), dtype=torch.uint8, device=dev)
            enc = jpeg.JpegEncoder(chunk, width, height, quality, R, dev)
            jpegs = []
        for lo in range(0, N, chunk):
            hi = min(N, lo + chunk)
            n = hi - lo
            self.handle.render(xpos[lo:hi], xquat[lo:hi], kpt[lo:hi], markers[lo:hi], show_marker_error, cam[lo:hi], tanh,
                               width, height, dbuf["rgb"][:n] if "rgb" in dbuf else None, dbuf["seg"][:n] if want_seg else None,
                               dbuf["depth"][:n] if want_depth else None)
            if want_jpeg:
                jpegs.extend(enc.encode(dbuf["rgb"][:n]))
            for k in out:
                out[k][lo:hi].copy_(dbuf[k][:n])
        if want_jpeg:
            out["jpeg"] = jpegs
        out["cam"], out["tan_half_fovy"] = cam, tanh
        out["xpos"], out["xquat"], out["markers"], out["kp"] = xpos, xquat, markers, kpt
        return out

    def close(self):
        self.handle.close()
