"""Builds and binds tests/tools/render_ref.c, the CPU restatement of the render kernel, mesh geoms included (test
infrastructure only).

Two builds, with the oracle's flags (oracle/Makefile): ``RR_REAL=float`` (the kernel's operation order: the tolerance-0
checker) and ``RR_REAL=double`` (independent evaluation; flags the pixels that float32 rounding can flip)."""

from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

TOOLS = Path(__file__).resolve().parent
SRC = TOOLS / "render_ref.c"
CFLAGS = ["-O3", "-mfma", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-Wall", "-std=c11"]


def lib_path(real: str) -> Path:
    return TOOLS / f"librender_ref_{'f32' if real == 'float' else 'f64'}.so"


def build(real: str = "float") -> Path:
    out = lib_path(real)
    if not out.exists() or out.stat().st_mtime < SRC.stat().st_mtime:
        subprocess.run(["gcc", *CFLAGS, f"-DRR_REAL={real}", "-o", str(out), str(SRC), "-lm"], check=True)
    return out


_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)


class RrScene(C.Structure):
    _fields_ = [
        ("nprim", C.c_int), ("nbody", C.c_int), ("nkp", C.c_int), ("nlight", C.c_int),
        ("prim_type", _i32p), ("prim_body", _i32p), ("prim_flags", _i32p),
        ("prim_size", _f32p), ("prim_pos", _f32p), ("prim_quat", _f32p), ("prim_rgba", _f32p), ("prim_rgb2", _f32p),
        ("prim_tex", _f32p), ("kp_rgba", _f32p), ("light_dir", _f32p), ("light_diff", _f32p),
        ("marker_rgba", C.c_float * 4), ("seg_rgba", C.c_float * 4), ("marker_r", C.c_float), ("seg_r", C.c_float),
        ("head_amb", C.c_float * 3), ("head_diff", C.c_float * 3), ("alpha", C.c_float), ("bg", C.c_float * 3),
        ("nmesh", C.c_int), ("node_offset", _i32p), ("tri_offset", _i32p), ("node_box", _f32p), ("node_link", _i32p),
        ("tri_vertex", _f32p), ("prim_mesh", _i32p),
    ]  # fmt: skip


class RenderRef:
    """``render(tables, nbody, xpos, xquat, kp, markers, show_error, cam, tan_half_fovy, W, H)`` -> rgb, seg, depth, amb
    (numpy).  ``tables``: the dict of ``stac_mjx_amd.render.render_tables``; its optional ``meshes`` entry is the dict of
    ``stac_mjx_amd.mesh.pack_meshes`` plus ``prim_mesh``.  ``brute=True`` ignores the hierarchy."""

    def __init__(self, real: str = "float"):
        self.lib = C.CDLL(str(build(real)))
        vp = C.c_void_p
        for fn in (self.lib.rr_render, self.lib.rr_render_brute):
            fn.argtypes = [C.POINTER(RrScene), C.c_int, vp, vp, vp, vp, C.c_int, vp, C.c_float, C.c_int, C.c_int, vp, vp, vp, vp]
            fn.restype = C.c_int

    def render(self, t, nbody, xpos, xquat, kp, markers, show_error, cam, tan_half_fovy, W, H, brute=False):
        keep = []

        def arr(a, dt):
            a = np.ascontiguousarray(np.asarray(a), dtype=dt)
            keep.append(a)
            return a

        def flat(a, dt, ptr):  # an empty table is passed as one zero, never read
            a = np.asarray(a)
            return arr(a.reshape(-1) if a.size else np.zeros(1), dt).ctypes.data_as(ptr)

        s = RrScene()
        s.nprim, s.nbody, s.nkp, s.nlight = len(t["prim_type"]), int(nbody), len(t["kp_rgba"]), len(t["light_dir"])
        for k in ("prim_type", "prim_body", "prim_flags"):
            setattr(s, k, arr(t[k], np.int32).ctypes.data_as(_i32p))
        for k, src in (("prim_size", "prim_size"), ("prim_pos", "prim_pos"), ("prim_quat", "prim_quat"), ("prim_rgba", "prim_rgba"),
                       ("prim_rgb2", "prim_rgb2"), ("prim_tex", "prim_texrepeat"), ("kp_rgba", "kp_rgba"),
                       ("light_dir", "light_dir"), ("light_diff", "light_diffuse")):
            setattr(s, k, flat(t[src], np.float32, _f32p))
        s.marker_rgba[:] = [float(v) for v in t["marker_rgba"]]
        s.seg_rgba[:] = [float(v) for v in t["segment_rgba"]]
        s.head_amb[:] = [float(v) for v in t["head_ambient"]]
        s.head_diff[:] = [float(v) for v in t["head_diffuse"]]
        s.bg[:] = [float(v) for v in t["background"]]
        s.marker_r, s.seg_r, s.alpha = float(t["marker_radius"]), float(t["segment_radius"]), float(t["alpha"])
        m = t.get("meshes")
        s.nmesh = 0
        if m is not None:
            s.nmesh = len(m["node_offset"]) - 1
            for k in ("node_offset", "tri_offset", "node_link", "prim_mesh"):
                setattr(s, k, flat(m[k], np.int32, _i32p))
            for k in ("node_box", "tri_vertex"):
                setattr(s, k, flat(m[k], np.float32, _f32p))
        cam = arr(cam, np.float32).reshape(-1, 12)
        N = cam.shape[0]
        xpos, xquat = arr(xpos, np.float32), arr(xquat, np.float32)
        kp = arr(kp, np.float32) if kp is not None else None
        markers = arr(markers, np.float32) if markers is not None else None
        rgb = np.zeros((N, H, W, 3), np.uint8)
        seg = np.zeros((N, H, W), np.int32)
        depth = np.zeros((N, H, W), np.float32)
        amb = np.zeros((N, H, W), np.uint8)
        p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        fn = self.lib.rr_render_brute if brute else self.lib.rr_render
        rc = fn(C.byref(s), N, p(xpos), p(xquat), p(kp), p(markers), 1 if show_error else 0, p(cam), C.c_float(float(tan_half_fovy)),
                int(W), int(H), p(rgb), p(seg), p(depth), p(amb))
        if rc != 0:
            raise RuntimeError(f"rr_render returned {rc}")
        return rgb, seg, depth, amb
