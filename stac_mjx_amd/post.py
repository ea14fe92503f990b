"""Post-processing of a continuous run on the GPU: ``stitch`` (the cross-fade of ``utils.handle_edge_effects``) and
``infer_qvel`` (``utils.compute_velocity_from_kinematics`` per clip) over ``stac_post_stitch`` / ``stac_post_qvel``
(csrc/stac_post.hip).

The values are those of the host functions in ``utils.py``: bit for bit, except the three root-gyro columns of ``qvel``, whose
double ``acos`` / ``sin`` come from another math library (at most 2 float32 ulp): DESIGN.md "Post-processing on the GPU".
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .engine import StacHipError, _ptr, load_library
from .utils import CONTINUOUS_BATCH_OVERLAP

MAX_OVERLAP = 32  # csrc/stac_post.hpp: kPostMaxOverlap


def bind(lib):
    """Argument types of the post-processing entry points (idempotent)."""
    vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    lib.stac_post_stitch_rows.restype = i64
    lib.stac_post_stitch_rows.argtypes = [i64, i32, i32]
    lib.stac_post_stitch.restype = i32
    lib.stac_post_stitch.argtypes = [vp, i64, i32, i32, i32, C.POINTER(f64), vp, i64, vp]
    lib.stac_post_qvel.restype = i32
    lib.stac_post_qvel.argtypes = [vp, i64, i32, i32, f64, i32, f64, vp, vp]
    return lib


def _fail(lib, what, rc):
    raise StacHipError(f"{what}: libstac_hip error {rc}: {lib.stac_last_error().decode('utf-8', 'replace')}")


def crossfade_mask(overlap: int = CONTINUOUS_BATCH_OVERLAP, center: float = 0.5, steepness: float = 10.0) -> np.ndarray:
    """The fade weights m[overlap] (float64), with the very expression of ``utils.handle_edge_effects``."""
    x = np.linspace(0.0, 1.0, int(overlap))
    return 0.5 * (1.0 + np.tanh(steepness * (x - center) / 2.0))


def stitch_rows(n_clips: int, n_frames_per_clip: int, overlap: int = CONTINUOUS_BATCH_OVERLAP) -> int:
    """Rows of the stitched array of ``n_clips`` windows (host only)."""
    lib = bind(load_library())
    R = int(lib.stac_post_stitch_rows(int(n_clips), int(n_frames_per_clip), int(overlap)))
    if R < 0:
        _fail(lib, "stac_post_stitch_rows", R)
    return R


def _device_f32(x, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError(f"{what} needs a CUDA tensor (the host path is in stac_mjx_amd.utils)")
    return x.to(dtype=torch.float32).contiguous()


def stitch(x: torch.Tensor, n_frames_per_clip: int, overlap: int = CONTINUOUS_BATCH_OVERLAP) -> torch.Tensor:
    """``utils.handle_edge_effects`` on one array: device tensor [C, F + overlap, ...] -> [R, ...] (``stitch_rows``), on the
    current stream of its device."""
    x = _device_f32(x, "stitch")
    F, ov = int(n_frames_per_clip), int(overlap)
    if x.dim() < 2 or x.shape[1] != F + ov:
        raise ValueError(f"stitch: expected [clips, {F + ov}, ...] for n_frames_per_clip = {F} and overlap = {ov}, got {tuple(x.shape)}")
    lib = bind(load_library())
    n_clips, trailing = x.shape[0], tuple(x.shape[2:])
    D = int(np.prod(trailing, dtype=np.int64))
    R = stitch_rows(n_clips, F, ov)
    out = torch.empty((R,) + trailing, dtype=torch.float32, device=x.device)
    if D == 0 or R == 0:
        return out
    m = np.ascontiguousarray(crossfade_mask(ov), dtype=np.float64)
    with torch.cuda.device(x.device):
        rc = lib.stac_post_stitch(_ptr(x), n_clips, F, ov, D, m.ctypes.data_as(C.POINTER(C.c_double)), _ptr(out), R,
                                  C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    if rc != 0:
        _fail(lib, "stac_post_stitch", rc)
    return out


def infer_qvel(qpos: torch.Tensor, n_frames_per_clip: int, dt: float, freejoint: bool, max_qvel: float = 20.0) -> torch.Tensor:
    """``utils.compute_velocity_from_kinematics`` on every clip of ``n_frames_per_clip`` rows: device tensor [N, nq] ->
    [N, nv] (nv = nq - 1 with a free joint), on the current stream of its device.  A row count that is not whole clips is a
    ``ValueError``, as the host path's reshape raises."""
    qpos = _device_f32(qpos, "infer_qvel")
    if qpos.dim() != 2:
        raise ValueError(f"infer_qvel: qpos must be [N, nq], got {tuple(qpos.shape)}")
    N, nq = qpos.shape
    F = int(n_frames_per_clip)
    if F < 1 or N % F != 0:
        raise ValueError(f"cannot reshape {N} rows of qpos into clips of {F} frames")
    if freejoint and nq < 7:
        raise ValueError(f"infer_qvel: a free joint needs nq >= 7, got {nq}")
    lib = bind(load_library())
    out = torch.empty((N, nq - (1 if freejoint else 0)), dtype=torch.float32, device=qpos.device)
    if N == 0:
        return out
    with torch.cuda.device(qpos.device):
        rc = lib.stac_post_qvel(_ptr(qpos), N, nq, F, float(dt), 1 if freejoint else 0, float(max_qvel), _ptr(out),
                                C.c_void_p(torch.cuda.current_stream(qpos.device).cuda_stream))
    if rc != 0:
        _fail(lib, "stac_post_qvel", rc)
    return out
