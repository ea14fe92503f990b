"""Post-processing of a continuous run on the GPU: ``stitch`` (the cross-fade of ``utils.handle_edge_effects``) and
``infer_qvel`` (``utils.compute_velocity_from_kinematics`` per clip) over ``stac_post_stitch`` / ``stac_post_qvel``
(csrc/stac_post.hip), and between the two ``smooth`` (``stac.smooth``, an engine extension: a Savitzky-Golay or Gaussian low-pass
of ``qpos`` along time over ``stac_post_smooth``, csrc/stac_smooth.hip; DESIGN.md "Smoothing fitted poses").

The values are those of the host functions in ``utils.py``: bit for bit, except the three root-gyro columns of ``qvel``, whose
double ``acos`` / ``sin`` come from another math library (at most 2 float32 ulp): DESIGN.md "Post-processing on the GPU".
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .abi import _f32p, _i32p, _ptr, check, device_tensor, stream_ptr
from .abi import declare as bind  # noqa: F401  (the name callers of the raw library know: the whole table, idempotent)
from .engine import load_library
from .utils import CONTINUOUS_BATCH_OVERLAP

MAX_OVERLAP = 32  # csrc/stac_post.hpp: kPostMaxOverlap
SMOOTH_MAX_HALF = 16  # csrc/stac_smooth.hpp: kSmoothMaxHalf
SMOOTH_MAX_QUAT = 64  # kSmoothMaxQuat
SMOOTH_LDS_FLOATS = 16384  # kSmoothLdsFloats
SMOOTH_MAX_TILE = 128  # kSmoothMaxTile


def crossfade_mask(overlap: int = CONTINUOUS_BATCH_OVERLAP, center: float = 0.5, steepness: float = 10.0) -> np.ndarray:
    """The fade weights m[overlap] (float64), with the very expression of ``utils.handle_edge_effects``."""
    x = np.linspace(0.0, 1.0, int(overlap))
    return 0.5 * (1.0 + np.tanh(steepness * (x - center) / 2.0))


def stitch_rows(n_clips: int, n_frames_per_clip: int, overlap: int = CONTINUOUS_BATCH_OVERLAP) -> int:
    """Rows of the stitched array of ``n_clips`` windows (host only)."""
    lib = load_library()
    return int(check(lib, "stac_post_stitch_rows", lib.stac_post_stitch_rows(int(n_clips), int(n_frames_per_clip), int(overlap))))


def _device_f32(x, what):
    return device_tensor(x, f"{what} needs a CUDA tensor (the host path is in stac_mjx_amd.utils)")


def stitch(x: torch.Tensor, n_frames_per_clip: int, overlap: int = CONTINUOUS_BATCH_OVERLAP) -> torch.Tensor:
    """``utils.handle_edge_effects`` on one array: device tensor [C, F + overlap, ...] -> [R, ...] (``stitch_rows``), on the
    current stream of its device."""
    x = _device_f32(x, "stitch")
    F, ov = int(n_frames_per_clip), int(overlap)
    if x.dim() < 2 or x.shape[1] != F + ov:
        raise ValueError(f"stitch: expected [clips, {F + ov}, ...] for n_frames_per_clip = {F} and overlap = {ov}, got {tuple(x.shape)}")
    lib = load_library()
    n_clips, trailing = x.shape[0], tuple(x.shape[2:])
    D = int(np.prod(trailing, dtype=np.int64))
    R = stitch_rows(n_clips, F, ov)
    out = torch.empty((R,) + trailing, dtype=torch.float32, device=x.device)
    if D == 0 or R == 0:
        return out
    m = np.ascontiguousarray(crossfade_mask(ov), dtype=np.float64)
    with torch.cuda.device(x.device):
        rc = lib.stac_post_stitch(_ptr(x), n_clips, F, ov, D, m.ctypes.data_as(C.POINTER(C.c_double)), _ptr(out), R, stream_ptr(x.device))
    check(lib, "stac_post_stitch", rc)
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
    lib = load_library()
    out = torch.empty((N, nq - (1 if freejoint else 0)), dtype=torch.float32, device=qpos.device)
    if N == 0:
        return out
    with torch.cuda.device(qpos.device):
        rc = lib.stac_post_qvel(_ptr(qpos), N, nq, F, float(dt), 1 if freejoint else 0, float(max_qvel), _ptr(out), stream_ptr(qpos.device))
    check(lib, "stac_post_qvel", rc)
    return out


def smooth_taps(kind: str, half_window: int, order: int | None = None, sigma: float | None = None) -> np.ndarray:
    """The tap table [W, W] float32 of ``smooth`` (W = 2 * half_window + 1), computed in float64 with numpy alone and rounded
    once.  Row p holds the weights of an output at window position p: row ``half_window`` is the filter of the interior of a
    clip, the rows before and after it serve the first and last ``half_window`` frames.

    ``savgol``: ``A @ pinv(A)`` of ``A = vander(j - half_window, order + 1)`` (computed from a QR factorisation): row p evaluates at position p the polynomial of
    ``order`` (default 2, 0 <= order < W) that fits the window in the least-squares sense -- ``scipy.signal.savgol_filter`` with
    ``mode="interp"``.  ``gaussian``: ``exp(-(j - p)^2 / (2 sigma^2))`` (``sigma`` in frames, default ``half_window / 2``), every
    row normalised to sum 1 in float64: at the ends the truncated, renormalised kernel."""
    return np.ascontiguousarray(_smooth_taps64(kind, half_window, order, sigma), dtype=np.float32)


def _smooth_taps64(kind, half_window, order, sigma) -> np.ndarray:
    """``smooth_taps`` before its rounding to float32 (tests hold it against scipy's coefficients)."""
    import math

    H = half_window
    if isinstance(H, bool) or not isinstance(H, (int, np.integer)) or not 1 <= H <= SMOOTH_MAX_HALF:
        raise ValueError(f"smooth_taps: half_window must be an integer in 1 .. {SMOOTH_MAX_HALF}, not {H!r}")
    H = int(H)
    W = 2 * H + 1
    j = np.arange(W, dtype=np.float64)
    if kind == "savgol":
        if sigma is not None:
            raise ValueError("smooth_taps: sigma belongs to kind = gaussian")
        order = 2 if order is None else order
        if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 0 <= order < W:
            raise ValueError(f"smooth_taps: order must be an integer with 0 <= order < {W}, not {order!r}")
        # A @ pinv(A) is the orthogonal projector onto the columns of A.  Scaling a column does not change their span, and Q Q^T of a
        # QR factorisation is that projector again: (j - H) / H and QR hold 1e-15 of exact rational arithmetic at every order, where
        # the literal float64 expression loses 1e-12 at H = 16, order 4 and everything at order 2 H (pinv drops singular values)
        q, _ = np.linalg.qr(np.vander((j - H) / H, int(order) + 1))
        taps = q @ q.T
    elif kind == "gaussian":
        if order is not None:
            raise ValueError("smooth_taps: order belongs to kind = savgol")
        sigma = H / 2.0 if sigma is None else sigma
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.floating, np.integer)) or not math.isfinite(sigma) or not sigma > 0:
            raise ValueError(f"smooth_taps: sigma must be a finite number > 0, not {sigma!r}")
        taps = np.exp(-((j[None, :] - j[:, None]) ** 2) / (2.0 * float(sigma) ** 2))
        taps = taps / taps.sum(axis=1, keepdims=True)
    else:
        raise ValueError(f"smooth_taps: kind must be savgol or gaussian, not {kind!r}")
    return taps


def smooth_tile_frames(nq: int, half_window: int) -> int:
    """Frames of a tile of the smoothing kernel for rows of ``nq`` floats (csrc/stac_smooth.hpp: smooth_tile_frames; 0 = the
    rows do not fit): what tests and benchmarks size their cases by."""
    W = 2 * half_window + 1
    T = (SMOOTH_LDS_FLOATS - W * W) // nq - 2 - 2 * half_window
    return 0 if T < 1 else min(T, SMOOTH_MAX_TILE)


def smooth(qpos: torch.Tensor, clip_len: int, taps, quat_cols, lb=None, ub=None) -> torch.Tensor:
    """``qpos`` [N, nq] (device tensor, whole clips of ``clip_len`` rows) filtered along time with the table of ``smooth_taps``
    -> a new tensor [N, nq], on the current stream of its device.  ``quat_cols``: the first columns of the quaternion blocks (3
    for a free joint, the address of every ball joint), which are aligned to their centre frame, summed and renormalised; every
    other column is a weighted sum, clamped to ``lb`` / ``ub`` ([nq], both or neither).  No window reaches into another clip.
    Bad arguments are a ``ValueError`` before the library is called."""
    qpos = _device_f32(qpos, "smooth")
    if qpos.dim() != 2:
        raise ValueError(f"smooth: qpos must be [N, nq], got {tuple(qpos.shape)}")
    N, nq = qpos.shape
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    if taps.ndim != 2 or taps.shape[0] != taps.shape[1] or taps.shape[0] % 2 != 1 or not 3 <= taps.shape[0] <= 2 * SMOOTH_MAX_HALF + 1:
        raise ValueError(f"smooth: taps must be [W, W] with W = 2 * half_window + 1, half_window in 1 .. {SMOOTH_MAX_HALF}, got {taps.shape}")
    W = taps.shape[0]
    L = int(clip_len)
    if L < W:
        raise ValueError(f"smooth: clips of {L} frames are shorter than the window of {W} frames")
    if N % L != 0:
        raise ValueError(f"cannot reshape {N} rows of qpos into clips of {L} frames")
    if nq < 1 or smooth_tile_frames(nq, W // 2) < 1:
        raise ValueError(f"smooth: rows of {nq} values leave no room for a window of {W} frames in the kernel's LDS")
    cols = np.ascontiguousarray(np.asarray(quat_cols, dtype=np.int64).reshape(-1))
    if cols.size > SMOOTH_MAX_QUAT:
        raise ValueError(f"smooth: {cols.size} quaternion blocks, at most {SMOOTH_MAX_QUAT}")
    srt = np.sort(cols)
    if cols.size and (srt[0] < 0 or srt[-1] > nq - 4 or np.any(np.diff(srt) < 4)):
        raise ValueError(f"smooth: quaternion blocks at columns {cols.tolist()} overlap or leave the row of {nq}")
    cols = cols.astype(np.int32)
    if (lb is None) != (ub is None):
        raise ValueError("smooth: lb and ub must be given together")
    bounds = []
    for name, b in (("lb", lb), ("ub", ub)):
        if b is None:
            bounds.append(None)
            continue
        b = b if isinstance(b, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(b, dtype=np.float32))
        b = b.to(device=qpos.device, dtype=torch.float32).contiguous().reshape(-1)
        if b.numel() != nq:
            raise ValueError(f"smooth: {name} must have {nq} entries, got {b.numel()}")
        bounds.append(b)
    lib = load_library()
    out = torch.empty_like(qpos)
    if N == 0:
        return out
    with torch.cuda.device(qpos.device):
        rc = lib.stac_post_smooth(_ptr(qpos), N, nq, L, W // 2, taps.ctypes.data_as(_f32p), cols.ctypes.data_as(_i32p), int(cols.size),
                                  _ptr(bounds[0]), _ptr(bounds[1]), _ptr(out), stream_ptr(qpos.device))
    check(lib, "stac_post_smooth", rc)
    return out
