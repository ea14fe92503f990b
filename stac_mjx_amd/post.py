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
RESAMPLE_MAX_UP = 32  # csrc/stac_resample.hpp: kResampleMaxUp
RESAMPLE_MAX_DOWN = 64  # kResampleMaxDown
RESAMPLE_MAX_WIN = 256  # kResampleMaxWin
RESAMPLE_MAX_LOBES = 16
RESAMPLE_MAX_BAND = 64  # kResampleMaxBand
RESAMPLE_OVERHANG = 3  # kResampleOverhang
RESAMPLE_LDS_FLOATS = 20480  # kResampleLdsFloats
RESAMPLE_MAX_TILE = 128  # kResampleMaxTile


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


# ---- stac.resample (engine extension; DESIGN.md "Resampling fitted poses") ---------------------------------------------------------
def resample_ratio(from_hz, to_hz) -> tuple:
    """``to_hz / from_hz`` in lowest terms -> ``(U, D)``: the series goes up by U and down by D.  The rates are read through their
    decimal text (``fractions.Fraction(str(rate))``), so 29.97 is 2997 / 100 and not its binary neighbour.  ``ValueError`` for a
    rate that is not a finite number > 0, and for a ratio with U > 32 or D > 64 (29.97 -> 50 is 5000 / 2997)."""
    from .config import resample_ratio as ratio

    rates = [v.item() if isinstance(v, np.generic) else v for v in (from_hz, to_hz)]
    U, D = ratio(rates[0], rates[1], ValueError, ("resample_ratio: from_hz", "resample_ratio: to_hz"))
    return int(U), int(D)


def _check_ratio(who, U, D):
    for name, v, hi in (("U", U, RESAMPLE_MAX_UP), ("D", D, RESAMPLE_MAX_DOWN)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= hi:
            raise ValueError(f"{who}: {name} must be an integer in 1 .. {hi}, not {v!r}")
    return int(U), int(D)


def resample_rows(L: int, U: int, D: int) -> int:
    """Output rows of a clip of ``L >= 1`` input rows: ``((L - 1) * U) // D + 1`` -- output m sits at input position m D / U and
    none lies beyond the last sample (csrc/stac_resample.hpp: resample_rows)."""
    U, D = _check_ratio("resample_rows", U, D)
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or L < 1:
        raise ValueError(f"resample_rows: a clip has at least one row, not {L!r}")
    return ((int(L) - 1) * U) // D + 1


def resample_source_rows(L: int, U: int, D: int) -> np.ndarray:
    """The nearest input row of every output of a clip of ``L`` rows, int64 [Lo]: ``n + (2 r > U)`` with ``n, r = divmod(m D, U)``,
    a tie goes down, clamped to L - 1.  What a per-frame mark of the resampled clip is gathered with."""
    Lo = resample_rows(L, U, D)
    p = np.arange(Lo, dtype=np.int64) * int(D)
    n, r = p // int(U), p % int(U)
    return np.minimum(n + (2 * r > int(U)), int(L) - 1).astype(np.int64)


def resample_taps(U: int, D: int, lobes: int = 10, beta: float = 5.0, normalise: bool = True) -> np.ndarray:
    """The tap table [U, W] float32 of ``resample``, computed in float64 with numpy alone and rounded once.  With M = max(U, D)
    and half = lobes * M the filter is ``h[i] = (1 / M) sinc((i - half) / M) kaiser(2 half + 1, beta)[i]``, divided by its sum and
    multiplied by U: the filter of ``scipy.signal.resample_poly(x, U, D, window=("kaiser", beta))`` when lobes = 10.  Row r holds
    the W = 2 H taps (H = half // U + 1) of an output at phase r: tap j belongs to input row n + (j - H + 1) and is
    ``h[half + r - (j - H + 1) U]``, 0 outside the filter.  ``normalise``: every row is divided by its own float64 sum, so that
    a constant column stays constant (the raw rows miss 1 by up to 6.5e-4); False gives scipy's filter itself."""
    return np.ascontiguousarray(_resample_taps64(U, D, lobes, beta, normalise), dtype=np.float32)


def _resample_taps64(U, D, lobes=10, beta=5.0, normalise=True) -> np.ndarray:
    """``resample_taps`` before its rounding to float32 (tests hold it against scipy)."""
    import math

    U, D = _check_ratio("resample_taps", U, D)
    if isinstance(lobes, bool) or not isinstance(lobes, (int, np.integer)) or not 1 <= lobes <= RESAMPLE_MAX_LOBES:
        raise ValueError(f"resample_taps: lobes must be an integer in 1 .. {RESAMPLE_MAX_LOBES}, not {lobes!r}")
    if isinstance(beta, bool) or not isinstance(beta, (int, float, np.integer, np.floating)) or not math.isfinite(beta) or beta < 0:
        raise ValueError(f"resample_taps: beta must be a finite number >= 0, not {beta!r}")
    M = max(U, D)
    half = int(lobes) * M
    H = half // U + 1
    W = 2 * H
    if W > RESAMPLE_MAX_WIN:
        raise ValueError(f"resample_taps: {U} / {D} with lobes = {lobes} needs {W} taps per output, at most {RESAMPLE_MAX_WIN}: fewer lobes")
    i = np.arange(2 * half + 1, dtype=np.float64)
    h = (1.0 / M) * np.sinc((i - half) / M) * np.kaiser(2 * half + 1, float(beta))
    h = h / h.sum() * U
    idx = half + np.arange(U)[:, None] - (np.arange(W)[None, :] - H + 1) * U
    inside = (idx >= 0) & (idx <= 2 * half)
    taps = np.where(inside, h[np.clip(idx, 0, 2 * half)], 0.0)
    if normalise:
        taps = taps / taps.sum(axis=1, keepdims=True)
    return taps


def resample_band_cols(C: int) -> int:
    """Columns of a band of the resampling kernel for rows of ``C`` floats (csrc/stac_resample.hpp: resample_band_cols)."""
    nb = -(-int(C) // RESAMPLE_MAX_BAND)
    return -(-int(C) // nb)


def resample_lds_floats(T: int, bw: int, U: int, D: int, H: int) -> int:
    """LDS floats of a tile of ``T`` outputs of a band of ``bw`` columns (csrc/stac_resample.hpp: resample_lds_floats)."""
    rows = ((T - 1) * D + U - 1) // U + 2 * H
    return min(T, U) * 2 * H + 2 * bw + rows * (bw + RESAMPLE_OVERHANG)


def resample_tile_rows(C: int, U: int, D: int, W: int) -> int:
    """Outputs of a tile of the resampling kernel for rows of ``C`` floats and windows of ``W`` taps (csrc/stac_resample.hpp:
    resample_tile_rows of the band of ``C``): what tests and benchmarks size their cases by."""
    bw, H, T = resample_band_cols(C), int(W) // 2, RESAMPLE_MAX_TILE
    while T > 1 and resample_lds_floats(T, bw, U, D, H) > RESAMPLE_LDS_FLOATS:
        T -= 1
    return T - T % U if T >= U else T


def resample(x: torch.Tensor, clip_len: int, U: int, D: int, taps, quat_cols=(), lb=None, ub=None) -> torch.Tensor:
    """``x`` [N, C] (device tensor, whole clips of ``clip_len`` rows) resampled along time by U / D with the table of
    ``resample_taps`` ([U, W], a numpy array or a tensor on the device of ``x``) -> a new tensor [(N / clip_len) * Lo, C]
    (Lo = ``resample_rows``), on the current stream of its device.  Rows outside a clip are its first or last row (no window
    reaches into another clip).  ``quat_cols``: the first columns of the quaternion blocks, which are aligned to the block of the
    nearest earlier input row, summed and renormalised; every other column is a weighted sum, clamped to ``lb`` / ``ub`` ([C],
    both or neither).  A zero tap is multiplied like any other: a NaN within the window of an output reaches it.
    Bad arguments are a ``ValueError`` before the library is called."""
    x = _device_f32(x, "resample")
    if x.dim() != 2:
        raise ValueError(f"resample: x must be [N, C], got {tuple(x.shape)}")
    N, ncol = x.shape
    U, D = _check_ratio("resample", U, D)
    if isinstance(taps, torch.Tensor):
        if taps.device != x.device:
            raise ValueError(f"resample: a tensor of taps must be on {x.device}, not {taps.device}")
        taps_dev = taps.to(dtype=torch.float32).contiguous()
    else:
        taps_dev = np.ascontiguousarray(taps, dtype=np.float32)
    if taps_dev.ndim != 2 or taps_dev.shape[0] != U or taps_dev.shape[1] % 2 != 0 or not 2 <= taps_dev.shape[1] <= RESAMPLE_MAX_WIN:
        raise ValueError(f"resample: taps must be [U = {U}, W] with an even W in 2 .. {RESAMPLE_MAX_WIN}, got {tuple(taps_dev.shape)}")
    W = int(taps_dev.shape[1])
    L = int(clip_len)
    if L < 1:
        raise ValueError(f"resample: a clip has at least one row, not {L}")
    if N % L != 0:
        raise ValueError(f"cannot reshape {N} rows into clips of {L} frames")
    if ncol < 1:
        raise ValueError("resample: rows without columns")
    cols = np.ascontiguousarray(np.asarray(quat_cols, dtype=np.int64).reshape(-1))
    if cols.size > SMOOTH_MAX_QUAT:
        raise ValueError(f"resample: {cols.size} quaternion blocks, at most {SMOOTH_MAX_QUAT}")
    srt = np.sort(cols)
    if cols.size and (srt[0] < 0 or srt[-1] > ncol - 4 or np.any(np.diff(srt) < 4)):
        raise ValueError(f"resample: quaternion blocks at columns {cols.tolist()} overlap or leave the row of {ncol}")
    cols = cols.astype(np.int32)
    if (lb is None) != (ub is None):
        raise ValueError("resample: lb and ub must be given together")
    bounds = []
    for name, b in (("lb", lb), ("ub", ub)):
        if b is None:
            bounds.append(None)
            continue
        b = b if isinstance(b, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(b, dtype=np.float32))
        b = b.to(device=x.device, dtype=torch.float32).contiguous().reshape(-1)
        if b.numel() != ncol:
            raise ValueError(f"resample: {name} must have {ncol} entries, got {b.numel()}")
        bounds.append(b)
    rows = (N // L) * resample_rows(L, U, D)
    out = torch.empty((rows, ncol), dtype=torch.float32, device=x.device)
    if N == 0:
        return out
    lib = load_library()
    if not isinstance(taps_dev, torch.Tensor):
        taps_dev = torch.as_tensor(taps_dev).to(x.device)
    with torch.cuda.device(x.device):
        rc = lib.stac_post_resample(_ptr(x), N, ncol, L, U, D, (W // 2 - 1) * U, _ptr(taps_dev), cols.ctypes.data_as(_i32p), int(cols.size),
                                    _ptr(bounds[0]), _ptr(bounds[1]), _ptr(out), rows, stream_ptr(x.device))
    check(lib, "stac_post_resample", rc)
    return out
