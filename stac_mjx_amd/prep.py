"""Filling missing keypoints before the fit on the GPU: ``fill_missing`` over ``stac_prep_fill`` (csrc/stac_prep.hip) and
``summary`` of the gap lengths it returns.

A keypoint is missing in a frame when one of its coordinates is NaN or infinite.  Every track is filled along time on its own
(``linear``: interpolation between its two valid neighbours in double; ``hold``: the nearer neighbour; leading and trailing runs
copy their one neighbour), valid values pass bit for bit, and ``gap`` holds, per frame and keypoint, 0 or the length of the
missing run: DESIGN.md "Filling missing keypoints".
"""

from __future__ import annotations

import ctypes as C

import torch

from .engine import StacHipError, _ptr, load_library

TILE_FRAMES = 64    # csrc/stac_prep.hpp: kPrepTileFrames (frames of a tile of the staged scan)
MAX_BLOCKS = 1024   # csrc/stac_prep.hpp: kPrepMaxBlocks (workgroups of a launch: the grid strides over the tiles beyond that)
MODES = {"linear": 0, "hold": 1}  # include/stac_hip.h: STAC_PREP_LINEAR, STAC_PREP_HOLD


def bind(lib):
    """Argument types of the two entry points (idempotent)."""
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.stac_prep_fill_workspace.restype = i64
    lib.stac_prep_fill_workspace.argtypes = [i64, i32]
    lib.stac_prep_fill.restype = i32
    lib.stac_prep_fill.argtypes = [vp, i64, i32, i32, vp, vp, vp, i64, vp]
    return lib


def _fail(lib, what, rc):
    raise StacHipError(f"{what}: libstac_hip error {rc}: {lib.stac_last_error().decode('utf-8', 'replace')}")


def mode_code(mode) -> int:
    if mode not in MODES:
        raise ValueError(f"fill_missing: mode must be linear or hold, not {mode!r}")
    return MODES[mode]


def workspace_bytes(n_frames: int, n_kp: int) -> int:
    """Bytes of device workspace of one ``stac_prep_fill`` call (host only)."""
    lib = bind(load_library())
    b = int(lib.stac_prep_fill_workspace(int(n_frames), int(n_kp)))
    if b < 0:
        _fail(lib, "stac_prep_fill_workspace", b)
    return b


def fill_missing(kp: torch.Tensor, mode: str = "linear"):
    """Device tensor [T, 3K] -> (filled [T, 3K] float32, gap [T, K] int32), on the current stream of its device.  The input is
    made contiguous float32 first and is never written."""
    code = mode_code(mode)
    if not isinstance(kp, torch.Tensor) or not kp.is_cuda:
        raise ValueError("fill_missing needs a CUDA tensor")
    if kp.dim() != 2 or kp.shape[1] % 3 != 0 or kp.shape[1] == 0:
        raise ValueError(f"fill_missing: kp must be [frames, 3 * keypoints], got {tuple(kp.shape)}")
    kp = kp.to(dtype=torch.float32).contiguous()
    T, K = int(kp.shape[0]), int(kp.shape[1]) // 3
    out = torch.empty_like(kp)
    gap = torch.empty((T, K), dtype=torch.int32, device=kp.device)
    if T == 0:
        return out, gap
    lib = bind(load_library())
    nbytes = workspace_bytes(T, K)
    work = torch.empty(nbytes // 8, dtype=torch.int64, device=kp.device)
    with torch.cuda.device(kp.device):
        rc = lib.stac_prep_fill(_ptr(kp), T, K, code, _ptr(out), _ptr(gap), _ptr(work), nbytes,
                                C.c_void_p(torch.cuda.current_stream(kp.device).cuda_stream))
    if rc != 0:
        _fail(lib, "stac_prep_fill", rc)
    return out, gap


def summary(gap) -> dict:
    """What a ``gap`` array [T, K] says per keypoint, computed in torch: ``missing`` (frames filled or left empty), ``longest``
    (the longest missing run) as int64 arrays [K], and ``empty`` (the keypoints without a single valid frame)."""
    g = torch.as_tensor(gap)
    if g.dim() != 2:
        raise ValueError(f"summary: gap must be [frames, keypoints], got {tuple(g.shape)}")
    T = int(g.shape[0])
    missing = (g > 0).sum(dim=0).to(torch.int64)
    longest = g.max(dim=0).values.to(torch.int64) if T else torch.zeros(g.shape[1], dtype=torch.int64)
    empty = torch.nonzero(missing == T).reshape(-1) if T else torch.zeros(0, dtype=torch.int64)
    return {"missing": missing.cpu().numpy(), "longest": longest.cpu().numpy(), "empty": [int(i) for i in empty.cpu().tolist()]}
