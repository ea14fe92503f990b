"""Choosing the calibration frames of a recording (``stac.fit_frames``; DESIGN.md "Choosing calibration frames"):
``select_diverse`` over ``stac_select_diverse`` of the companion library ``csrc/select/libstac_select.so`` -- greedy farthest-point
selection over the frames' pairwise keypoint distances, on the GPU -- and ``select_strided``, every (candidates / n)-th candidate, on
the host.

The rule of ``select_diverse`` is stated once, in ``csrc/select/stac_select.hpp``.  There is no tensor-operation fallback: without
the built library the call raises.
"""

from __future__ import annotations

import numpy as np
import torch

from .abi import StacHipError, _ptr, stream_ptr
from .config import checked_int
from .engine import load_select_library
from .prep import _series

MODES = ("first", "strided", "diverse")  # stac.fit_frames
MAX_KP = 64            # csrc/select/stac_select.hpp: kSelectMaxKp (keypoints of a descriptor at most; 2 at least)
MAX_FRAMES = 2**32 - 1  # csrc/select/stac_select.hpp: kSelectMaxFrames (the frame index in the key of a pick)


def _check(lib, what, rc):
    if rc < 0:
        raise StacHipError(f"{what}: libstac_select error {rc}: {lib.stac_select_last_error().decode('utf-8', 'replace')}")
    return rc


def workspace_bytes(n_frames: int, n_kp: int) -> int:
    """Bytes of device workspace of one ``stac_select_diverse`` call (host only)."""
    lib = load_select_library()
    return int(_check(lib, "stac_select_workspace", lib.stac_select_workspace(int(n_frames), int(n_kp))))


def _candidates(cand, T, fn):
    """``cand`` (None, or [T] of anything with a truth value: a tensor or an array) as a host bool array, or None."""
    if cand is None:
        return None
    c = cand.detach().cpu().numpy() if isinstance(cand, torch.Tensor) else np.asarray(cand)
    if c.shape != (T,):
        raise ValueError(f"{fn}: cand must be [{T}], one entry per frame, got {c.shape}")
    return c != 0


def select_strided(T: int, n: int, cand=None) -> np.ndarray:
    """``n`` of the ``T`` frames at even steps through the candidates, on the host: candidate number ``(i * n_cand) // n`` for
    i in 0 .. n - 1, as int64 frame indices in ascending order.  ``cand`` ([T], None: every frame) marks the candidates.
    ``ValueError`` for fewer candidates than ``n``."""
    T = checked_int(T, "select_strided: T", ValueError, 1)
    n = checked_int(n, "select_strided: n", ValueError, 1)
    c = _candidates(cand, T, "select_strided")
    frames = np.arange(T, dtype=np.int64) if c is None else np.flatnonzero(c).astype(np.int64)
    if frames.size < n:
        raise ValueError(f"select_strided: {n} frames wanted, but only {frames.size} of the {T} frames are candidates")
    return frames[[(i * int(frames.size)) // n for i in range(n)]]


def select_diverse(kp: torch.Tensor, n: int, cand=None):
    """Device tensor [T, 3K] -> ``(sel [n] int64, radius2 [n] float32, n_selected)``, device tensors in selection order and an int,
    on the current stream of its device: the first pick is the lowest-index candidate, every further pick the candidate whose
    descriptor (its K (K - 1) / 2 keypoint distances) is farthest from those of all earlier picks; ``radius2[i]`` is that squared
    distance (+inf for the first).  A frame is a candidate iff all its coordinates are finite and ``cand`` ([T], None: all ones)
    is not 0 there.  The selection stops early when every candidate equals an earlier pick or none is left: entries behind
    ``n_selected`` are -1 and NaN.  2 .. 64 keypoints, ``1 <= n <= T``.  The one host synchronisation is the read of
    ``n_selected``.  The input is made contiguous float32 first and is never written."""
    kp, T, K = _series(kp, "select_diverse")
    if K < 2 or K > MAX_KP:
        raise ValueError(f"select_diverse: 2 .. {MAX_KP} keypoints, got {K}")
    if T < 1 or T > MAX_FRAMES:
        raise ValueError(f"select_diverse: 1 .. 2^32 - 1 frames, got {T}")
    n = checked_int(n, "select_diverse: n", ValueError, 1, T)
    c = _candidates(cand, T, "select_diverse")
    cand_dev = None if c is None else torch.as_tensor(c.astype(np.uint8)).to(kp.device)
    lib = load_select_library()
    nbytes = workspace_bytes(T, K)
    work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=kp.device)
    sel = torch.empty(n, dtype=torch.int64, device=kp.device)
    radius2 = torch.empty(n, dtype=torch.float32, device=kp.device)
    n_selected = torch.empty(1, dtype=torch.int64, device=kp.device)
    with torch.cuda.device(kp.device):
        rc = lib.stac_select_diverse(_ptr(kp), T, K, _ptr(cand_dev), n, _ptr(sel), _ptr(radius2), _ptr(n_selected), _ptr(work), nbytes,
                                     stream_ptr(kp.device))
    _check(lib, "stac_select_diverse", rc)
    return sel, radius2, int(n_selected.item())
