"""Filling missing keypoints before the fit on the GPU: ``fill_missing`` over ``stac_prep_fill`` (csrc/stac_prep.hip) and
``summary`` of the gap lengths it returns; and, in front of it, ``reject_outliers`` over ``stac_prep_reject``
(csrc/stac_outlier.hip): finite but wrong keypoints become missing ones (DESIGN.md "Rejecting keypoint outliers"); and
``reject_pairwise`` over ``stac_prep_pairwise`` (csrc/stac_pairwise.hip), the detector without a time window (DESIGN.md
"Rejecting keypoints by pairwise distances"); and, in front of all of them, ``repair_swaps`` over ``stac_prep_swaps`` (the same
unit): two keypoints that carry each other's label in a frame are exchanged back (DESIGN.md "Repairing keypoint swaps").

A keypoint is missing in a frame when one of its coordinates is NaN or infinite.  Every track is filled along time on its own
(``linear``: interpolation between its two valid neighbours in double; ``hold``: the nearer neighbour; leading and trailing runs
copy their one neighbour), valid values pass bit for bit, and ``gap`` holds, per frame and keypoint, 0 or the length of the
missing run: DESIGN.md "Filling missing keypoints".
"""

from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from .abi import _ptr, check, device_tensor, stream_ptr
from .abi import declare as bind  # noqa: F401  (the name callers of the raw library know: the whole table, idempotent)
from .engine import load_library

TILE_FRAMES = 64    # csrc/stac_prep.hpp: kPrepTileFrames (frames of a tile of the staged scan)
MAX_BLOCKS = 1024   # csrc/stac_prep.hpp: kPrepMaxBlocks (workgroups of a launch: the grid strides over the tiles beyond that)
MODES = {"linear": 0, "hold": 1}  # include/stac_hip.h: STAC_PREP_LINEAR, STAC_PREP_HOLD
MAX_HALF_WINDOW = 16  # csrc/stac_outlier.hpp: kOutlierMaxHalf (largest half-width of the outlier window)
MAD_TO_SIGMA = 1.4826  # the median absolute deviation of a normal distribution is sigma / 1.4826
PAIRWISE_MAX_KP = 64  # csrc/stac_pairwise.hpp: kPairwiseMaxKp (keypoints of reject_pairwise at most)


def mode_code(mode) -> int:
    if mode not in MODES:
        raise ValueError(f"fill_missing: mode must be linear or hold, not {mode!r}")
    return MODES[mode]


def workspace_bytes(n_frames: int, n_kp: int) -> int:
    """Bytes of device workspace of one ``stac_prep_fill`` call (host only)."""
    lib = load_library()
    return int(check(lib, "stac_prep_fill_workspace", lib.stac_prep_fill_workspace(int(n_frames), int(n_kp))))


def fill_missing(kp: torch.Tensor, mode: str = "linear"):
    """Device tensor [T, 3K] -> (filled [T, 3K] float32, gap [T, K] int32), on the current stream of its device.  The input is
    made contiguous float32 first and is never written."""
    code = mode_code(mode)
    kp = device_tensor(kp, "fill_missing needs a CUDA tensor")
    if kp.dim() != 2 or kp.shape[1] % 3 != 0 or kp.shape[1] == 0:
        raise ValueError(f"fill_missing: kp must be [frames, 3 * keypoints], got {tuple(kp.shape)}")
    T, K = int(kp.shape[0]), int(kp.shape[1]) // 3
    out = torch.empty_like(kp)
    gap = torch.empty((T, K), dtype=torch.int32, device=kp.device)
    if T == 0:
        return out, gap
    lib = load_library()
    nbytes = workspace_bytes(T, K)
    work = torch.empty(nbytes // 8, dtype=torch.int64, device=kp.device)
    with torch.cuda.device(kp.device):
        rc = lib.stac_prep_fill(_ptr(kp), T, K, code, _ptr(out), _ptr(gap), _ptr(work), nbytes, stream_ptr(kp.device))
    check(lib, "stac_prep_fill", rc)
    return out, gap


def outlier_params(half_window, n_sigma, min_dev):
    """-> (h, thr, min_dev) as ``stac_prep_reject`` takes them: ``thr = n_sigma * 1.4826`` in double.  ValueError for a half-width
    outside 1 .. 16 or a negative or non-finite ``n_sigma`` / ``min_dev``."""
    if isinstance(half_window, bool) or not isinstance(half_window, int) or not 1 <= half_window <= MAX_HALF_WINDOW:
        raise ValueError(f"reject_outliers: half_window must be an integer in 1 .. {MAX_HALF_WINDOW}, not {half_window!r}")
    vals = []
    for name, v in (("n_sigma", n_sigma), ("min_dev", min_dev)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"reject_outliers: {name} must be a finite number >= 0, not {v!r}")
        vals.append(float(v))
    thr = vals[0] * MAD_TO_SIGMA
    if not math.isfinite(thr):
        raise ValueError(f"reject_outliers: n_sigma = {n_sigma!r} is too large")
    return half_window, thr, vals[1]


def reject_outliers(kp: torch.Tensor, half_window: int = 5, n_sigma: float = 3.0, min_dev: float = 0.0):
    """Device tensor [T, 3K] -> (out [T, 3K] float32, flag [T, K] uint8), on the current stream of its device: the Hampel
    identifier per track and coordinate over the frames t - half_window .. t + half_window; a rejected keypoint leaves as three
    NaN with flag 1, everything else bit for bit.  The input is made contiguous float32 first and is never written."""
    h, thr, floor = outlier_params(half_window, n_sigma, min_dev)
    kp = device_tensor(kp, "reject_outliers needs a CUDA tensor")
    if kp.dim() != 2 or kp.shape[1] % 3 != 0 or kp.shape[1] == 0:
        raise ValueError(f"reject_outliers: kp must be [frames, 3 * keypoints], got {tuple(kp.shape)}")
    T, K = int(kp.shape[0]), int(kp.shape[1]) // 3
    out = torch.empty_like(kp)
    flag = torch.empty((T, K), dtype=torch.uint8, device=kp.device)
    if T == 0:
        return out, flag
    lib = load_library()
    with torch.cuda.device(kp.device):
        rc = lib.stac_prep_reject(_ptr(kp), T, K, h, thr, floor, _ptr(out), _ptr(flag), stream_ptr(kp.device))
    check(lib, "stac_prep_reject", rc)
    return out, flag


def pairwise_params(n_sigma, min_dev, votes):
    """-> (thr, min_dev, votes) as ``stac_prep_pairwise`` takes them: ``thr = n_sigma * 1.4826`` in double.  ValueError for a
    negative or non-finite ``n_sigma`` / ``min_dev`` or a ``votes`` that is not an integer >= 1."""
    vals = []
    for name, v in (("n_sigma", n_sigma), ("min_dev", min_dev)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"reject_pairwise: {name} must be a finite number >= 0, not {v!r}")
        vals.append(float(v))
    if isinstance(votes, bool) or not isinstance(votes, int) or not 1 <= votes <= 2**31 - 1:
        raise ValueError(f"reject_pairwise: votes must be an integer >= 1, not {votes!r}")
    thr = vals[0] * MAD_TO_SIGMA
    if not math.isfinite(thr):
        raise ValueError(f"reject_pairwise: n_sigma = {n_sigma!r} is too large")
    return thr, vals[1], votes


def pairwise_workspace_bytes(n_frames: int, n_kp: int) -> int:
    """Bytes of device workspace of one ``stac_prep_pairwise`` call (host only)."""
    lib = load_library()
    return int(check(lib, "stac_prep_pairwise_workspace", lib.stac_prep_pairwise_workspace(int(n_frames), int(n_kp))))


def reject_pairwise(kp: torch.Tensor, n_sigma: float = 6.0, min_dev: float = 0.002, votes: int = 2):
    """Device tensor [T, 3K] -> (out [T, 3K] float32, flag [T, K] uint8, stats), on the current stream of its device: a keypoint
    that is in at least ``votes`` pairs whose distance lies further than ``n_sigma * 1.4826`` median absolute deviations, and
    than ``min_dev``, from that pair's median over the whole series leaves as three NaN with flag 1 (the keypoint in the most
    such pairs first, its pairs then count for nobody else), everything else bit for bit: DESIGN.md "Rejecting keypoints by
    pairwise distances".  ``stats``: ``pair_n`` int64, ``pair_med`` and ``pair_mad`` float64, [K (K - 1) / 2] device tensors, the
    pairs (a, b), a < b, in lexicographic order.  At most 64 keypoints.  The input is made contiguous float32 first and is never
    written."""
    thr, floor, votes = pairwise_params(n_sigma, min_dev, votes)
    kp = device_tensor(kp, "reject_pairwise needs a CUDA tensor")
    if kp.dim() != 2 or kp.shape[1] % 3 != 0 or kp.shape[1] == 0:
        raise ValueError(f"reject_pairwise: kp must be [frames, 3 * keypoints], got {tuple(kp.shape)}")
    T, K = int(kp.shape[0]), int(kp.shape[1]) // 3
    P = K * (K - 1) // 2
    out = torch.empty_like(kp)
    flag = torch.empty((T, K), dtype=torch.uint8, device=kp.device)
    # (room for one element also without a pair: the entry point takes no null pointer)
    pair_n = torch.zeros(max(P, 1), dtype=torch.int64, device=kp.device)
    pair_med = torch.full((max(P, 1),), math.nan, dtype=torch.float64, device=kp.device)
    pair_mad = torch.full((max(P, 1),), math.nan, dtype=torch.float64, device=kp.device)
    stats = {"pair_n": pair_n[:P], "pair_med": pair_med[:P], "pair_mad": pair_mad[:P]}
    if T == 0:
        return out, flag, stats
    lib = load_library()
    nbytes = pairwise_workspace_bytes(T, K)
    work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=kp.device)
    with torch.cuda.device(kp.device):
        rc = lib.stac_prep_pairwise(_ptr(kp), T, K, thr, floor, votes, _ptr(out), _ptr(flag), _ptr(pair_n), _ptr(pair_med), _ptr(pair_mad),
                                    _ptr(work), nbytes, stream_ptr(kp.device))
    check(lib, "stac_prep_pairwise", rc)
    return out, flag, stats


def swaps_params(n_sigma, min_dev, min_bad):
    """-> (thr, min_dev, min_bad) as ``stac_prep_swaps`` takes them: ``thr = n_sigma * 1.4826`` in double.  ValueError for a
    negative or non-finite ``n_sigma`` / ``min_dev`` or a ``min_bad`` that is not an integer >= 1."""
    vals = []
    for name, v in (("n_sigma", n_sigma), ("min_dev", min_dev)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"repair_swaps: {name} must be a finite number >= 0, not {v!r}")
        vals.append(float(v))
    if isinstance(min_bad, bool) or not isinstance(min_bad, int) or not 1 <= min_bad <= 2**31 - 1:
        raise ValueError(f"repair_swaps: min_bad must be an integer >= 1, not {min_bad!r}")
    thr = vals[0] * MAD_TO_SIGMA
    if not math.isfinite(thr):
        raise ValueError(f"repair_swaps: n_sigma = {n_sigma!r} is too large")
    return thr, vals[1], min_bad


def swaps_pairs(pairs, n_kp: int) -> list:
    """The candidates ``pairs`` as a list of ``(a, b)`` index tuples.  ValueError for anything that is not a sequence of pairs of
    integers in ``0 .. n_kp - 1`` with ``a != b`` and every keypoint in at most one pair."""
    out, seen = [], set()
    for p in list(pairs):
        p = tuple(p)
        if len(p) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in p):
            raise ValueError(f"repair_swaps: a candidate is a pair of keypoint indices, not {p!r}")
        a, b = int(p[0]), int(p[1])
        if not (0 <= a < n_kp and 0 <= b < n_kp) or a == b:
            raise ValueError(f"repair_swaps: candidate ({a}, {b}) must name two different keypoints in 0 .. {n_kp - 1}")
        if a in seen or b in seen:
            raise ValueError(f"repair_swaps: candidate ({a}, {b}) has a keypoint that an earlier candidate holds")
        seen.update((a, b))
        out.append((a, b))
    return out


def swaps_workspace_bytes(n_frames: int, n_kp: int) -> int:
    """Bytes of device workspace of one ``stac_prep_swaps`` call (host only)."""
    lib = load_library()
    return int(check(lib, "stac_prep_swaps_workspace", lib.stac_prep_swaps_workspace(int(n_frames), int(n_kp))))


def repair_swaps(kp: torch.Tensor, pairs, n_sigma: float = 6.0, min_dev: float = 0.002, min_bad: int = 3):
    """Device tensor [T, 3K] and S candidate pairs of keypoint indices -> (out [T, 3K] float32, flag [T, S] uint8, stats), on the
    current stream of its device: in a frame where, for a candidate (a, b), at least ``min_bad`` distances from a or b to the other
    keypoints lie further than ``n_sigma * 1.4826`` median absolute deviations, and than ``min_dev``, from their pair's median over
    the whole series, and at most half as many do once the two labels are exchanged, the two keypoints are exchanged in ``out``
    bit for bit and ``flag`` is 1; everything else passes bit for bit: DESIGN.md "Repairing keypoint swaps".  ``stats`` as
    ``reject_pairwise``'s, of the series as given.  At most 64 keypoints.  The input is made contiguous float32 first and is
    never written."""
    thr, floor, min_bad = swaps_params(n_sigma, min_dev, min_bad)
    kp = device_tensor(kp, "repair_swaps needs a CUDA tensor")
    if kp.dim() != 2 or kp.shape[1] % 3 != 0 or kp.shape[1] == 0:
        raise ValueError(f"repair_swaps: kp must be [frames, 3 * keypoints], got {tuple(kp.shape)}")
    T, K = int(kp.shape[0]), int(kp.shape[1]) // 3
    cand = swaps_pairs(pairs, K)
    S, P = len(cand), K * (K - 1) // 2
    out = torch.empty_like(kp)
    flag = torch.zeros((T, max(S, 1)), dtype=torch.uint8, device=kp.device)  # (room for a column also without a candidate)
    pair_n = torch.zeros(max(P, 1), dtype=torch.int64, device=kp.device)
    pair_med = torch.full((max(P, 1),), math.nan, dtype=torch.float64, device=kp.device)
    pair_mad = torch.full((max(P, 1),), math.nan, dtype=torch.float64, device=kp.device)
    stats = {"pair_n": pair_n[:P], "pair_med": pair_med[:P], "pair_mad": pair_mad[:P]}
    if T == 0:
        return out, flag[:, :S], stats
    lib = load_library()
    nbytes = swaps_workspace_bytes(T, K)
    work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=kp.device)
    table = (ctypes.c_int32 * max(2 * S, 1))(*[v for ab in cand for v in ab])  # host memory: read before the call returns
    with torch.cuda.device(kp.device):
        rc = lib.stac_prep_swaps(_ptr(kp), T, K, table if S else None, S, thr, floor, min_bad, _ptr(out), _ptr(flag), _ptr(pair_n),
                                 _ptr(pair_med), _ptr(pair_mad), _ptr(work), nbytes, stream_ptr(kp.device))
    check(lib, "stac_prep_swaps", rc)
    return out, flag[:, :S], stats


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
