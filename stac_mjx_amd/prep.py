"""Filling missing keypoints before the fit on the GPU: ``fill_missing`` over ``stac_prep_fill`` (csrc/stac_prep.hip) and
``summary`` of the gap lengths it returns; and, in front of it, ``reject_outliers`` over ``stac_prep_reject``
(csrc/stac_outlier.hip): finite but wrong keypoints become missing ones (DESIGN.md "Rejecting keypoint outliers"); and
``reject_pairwise`` over ``stac_prep_pairwise`` (csrc/stac_pairwise.hip), the detector without a time window (DESIGN.md
"Rejecting keypoints by pairwise distances"); and, in front of all of them, ``repair_swaps`` over ``stac_prep_swaps`` (the same
unit): two keypoints that carry each other's label in a frame are exchanged back (DESIGN.md "Repairing keypoint swaps"); and,
directly in front of ``fill_missing``, ``fill_donors`` over ``stac_prep_donor`` (csrc/stac_donor.hip): a missing keypoint is carried
through its gap by three rigid partners that are still tracked (DESIGN.md "Filling gaps from donor keypoints").

A keypoint is missing in a frame when one of its coordinates is NaN or infinite.  Every track is filled along time on its own
(``linear``: interpolation between its two valid neighbours in double; ``hold``: the nearer neighbour; leading and trailing runs
copy their one neighbour), valid values pass bit for bit, and ``gap`` holds, per frame and keypoint, 0 or the length of the
missing run: DESIGN.md "Filling missing keypoints".

What the four wrappers share is said once: ``_series`` (the ``[T, 3K]`` argument), ``_workspace`` (size and allocation),
``_pair_stats`` (the buffers of the pairwise statistics), ``_pair_params`` / ``_mad_threshold`` over the value checkers of
``config``.  A fifth stage: DESIGN.md "Adding a preparation stage".
"""

from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from .abi import _ptr, check, device_tensor, stream_ptr
from .abi import declare as bind  # noqa: F401  (the name callers of the raw library know: the whole table, idempotent)
from .config import INT32_MAX, checked_int, checked_number
from .engine import load_library

TILE_FRAMES = 64    # csrc/stac_prep.hpp: kPrepTileFrames (frames of a tile of the staged scan)
MAX_BLOCKS = 1024   # csrc/stac_prep.hpp: kPrepMaxBlocks (workgroups of a launch: the grid strides over the tiles beyond that)
MODES = {"linear": 0, "hold": 1}  # include/stac_hip.h: STAC_PREP_LINEAR, STAC_PREP_HOLD
MAX_HALF_WINDOW = 16  # csrc/stac_outlier.hpp: kOutlierMaxHalf (largest half-width of the outlier window)
MAD_TO_SIGMA = 1.4826  # the median absolute deviation of a normal distribution is sigma / 1.4826
PAIRWISE_MAX_KP = 64  # csrc/stac_pairwise.hpp: kPairwiseMaxKp (keypoints of reject_pairwise at most)
DONOR_MAX_TRIPLES = 8  # csrc/stac_donor.hpp: kDonorMaxTriples (donor triples of a keypoint at most; kDonorMaxKp is 64 as well)


def mode_code(mode) -> int:
    if mode not in MODES:
        raise ValueError(f"fill_missing: mode must be linear or hold, not {mode!r}")
    return MODES[mode]


def workspace_bytes(n_frames: int, n_kp: int) -> int:
    """Bytes of device workspace of one ``stac_prep_fill`` call (host only)."""
    return _workspace("stac_prep_fill", n_frames, n_kp)[0]


def _series(kp, fn):
    """-> (kp as a contiguous float32 device tensor, T, K) of the series argument [T, 3K] of the wrapper ``fn``."""
    kp = device_tensor(kp, f"{fn} needs a CUDA tensor")
    if kp.dim() != 2 or kp.shape[1] % 3 != 0 or kp.shape[1] == 0:
        raise ValueError(f"{fn}: kp must be [frames, 3 * keypoints], got {tuple(kp.shape)}")
    return kp, int(kp.shape[0]), int(kp.shape[1]) // 3


def _workspace(entry, n_frames, n_kp, device=None):
    """Bytes of device workspace of one call of the entry point ``entry`` (host only) and, with ``device``, that many bytes there
    as an int64 tensor: (bytes, tensor)."""
    lib = load_library()
    nbytes = int(check(lib, entry + "_workspace", getattr(lib, entry + "_workspace")(int(n_frames), int(n_kp))))
    return nbytes, None if device is None else torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)


def _pair_stats(K, device):
    """The statistics buffers of the K (K - 1) / 2 keypoint pairs, with room for one element also without a pair (the entry points
    take no null pointer), and ``stats``, the views of their pairs: ``pair_n`` int64 zeros, ``pair_med`` / ``pair_mad`` float64 NaN."""
    P = K * (K - 1) // 2
    bufs = (torch.zeros(max(P, 1), dtype=torch.int64, device=device), torch.full((max(P, 1),), math.nan, dtype=torch.float64, device=device),
            torch.full((max(P, 1),), math.nan, dtype=torch.float64, device=device))
    return bufs, {name: b[:P] for name, b in zip(("pair_n", "pair_med", "pair_mad"), bufs)}


def _mad_threshold(fn, n_sigma) -> float:
    """``thr = n_sigma * 1.4826`` in double, as the entry points take it."""
    thr = float(n_sigma) * MAD_TO_SIGMA
    if not math.isfinite(thr):
        raise ValueError(f"{fn}: n_sigma = {n_sigma!r} is too large")
    return thr


def _pair_params(fn, n_sigma, min_dev, count_name, count):
    checked_number(n_sigma, f"{fn}: n_sigma", ValueError)
    floor = checked_number(min_dev, f"{fn}: min_dev", ValueError)
    checked_int(count, f"{fn}: {count_name}", ValueError, 1, INT32_MAX, "an integer >= 1")
    return _mad_threshold(fn, n_sigma), floor, count


def fill_missing(kp: torch.Tensor, mode: str = "linear"):
    """Device tensor [T, 3K] -> (filled [T, 3K] float32, gap [T, K] int32), on the current stream of its device.  The input is
    made contiguous float32 first and is never written."""
    code = mode_code(mode)
    kp, T, K = _series(kp, "fill_missing")
    out = torch.empty_like(kp)
    gap = torch.empty((T, K), dtype=torch.int32, device=kp.device)
    if T == 0:
        return out, gap
    lib = load_library()
    nbytes, work = _workspace("stac_prep_fill", T, K, kp.device)
    with torch.cuda.device(kp.device):
        rc = lib.stac_prep_fill(_ptr(kp), T, K, code, _ptr(out), _ptr(gap), _ptr(work), nbytes, stream_ptr(kp.device))
    check(lib, "stac_prep_fill", rc)
    return out, gap


def outlier_params(half_window, n_sigma, min_dev):
    """-> (h, thr, min_dev) as ``stac_prep_reject`` takes them: ``thr = n_sigma * 1.4826`` in double.  ValueError for a half-width
    outside 1 .. 16 or a negative or non-finite ``n_sigma`` / ``min_dev``."""
    checked_int(half_window, "reject_outliers: half_window", ValueError, 1, MAX_HALF_WINDOW)
    checked_number(n_sigma, "reject_outliers: n_sigma", ValueError)
    floor = checked_number(min_dev, "reject_outliers: min_dev", ValueError)
    return half_window, _mad_threshold("reject_outliers", n_sigma), floor


def reject_outliers(kp: torch.Tensor, half_window: int = 5, n_sigma: float = 3.0, min_dev: float = 0.0):
    """Device tensor [T, 3K] -> (out [T, 3K] float32, flag [T, K] uint8), on the current stream of its device: the Hampel
    identifier per track and coordinate over the frames t - half_window .. t + half_window; a rejected keypoint leaves as three
    NaN with flag 1, everything else bit for bit.  The input is made contiguous float32 first and is never written."""
    h, thr, floor = outlier_params(half_window, n_sigma, min_dev)
    kp, T, K = _series(kp, "reject_outliers")
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
    return _pair_params("reject_pairwise", n_sigma, min_dev, "votes", votes)


def pairwise_workspace_bytes(n_frames: int, n_kp: int) -> int:
    """Bytes of device workspace of one ``stac_prep_pairwise`` call (host only)."""
    return _workspace("stac_prep_pairwise", n_frames, n_kp)[0]


def reject_pairwise(kp: torch.Tensor, n_sigma: float = 6.0, min_dev: float = 0.002, votes: int = 2):
    """Device tensor [T, 3K] -> (out [T, 3K] float32, flag [T, K] uint8, stats), on the current stream of its device: a keypoint
    that is in at least ``votes`` pairs whose distance lies further than ``n_sigma * 1.4826`` median absolute deviations, and
    than ``min_dev``, from that pair's median over the whole series leaves as three NaN with flag 1 (the keypoint in the most
    such pairs first, its pairs then count for nobody else), everything else bit for bit: DESIGN.md "Rejecting keypoints by
    pairwise distances".  ``stats``: ``pair_n`` int64, ``pair_med`` and ``pair_mad`` float64, [K (K - 1) / 2] device tensors, the
    pairs (a, b), a < b, in lexicographic order.  At most 64 keypoints.  The input is made contiguous float32 first and is never
    written."""
    thr, floor, votes = pairwise_params(n_sigma, min_dev, votes)
    kp, T, K = _series(kp, "reject_pairwise")
    out = torch.empty_like(kp)
    flag = torch.empty((T, K), dtype=torch.uint8, device=kp.device)
    (pair_n, pair_med, pair_mad), stats = _pair_stats(K, kp.device)
    if T == 0:
        return out, flag, stats
    lib = load_library()
    nbytes, work = _workspace("stac_prep_pairwise", T, K, kp.device)
    with torch.cuda.device(kp.device):
        rc = lib.stac_prep_pairwise(_ptr(kp), T, K, thr, floor, votes, _ptr(out), _ptr(flag), _ptr(pair_n), _ptr(pair_med), _ptr(pair_mad),
                                    _ptr(work), nbytes, stream_ptr(kp.device))
    check(lib, "stac_prep_pairwise", rc)
    return out, flag, stats


def swaps_params(n_sigma, min_dev, min_bad):
    """-> (thr, min_dev, min_bad) as ``stac_prep_swaps`` takes them: ``thr = n_sigma * 1.4826`` in double.  ValueError for a
    negative or non-finite ``n_sigma`` / ``min_dev`` or a ``min_bad`` that is not an integer >= 1."""
    return _pair_params("repair_swaps", n_sigma, min_dev, "min_bad", min_bad)


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
    return _workspace("stac_prep_swaps", n_frames, n_kp)[0]


def repair_swaps(kp: torch.Tensor, pairs, n_sigma: float = 6.0, min_dev: float = 0.002, min_bad: int = 3):
    """Device tensor [T, 3K] and S candidate pairs of keypoint indices -> (out [T, 3K] float32, flag [T, S] uint8, stats), on the
    current stream of its device: in a frame where, for a candidate (a, b), at least ``min_bad`` distances from a or b to the other
    keypoints lie further than ``n_sigma * 1.4826`` median absolute deviations, and than ``min_dev``, from their pair's median over
    the whole series, and at most half as many do once the two labels are exchanged, the two keypoints are exchanged in ``out``
    bit for bit and ``flag`` is 1; everything else passes bit for bit: DESIGN.md "Repairing keypoint swaps".  ``stats`` as
    ``reject_pairwise``'s, of the series as given.  At most 64 keypoints.  The input is made contiguous float32 first and is
    never written."""
    thr, floor, min_bad = swaps_params(n_sigma, min_dev, min_bad)
    kp, T, K = _series(kp, "repair_swaps")
    cand = swaps_pairs(pairs, K)
    S = len(cand)
    out = torch.empty_like(kp)
    flag = torch.zeros((T, max(S, 1)), dtype=torch.uint8, device=kp.device)  # (room for a column also without a candidate)
    (pair_n, pair_med, pair_mad), stats = _pair_stats(K, kp.device)
    if T == 0:
        return out, flag[:, :S], stats
    lib = load_library()
    nbytes, work = _workspace("stac_prep_swaps", T, K, kp.device)
    table = (ctypes.c_int32 * max(2 * S, 1))(*[v for ab in cand for v in ab])  # host memory: read before the call returns
    with torch.cuda.device(kp.device):
        rc = lib.stac_prep_swaps(_ptr(kp), T, K, table if S else None, S, thr, floor, min_bad, _ptr(out), _ptr(flag), _ptr(pair_n),
                                 _ptr(pair_med), _ptr(pair_mad), _ptr(work), nbytes, stream_ptr(kp.device))
    check(lib, "stac_prep_swaps", rc)
    return out, flag[:, :S], stats


def donor_triples(n_triples) -> int:
    """``n_triples`` as ``stac_prep_donor`` takes it; ValueError for anything but an integer in 1 .. 8."""
    return checked_int(n_triples, "fill_donors: n_triples", ValueError, 1, DONOR_MAX_TRIPLES)


def donor_workspace_bytes(n_frames: int, n_kp: int) -> int:
    """Bytes of device workspace of one ``stac_prep_donor`` call (host only)."""
    return _workspace("stac_prep_donor", n_frames, n_kp)[0]


def donor_table(stats, K: int, n_triples: int = 4) -> np.ndarray:
    """The automatic donor table ``[K, n_triples, 3]`` int32 from the pairwise statistics of ``reject_pairwise`` (``pair_n`` and
    ``pair_mad`` over the pairs (a, b), a < b, in lexicographic order; tensors or arrays), on the host.  The candidates of keypoint k
    are the other keypoints whose pair with k has ``pair_n >= 3`` (and a ``pair_mad`` that is a number), ordered by (``pair_mad``,
    index): the partners it keeps the steadiest distance to.  With c0 .. c3 the first four, the triples are (c0, c1, c2), (c0, c1, c3),
    (c0, c2, c3), (c1, c2, c3), those that exist, cut to ``n_triples``; fewer than three candidates give none.  A row that is no
    triple is (-1, -1, -1): the end of that keypoint's list."""
    n_triples = donor_triples(n_triples)
    K = checked_int(K, "donor_table: K", ValueError, 1, PAIRWISE_MAX_KP)
    host = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)  # noqa: E731
    pair_n, pair_mad = host(stats["pair_n"]).astype(np.int64), host(stats["pair_mad"]).astype(np.float64)
    P = K * (K - 1) // 2
    if pair_n.shape != (P,) or pair_mad.shape != (P,):
        raise ValueError(f"donor_table: pair_n and pair_mad must be [{P}], the pairs of {K} keypoints, got {pair_n.shape} and {pair_mad.shape}")
    don = np.full((K, n_triples, 3), -1, np.int32)
    for k in range(K):
        cand = []
        for j in range(K):
            if j != k:
                a, b = min(j, k), max(j, k)
                p = a * (2 * K - a - 1) // 2 + (b - a - 1)
                if pair_n[p] >= 3 and not math.isnan(pair_mad[p]):
                    cand.append((float(pair_mad[p]), j))
        c = [j for _, j in sorted(cand)[:4]]
        rows = [(c[x], c[y], c[z]) for x, y, z in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)) if z < len(c)]
        for d, row in enumerate(rows[:n_triples]):
            don[k, d] = row
    return don


def fill_donors(kp: torch.Tensor, don):
    """Device tensor [T, 3K] and a donor table ``don`` [K, D, 3] (int32; a tensor or an array, D in 1 .. 8) -> (out [T, 3K] float32,
    gap [T, K] int32, src [T, K] uint8), on the current stream of its device: a missing keypoint is filled by the first usable donor
    triple of its list -- its coordinates in the frame of the three donors, interpolated between the two ends of the gap, carried
    back by the donors' frame in its own frame -- and stays missing if there is none; everything else passes bit for bit: DESIGN.md
    "Filling gaps from donor keypoints".  ``gap`` is ``fill_missing``'s of the input; ``src`` is 0 where observed, d + 1 where triple
    d filled, 255 where missing and left so.  At most 64 keypoints.  The input is made contiguous float32 first and is never
    written."""
    kp, T, K = _series(kp, "fill_donors")
    don = don if isinstance(don, torch.Tensor) else torch.as_tensor(np.array(don))  # (a copy: torch does not wrap a read-only array)
    if don.dim() != 3 or don.shape[0] != K or don.shape[2] != 3 or don.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"fill_donors: don must be an integer table [{K}, triples, 3], got {tuple(don.shape)} {don.dtype}")
    D = donor_triples(int(don.shape[1]))
    if don.dtype == torch.int64:  # (by value: an index beyond int32 ends a list like any index out of range)
        don = don.clamp(-1, INT32_MAX)
    don = don.to(device=kp.device, dtype=torch.int32).contiguous()
    out = torch.empty_like(kp)
    gap = torch.empty((T, K), dtype=torch.int32, device=kp.device)
    src = torch.empty((T, K), dtype=torch.uint8, device=kp.device)
    if T == 0:
        return out, gap, src
    lib = load_library()
    nbytes, work = _workspace("stac_prep_donor", T, K, kp.device)
    with torch.cuda.device(kp.device):
        rc = lib.stac_prep_donor(_ptr(kp), T, K, _ptr(don), D, _ptr(out), _ptr(gap), _ptr(src), _ptr(work), nbytes, stream_ptr(kp.device))
    check(lib, "stac_prep_donor", rc)
    return out, gap, src


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
