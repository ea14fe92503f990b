"""Fit report on the GPU: ``fit_errors`` over ``stac_report_errors`` (csrc/stac_report.hip) and ``summarize`` of what it returns
(DESIGN.md "Fit report").

Per (frame, keypoint) pair the squared distance between the fitted marker and the keypoint, in double, rounded once to float32
(``sqerr``); a pair is *counted* when its six inputs are finite and the keypoint was observed (``gap == 0``).  Over the counted
pairs: per frame their number and summed squared error (the quantity of the reference's ``graph_error.ipynb``), per keypoint the
count, sum, maximum with its first frame, a histogram over ``bits >> 21`` and exact nearest-rank quantiles.  The device takes no
square root; ``summarize`` takes the few it needs on the host.
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from .abi import StacReportParams as Params  # include/stac_hip.h: stac_report_params
from .abi import check, device_tensor
from .abi import declare as bind  # noqa: F401  (the name callers of the raw library know: the whole table, idempotent)
from .engine import load_library

TILE_FRAMES = 64    # csrc/stac_report.hpp: kReportTileFrames (frames of a tile of the first pass)
MAX_BLOCKS = 1024   # csrc/stac_report.hpp: kReportMaxBlocks (workgroups of a launch: the grid strides over the work beyond that)
SEG_FRAMES = 8192   # csrc/stac_report.hpp: kReportSegFrames (frames of one keypoint per work item of a counting pass)
MAX_QUANT = 8       # csrc/stac_report.hpp: kReportMaxQuant
HIST_BINS = 1024    # csrc/stac_report.hpp: kReportBins0 (bins of `hist`: bits >> 21)
DEFAULT_PERMILLE = (500, 900, 990)
NAN_BITS = 0x7FC00000


def workspace_formula(n_frames: int, n_kp: int, n_quant: int) -> int:
    """The workspace size from the constants above (csrc/stac_report.hpp: report_layout).  Per keypoint: per tile 64 keys of 4 bytes
    and 16 bytes of partials; per quantile two histograms of 2048 and 1024 64-bit bins and 16 bytes of select state."""
    tiles = (n_frames + TILE_FRAMES - 1) // TILE_FRAMES
    return n_kp * (tiles * (4 * TILE_FRAMES + 16) + n_quant * (8 * (2048 + 1024) + 16))


def workspace_bytes(n_frames: int, n_kp: int, n_quant: int) -> int:
    """Bytes of device workspace of one ``stac_report_errors`` call (host only)."""
    lib = load_library()
    return int(check(lib, "stac_report_workspace", lib.stac_report_workspace(int(n_frames), int(n_kp), int(n_quant))))


def check_permille(permille) -> tuple:
    """-> the permille values as a tuple of ints; ``ValueError`` unless 1 .. 8 integers in 0 .. 1000."""
    if isinstance(permille, (str, bytes)) or not hasattr(permille, "__iter__"):
        raise ValueError(f"report: permille must be a list of integers in 0 .. 1000, not {permille!r}")
    p = list(permille)
    if not 1 <= len(p) <= MAX_QUANT:
        raise ValueError(f"report: 1 .. {MAX_QUANT} quantiles, not {len(p)}")
    for v in p:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 1000:
            raise ValueError(f"report: a permille value must be an integer in 0 .. 1000, not {v!r}")
    return tuple(int(v) for v in p)


def fit_errors(markers: torch.Tensor, kp: torch.Tensor, gap: torch.Tensor | None = None, permille=DEFAULT_PERMILLE) -> dict:
    """Device tensors ``markers`` [N, K, 3], ``kp`` [N, 3K] and, optionally, ``gap`` [N, K] -> a dict of device tensors: ``sqerr``
    [N, K] float32, ``frame_sse`` [N] float64, ``frame_n`` [N] int32, ``count`` [K] int64, ``sum`` [K] float64, ``max`` [K]
    float32, ``argmax`` [K] int64, ``hist`` [K, 1024] int64, ``quant`` [K, Q] float32 -- all squared distances.  Runs on the
    current stream of the inputs' device, without a copy to the host.  The inputs are made contiguous float32 / int32 first and
    are never written."""
    perm = check_permille(permille)
    Q = len(perm)
    markers = device_tensor(markers, "fit_errors needs CUDA tensors (markers is not one)")
    kp = device_tensor(kp, "fit_errors needs CUDA tensors (kp is not one)")
    gap = device_tensor(gap, "fit_errors needs CUDA tensors (gap is not one)", torch.int32) if gap is not None else None
    if markers.dim() != 3 or markers.shape[2] != 3 or markers.shape[1] == 0:
        raise ValueError(f"fit_errors: markers must be [frames, keypoints, 3], got {tuple(markers.shape)}")
    N, K = int(markers.shape[0]), int(markers.shape[1])
    if kp.dim() != 2 or tuple(kp.shape) != (N, 3 * K):
        raise ValueError(f"fit_errors: kp must be [{N}, {3 * K}] like markers, got {tuple(kp.shape)}")
    if gap is not None and tuple(gap.shape) != (N, K):
        raise ValueError(f"fit_errors: gap must be [{N}, {K}], got {tuple(gap.shape)}")
    dev = markers.device
    if kp.device != dev or (gap is not None and gap.device != dev):
        raise ValueError("fit_errors: markers, kp and gap must be on one device")
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    out = {"sqerr": new((N, K), torch.float32), "frame_sse": new((N,), torch.float64), "frame_n": new((N,), torch.int32),
           "count": new((K,), torch.int64), "sum": new((K,), torch.float64), "max": new((K,), torch.float32),
           "argmax": new((K,), torch.int64), "hist": new((K, HIST_BINS), torch.int64), "quant": new((K, Q), torch.float32)}
    if N == 0:  # the neutral element of every statistic, without a call
        out["count"].zero_()
        out["sum"].zero_()
        out["hist"].zero_()
        out["argmax"].fill_(-1)
        out["max"].fill_(float("nan"))
        out["quant"].fill_(float("nan"))
        return out
    lib = load_library()
    nbytes = workspace_bytes(N, K, Q)
    work = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    host_perm = (C.c_int32 * Q)(*perm)
    with torch.cuda.device(dev):
        p = Params(markers=markers.data_ptr(), kp=kp.data_ptr(), gap=gap.data_ptr() if gap is not None else None, n_frames=N, n_kp=K,
                   n_quant=Q, permille=host_perm, workspace=work.data_ptr(), workspace_bytes=nbytes,
                   stream=torch.cuda.current_stream(dev).cuda_stream, **{k: v.data_ptr() for k, v in out.items()})
        rc = lib.stac_report_errors(C.byref(p))
    check(lib, "stac_report_errors", rc)
    return out


def _host(res: dict) -> dict:
    return {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in res.items()}


def bin_lower_edge(b: int) -> float:
    """The smallest squared distance of bin ``b`` of ``hist``: the float32 with the bits ``b << 21``."""
    return float(np.array([int(b) << 21], np.uint32).view(np.float32)[0])


def _root(v) -> float | None:
    v = float(v)
    return None if math.isnan(v) else math.sqrt(v)


def _hist_quantile(hist, n: int, permille: int):
    """Nearest rank, lower, from a merged histogram: the distance at the LOWER edge of the bin that holds the rank."""
    if n == 0:
        return None
    rank = (permille * (n - 1)) // 1000
    b = int(np.searchsorted(np.cumsum(hist), rank, side="right"))
    return math.sqrt(bin_lower_edge(b))


def summarize(res: dict, kp_names, worst: int = 10, permille=None) -> dict:
    """What ``fit_errors`` returned (device tensors or numpy arrays) as a plain dict that serialises to JSON.  Distances are
    square roots of the squared ones, in the units of ``kp_data`` as fitted; ``None`` stands where nothing was counted.
    ``keypoints[name]``: ``n``, ``rms`` (sqrt(sum / n)), ``max``, ``quantiles`` (one distance per permille value),
    ``argmax_frame`` and ``not_counted`` (the share of frames in which the keypoint was not counted).  ``overall``: the same over
    all pairs from the summed ``count`` / ``sum`` and the merged ``hist`` -- its quantiles are therefore the lower edges of
    quarter-octave bins, not exact values -- and the mean and maximum of ``frame_sse``.  ``worst_frames``: the ``worst`` frames
    of largest ``frame_sse`` (ties to the lower frame; frames without a counted keypoint are not listed)."""
    r = _host(res)
    kp_names = [str(n) for n in kp_names]
    K, Q = r["quant"].shape
    if len(kp_names) != K:
        raise ValueError(f"summarize: {len(kp_names)} names for {K} keypoints")
    perm = check_permille(permille) if permille is not None else (DEFAULT_PERMILLE if Q == len(DEFAULT_PERMILLE) else None)
    if perm is None or len(perm) != Q:
        raise ValueError(f"summarize: the result has {Q} quantiles: give their permille values")
    if isinstance(worst, bool) or not isinstance(worst, (int, np.integer)) or worst < 0:
        raise ValueError(f"summarize: worst must be an integer >= 0, not {worst!r}")
    N = int(r["frame_sse"].shape[0])
    keypoints = {}
    for k, name in enumerate(kp_names):
        n = int(r["count"][k])
        keypoints[name] = {
            "n": n,
            "rms": math.sqrt(float(r["sum"][k]) / n) if n else None,
            "max": _root(r["max"][k]) if n else None,
            "quantiles": [(_root(v) if n else None) for v in r["quant"][k]],
            "argmax_frame": int(r["argmax"][k]),
            "not_counted": (1.0 - n / N) if N else None,
        }
    n_all = int(r["count"].sum())
    hist_all = r["hist"].sum(axis=0)
    total = float(np.sum(r["sum"][r["count"] > 0])) if n_all else 0.0
    counted_max = r["max"][r["count"] > 0]
    sse = r["frame_sse"]
    listed = np.flatnonzero(r["frame_n"] > 0)
    overall = {
        "n": n_all,
        "rms": math.sqrt(total / n_all) if n_all else None,
        "max": math.sqrt(float(counted_max.max())) if n_all else None,
        "quantiles": [_hist_quantile(hist_all, n_all, p) for p in perm],
        "not_counted": (1.0 - n_all / (N * K)) if N else None,
        "frame_sse_mean": float(np.mean(sse[listed])) if listed.size else None,
        "frame_sse_max": float(np.max(sse[listed])) if listed.size else None,
    }
    order = np.argsort(-sse, kind="stable")
    worst_frames = []
    for t in order:
        if len(worst_frames) >= worst:
            break
        if r["frame_n"][t] > 0:
            worst_frames.append({"frame": int(t), "frame_sse": float(sse[t]), "frame_n": int(r["frame_n"][t])})
    return {"n_frames": N, "permille": list(perm), "kp_names": kp_names, "keypoints": keypoints, "overall": overall,
            "worst_frames": worst_frames}


def table_lines(summary: dict) -> list:
    """One line per keypoint of a summary, for the log."""
    perm = summary["permille"]
    fmt = lambda v: "       -" if v is None else f"{v:8.5f}"  # noqa: E731
    lines = []
    for name, s in summary["keypoints"].items():
        qs = " ".join(f"p{p / 10:g} {fmt(v)}" for p, v in zip(perm, s["quantiles"]))
        lines.append(f"report: {name}: n {s['n']} rms {fmt(s['rms'])} {qs} max {fmt(s['max'])} at frame {s['argmax_frame']}")
    return lines


def overall_lines(summary: dict) -> list:
    """The two-line overall summary of a report."""
    o, perm = summary["overall"], summary["permille"]
    fmt = lambda v: "-" if v is None else f"{v:.5f}"  # noqa: E731
    qs = ", ".join(f"p{p / 10:g} >= {fmt(v)}" for p, v in zip(perm, o["quantiles"]))
    share = "-" if o["not_counted"] is None else f"{100.0 * o['not_counted']:.3f} %"
    return [f"report: {summary['n_frames']} frames, {o['n']} observed keypoints ({share} not counted): rms {fmt(o['rms'])}, {qs}, "
            f"max {fmt(o['max'])}",
            f"report: frame_sse mean {fmt(o['frame_sse_mean'])}, max {fmt(o['frame_sse_max'])}; worst frames "
            + (", ".join(str(w['frame']) for w in summary['worst_frames']) or "-")]
