"""Pose steps of a fitted series (``stac.seam_report``; DESIGN.md "Warm-started clips and pose steps"): ``seam_steps`` over
``stac_seam_steps`` of the companion library ``csrc/seam/libstac_seam.so`` -- per row how far the pose moved since the row before it,
per column the largest step within the clips and across their borders, one fused pass on the GPU -- and ``summarize``, what
``<ik file>.seams.json`` holds.

The rule is stated once, in ``csrc/seam/stac_seam.hpp``.  There is no tensor-operation fallback: without the built library the call
raises.
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from .abi import StacHipError, _ptr, stream_ptr
from .engine import load_seam_library

MAX_QUAT = 64    # csrc/seam/stac_seam.hpp: kSeamMaxQuat
MAX_NQ = 4096    # csrc/seam/stac_seam.hpp: kSeamMaxNq
FIRST_FRAMES = 5  # the frames at the head of a clip whose marker error the summary sets against the whole run's


def _check(lib, what, rc):
    if rc < 0:
        raise StacHipError(f"{what}: libstac_seam error {rc}: {lib.stac_seam_last_error().decode('utf-8', 'replace')}")
    return rc


def seam_steps(qpos: torch.Tensor, clip_len: int, quat_cols=(), n_lin: int = 0) -> dict:
    """Device tensor [N, nq] -> ``{step_joint [N], step_col [N] int32, step_rot [N], step_lin2 [N], col_max_in [nq], col_max_seam
    [nq]}``, device tensors, on the current stream of its device (``stac_seam_steps``; the header states every word).  ``clip_len``
    divides N; ``quat_cols``: the first columns of the quaternion blocks of a row; ``n_lin``: 3 where a row starts with a free
    joint's translation, else 0.  The input is made contiguous float32 first and is never written; no host synchronisation."""
    if not isinstance(qpos, torch.Tensor) or not qpos.is_cuda or qpos.dim() != 2:
        raise ValueError("seam_steps: qpos must be a CUDA tensor [rows, nq]")
    q = qpos.to(torch.float32).contiguous()
    N, nq = int(q.shape[0]), int(q.shape[1])
    cols = np.ascontiguousarray(np.asarray(list(quat_cols), dtype=np.int32).reshape(-1))
    lib = load_seam_library()
    mk = lambda n, dt=torch.float32: torch.empty(n, dtype=dt, device=q.device)  # noqa: E731
    out = {"step_joint": mk(N), "step_col": mk(N, torch.int32), "step_rot": mk(N), "step_lin2": mk(N), "col_max_in": mk(nq),
           "col_max_seam": mk(nq)}
    with torch.cuda.device(q.device):
        rc = lib.stac_seam_steps(_ptr(q), N, nq, int(clip_len), cols.ctypes.data_as(C.POINTER(C.c_int32)) if cols.size else None,
                                 int(cols.size), int(n_lin), _ptr(out["step_joint"]), _ptr(out["step_col"]), _ptr(out["step_rot"]),
                                 _ptr(out["step_lin2"]), _ptr(out["col_max_in"]), _ptr(out["col_max_seam"]), stream_ptr(q.device))
    _check(lib, "stac_seam_steps", rc)
    return out


def scalar_columns(nq: int, quat_cols=(), n_lin: int = 0) -> np.ndarray:
    """The columns of a row that are neither the translation nor in a quaternion block (hinges and slides), ascending, int64."""
    keep = np.ones(int(nq), bool)
    keep[: int(n_lin)] = False
    for c in quat_cols:
        keep[int(c): int(c) + 4] = False
    return np.flatnonzero(keep).astype(np.int64)


def kth_rank(permille: int, n: int) -> int:
    """The 1-based rank of the ``permille`` quantile of n values: ceil(permille n / 1000), at least 1 (integer arithmetic)."""
    return max(1, -(-int(permille) * int(n) // 1000))


def rot_degrees(r) -> np.ndarray:
    """``step_rot`` (1 - |<a, b>| of two unit quaternions) as the angle between the two orientations in degrees: 2 acos(1 - r)."""
    r = np.asarray(r, dtype=np.float64)
    return np.degrees(2.0 * np.arccos(np.clip(1.0 - r, -1.0, 1.0)))


def summarize(res: dict, clip_len: int, names_qpos, marker_sites=None, kp_data=None) -> dict:
    """The summary of ``seam_steps``' device tensors ``res``: per seam (the rows t = clip_len, 2 clip_len, ...) ``step_joint`` (rad),
    the ``names_qpos`` name of ``step_col``, the rotation in degrees and the translation in mm; the mean and the maximum of the seams'
    ``step_joint``; the exact p50 / p99 (rank ``kth_rank``; ``torch.kthvalue`` on the device) and the maximum of the finite
    ``step_joint`` within the clips; per column the largest step within the clips and across a border; and, given ``marker_sites``
    [N, K, 3] and ``kp_data`` [N, 3K], the mean marker error in mm of the first ``FIRST_FRAMES`` frames of the clips 1 .. against
    the whole run's."""
    N, L = int(res["step_joint"].shape[0]), int(clip_len)
    names = [str(n) for n in names_qpos]
    t = torch.arange(N, device=res["step_joint"].device)
    is_seam = (t % L == 0) & (t > 0)
    inner = res["step_joint"][(t % L != 0)]
    inner = inner[torch.isfinite(inner)]
    quant = {}
    for name, pm in (("p50", 500), ("p99", 990)):
        quant[name] = float(torch.kthvalue(inner, kth_rank(pm, inner.numel())).values) if inner.numel() else None
    sj = res["step_joint"][is_seam].cpu().numpy()
    sc = res["step_col"][is_seam].cpu().numpy()
    fin = sj[np.isfinite(sj)]
    num = lambda v: None if not math.isfinite(float(v)) else float(v)  # noqa: E731  (JSON has no NaN)
    out = {
        "n_rows": N, "clip_len": L, "n_seams": int(sj.size),
        "seams": {"row": [int(i) for i in range(L, N, L)], "step_joint": [num(v) for v in sj],
                  "step_col": [names[c] if 0 <= c < len(names) else None for c in sc],
                  "rot_deg": [num(v) for v in rot_degrees(res["step_rot"][is_seam].cpu().numpy())],
                  "lin_mm": [num(v) for v in np.sqrt(res["step_lin2"][is_seam].cpu().numpy().astype(np.float64)) * 1e3]},
        "seam_mean": float(fin.mean()) if fin.size else None, "seam_max": float(fin.max()) if fin.size else None,
        "within": {"n": int(inner.numel()), "p50": quant["p50"], "p99": quant["p99"], "max": float(inner.max()) if inner.numel() else None},
        "names_qpos": names, "col_max_in": [float(v) for v in res["col_max_in"].cpu().numpy()],
        "col_max_seam": [float(v) for v in res["col_max_seam"].cpu().numpy()],
    }
    if marker_sites is not None and kp_data is not None:
        m = np.asarray(marker_sites, dtype=np.float32)
        err = np.linalg.norm(m - np.asarray(kp_data, dtype=np.float32).reshape(m.shape), axis=-1).mean(axis=-1)
        rows = np.arange(N)
        head = (rows >= L) & (rows % L < FIRST_FRAMES)
        out["marker_error_mm"] = num(err.mean() * 1e3) if err.size else None
        out["marker_error_first_frames_mm"] = num(err[head].mean() * 1e3) if head.any() else None
    return out
