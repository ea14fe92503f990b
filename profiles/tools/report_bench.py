"""``stac_report_errors`` (stac.report) on one GPU against a plain torch statement of the same rule (DESIGN.md "Fit report",
profiles/report/report_bench.json).

  python profiles/tools/report_bench.py --out profiles/report/report_bench.json [--frames 1000000] [--kp 23] [--reps 20]

Markers are seeded keypoints plus residuals of 1 mm times a log-normal factor; 3 % of the pairs have ``gap > 0``.  Each side is timed
by device events around one call on preallocated buffers (the kernel side: the whole of ``stac_report_errors``, two memsets and
seven launches; the torch side: ``torch_report`` below), ``--reps`` times after three warm-up calls.  Every exact output is compared
bit for bit, and both sides' ``sum`` against ``math.fsum`` on the host within count * 2^-52 * fsum.  Bytes: what has to move at least
(the inputs read once, ``sqerr`` written once and read twice) over the kernel time, against the HBM peak; and what this
implementation moves (the keys written once and read three times instead of the two reads of ``sqerr``).  ``--bench-this`` /
``--bench-parent``: frames/s of ``bench.py``'s default line measured elsewhere in the same session, recorded as given.
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT)]

HBM_PEAK_SPEC = 8.0e12       # bytes/s, MI355X data sheet
HBM_PEAK_MEASURED = 6.29e12  # bytes/s, a float4 copy kernel on this part
NAN_BITS = 0x7FC00000


def torch_report(markers, kp, gap, permille):
    """The rule in plain torch: double arithmetic (every operation one torch call, so it rounds as the kernel's), a ``torch.sort``
    per keypoint column, gathers at the ranks, a ``bincount`` of ``bits >> 21``.  No copy to the host."""
    N, K = markers.shape[:2]
    dev = markers.device
    y = kp.view(N, K, 3)
    d = markers.double() - y.double()
    sq = d * d
    e = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    finite = torch.isfinite(markers).all(dim=2) & torch.isfinite(y).all(dim=2)
    nan = torch.tensor([NAN_BITS], dtype=torch.int32, device=dev).view(torch.float32)
    sqerr = torch.where(finite, e.float(), nan)
    counted = finite & (gap == 0) if gap is not None else finite
    frame_n = counted.sum(dim=1, dtype=torch.int32)
    frame_sse = torch.zeros(N, dtype=torch.float64, device=dev)
    for k in range(K):  # ascending k, sequentially
        frame_sse = torch.where(counted[:, k], frame_sse + e[:, k], frame_sse)
    count = counted.sum(dim=0)
    total = torch.where(counted, e, torch.zeros((), dtype=torch.float64, device=dev)).sum(dim=0)
    bits = sqerr.view(torch.int32)
    key = torch.where(counted, bits, torch.full((), 0x7FFFFFFF, dtype=torch.int32, device=dev))  # not counted: sorts last
    perm = torch.tensor(list(permille), dtype=torch.int64, device=dev)
    nan_bits = torch.full((), NAN_BITS, dtype=torch.int32, device=dev)
    mx, argmax, hist, quant = [], [], [], []
    for k in range(K):
        col = key[:, k]
        s = torch.sort(col).values
        n = count[k]
        last = (n - 1).clamp(min=0)
        top = s[last]
        mx.append(torch.where(n > 0, top, nan_bits))
        argmax.append(torch.where(n > 0, (col == top).to(torch.uint8).argmax(), torch.full((), -1, dtype=torch.int64, device=dev)))
        quant.append(torch.where(n > 0, s[(perm * last) // 1000], nan_bits))
        hist.append(torch.bincount(bits[:, k] >> 21, weights=counted[:, k].double(), minlength=1024)[:1024].long())
    return {"sqerr": sqerr, "frame_sse": frame_sse, "frame_n": frame_n, "count": count, "sum": total,
            "max": torch.stack(mx).view(torch.float32), "argmax": torch.stack(argmax), "hist": torch.stack(hist),
            "quant": torch.stack(quant).view(torch.float32)}


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms_median": float(np.median(ms)), "ms_min_max": [float(min(ms)), float(max(ms))], "reps": reps}


def _bits(t):
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--kp", type=int, default=23)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bench-this", default="")
    ap.add_argument("--bench-parent", default="")
    args = ap.parse_args()

    from stac_mjx_amd import report
    from stac_mjx_amd.engine import load_library

    if not torch.cuda.is_available():
        raise SystemExit("report_bench needs a GPU: nothing is measured without one")
    lib = load_library()
    N, K, permille = args.frames, args.kp, report.DEFAULT_PERMILLE
    Q = len(permille)
    rng = np.random.default_rng(9)
    kp_np = (0.05 * rng.standard_normal((N, K, 3))).astype(np.float32)
    m_np = kp_np + (0.001 * rng.standard_normal((N, K, 3)) * rng.lognormal(0.0, 0.5, (N, K, 1))).astype(np.float32)
    gap_np = np.where(rng.random((N, K)) < 0.03, 3, 0).astype(np.int32)
    markers, kp, gap = torch.as_tensor(m_np).cuda(), torch.as_tensor(kp_np.reshape(N, 3 * K)).cuda(), torch.as_tensor(gap_np).cuda()

    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device="cuda")  # noqa: E731
    out = {"sqerr": new((N, K), torch.float32), "frame_sse": new((N,), torch.float64), "frame_n": new((N,), torch.int32),
           "count": new((K,), torch.int64), "sum": new((K,), torch.float64), "max": new((K,), torch.float32),
           "argmax": new((K,), torch.int64), "hist": new((K, 1024), torch.int64), "quant": new((K, Q), torch.float32)}
    nbytes = report.workspace_bytes(N, K, Q)
    work = new((nbytes // 8,), torch.int64)
    host_perm = (C.c_int32 * Q)(*permille)
    params = report.Params(markers=markers.data_ptr(), kp=kp.data_ptr(), gap=gap.data_ptr(), n_frames=N, n_kp=K, n_quant=Q, permille=host_perm,
                           workspace=work.data_ptr(), workspace_bytes=nbytes, stream=torch.cuda.current_stream().cuda_stream,
                           **{k: v.data_ptr() for k, v in out.items()})

    def kernel():
        rc = lib.stac_report_errors(C.byref(params))
        assert rc == 0, lib.stac_last_error().decode()

    k_time = timed(kernel, args.reps)
    t_time = timed(lambda: torch_report(markers, kp, gap, permille), max(args.reps // 4, 3))
    ref = torch_report(markers, kp, gap, permille)
    equal = {name: bool(torch.equal(_bits(out[name]), _bits(ref[name]))) for name in out if name != "sum"}
    # both sums against fsum on the host
    d = m_np.astype(np.float64) - kp_np.astype(np.float64)
    e = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    sums = {"kernel": out["sum"].cpu().numpy(), "torch": ref["sum"].cpu().numpy()}
    worst = {"kernel": 0.0, "torch": 0.0}
    for k in range(K):
        col = e[gap_np[:, k] == 0, k]
        f = math.fsum(col.tolist())
        for side in sums:
            worst[side] = max(worst[side], abs(sums[side][k] - f) / (len(col) * 2.0 ** -52 * f))
    pairs = N * K
    least = {"markers, kp and gap read once": 28 * pairs, "sqerr written once": 4 * pairs, "sqerr read twice": 8 * pairs}
    moved = {"markers, kp and gap read once": 28 * pairs, "sqerr written once": 4 * pairs, "keys written once": 4 * pairs,
             "keys read three times": 12 * pairs}
    total_least, total_moved = int(sum(least.values())), int(sum(moved.values()))
    rate = total_least / (k_time["ms_median"] * 1e-3)
    result = {"tool": "profiles/tools/report_bench.py", "command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
              "n_frames": N, "n_kp": K, "permille": list(permille), "gap_fraction": float((gap_np > 0).mean()),
              "tile_frames": report.TILE_FRAMES, "seg_frames": report.SEG_FRAMES, "max_blocks": report.MAX_BLOCKS, "workspace_bytes": nbytes,
              "timing": "device events around one call on preallocated buffers, after 3 warm-up calls",
              "bytes_moved_at_least": least | {"total": total_least}, "bytes_this_implementation_moves": moved | {"total": total_moved},
              "hbm_peak_bytes_per_s": {"spec": HBM_PEAK_SPEC, "measured float4 copy": HBM_PEAK_MEASURED},
              "stac_report_errors": k_time | {"bytes_per_s_of_the_least": rate, "fraction_of_hbm_peak_spec": rate / HBM_PEAK_SPEC,
                                              "fraction_of_hbm_peak_measured": rate / HBM_PEAK_MEASURED,
                                              "bytes_per_s_moved": total_moved / (k_time["ms_median"] * 1e-3)},
              "torch_report": t_time, "torch_over_kernel": t_time["ms_median"] / k_time["ms_median"], "bit_equal": equal,
              "sum_error_over_bound": worst, "sum_bound": "count * 2^-52 * fsum"}
    print(json.dumps({"kernel_ms": k_time["ms_median"], "torch_ms": t_time["ms_median"], "torch_over_kernel": result["torch_over_kernel"],
                      "fraction_of_hbm_peak_spec": rate / HBM_PEAK_SPEC, "bit_equal": equal, "sum_error_over_bound": worst}), flush=True)
    if not all(equal.values()) or max(worst.values()) > 1.0:
        raise SystemExit("report_bench: torch_report and stac_report_errors disagree")
    if args.bench_this or args.bench_parent:
        result["bench_py_default_line_frames_per_s"] = {
            "command": "python bench.py --gpus 1 --steps 3 --warmup 1 (the parent commit's library, then this tree's, three times alternating)",
            "parent_commit": [float(v) for v in args.bench_parent.split(",") if v], "this_tree": [float(v) for v in args.bench_this.split(",") if v]}
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1) + "\n")
        print(f"wrote {path}")


if __name__ == "__main__":
    main()
