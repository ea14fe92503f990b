"""``stac.resample`` on one GPU: the kernel's time, its traffic against the HBM peak, its cost per output element and tap next to
``stac_post_smooth``'s on the same rows, and ``scipy.signal.resample_poly`` on the host for the same array (DESIGN.md "Resampling
fitted poses", profiles/post/resample_bench.json).

  python profiles/tools/resample_bench.py --out profiles/post/resample_bench.json [--parent-lib PATH/libstac_hip.so]
        [--parent-tree PATH]

Kernel: rodent rows (nq = 74, the free joint's quaternion at column 3, bounds) of 100 000 and 1 000 000 frames as one clip, 300 -> 50
and 120 -> 50 Hz with ten lobes.  Per shape one warm-up of ``--reps`` launches, then ``--turns`` turns of ``--reps`` launches of
``stac_post_resample`` on a destination allocated once, each turn between two device events; median, minimum and maximum over the
turns.  Bytes moved: one read of the input and one write of the output; the read amplification of the tile the host picks is stated
beside it.  The random input is a stand-in: the kernel's time does not depend on the values.

Smooth: ``stac_post_smooth`` on the same rows in the same session, half-widths 3 and 16, timed the same way; with ``--parent-lib``
through that library (the parent commit's), else through this tree's.  Its cost per output element and tap stands beside resample's.

Host: the wall time of ``scipy.signal.resample_poly(x, U, D, axis=0, window=("kaiser", 5.0), padtype="edge")`` on the same array,
the better of two calls (left out where scipy is missing).

``--parent-tree``: the default line of ``bench.py`` (``--gpus 1 --steps 3 --warmup 1``) as child processes, this tree and a built
checkout of the parent commit alternating, three runs each.  Every GPU step of a child process runs under ``timeout``.
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT)]

HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X, HBM3E (6.29e12 measured by a float4 copy)
NQ, QUAT = 74, [3]
ROWS = (100_000, 1_000_000)
RATES = ((300, 50), (120, 50))
SMOOTH_HALF = (3, 16)


def _timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def _measure(fn, reps, turns):
    _timed(fn, reps)
    t = [_timed(fn, reps) for _ in range(turns)]
    return {"median": float(np.median(t)), "min_max": [min(t), max(t)]}


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def kernel_section(reps, turns, parent_lib):
    from stac_mjx_amd import abi, post
    from stac_mjx_amd.engine import load_library

    lib = load_library()
    slib, smooth_from = lib, "this tree's library"
    if parent_lib:  # (only the one function is declared: the parent's library does not have this tree's newest ones)
        slib = C.CDLL(str(Path(parent_lib).resolve()))
        slib.stac_post_smooth.restype, slib.stac_post_smooth.argtypes = abi.PROTOTYPES["stac_post_smooth"]
        smooth_from = "the parent commit's library"
    out = []
    cols = np.asarray(QUAT, dtype=np.int32)
    colp = cols.ctypes.data_as(C.POINTER(C.c_int32))
    for N in ROWS:
        g = torch.Generator(device="cuda").manual_seed(1)
        q = torch.randn((N, NQ), device="cuda", generator=g)
        q[:, 3:7] /= q[:, 3:7].norm(dim=1, keepdim=True)
        lb, ub = torch.full((NQ,), -3.0, device="cuda"), torch.full((NQ,), 3.0, device="cuda")
        stream = abi.stream_ptr(q.device)
        smooth = {}
        for H in SMOOTH_HALF:
            taps = post.smooth_taps("savgol", H)
            dst = torch.empty_like(q)

            def run_smooth():
                rc = slib.stac_post_smooth(_ptr(q), N, NQ, N, H, taps.ctypes.data_as(C.POINTER(C.c_float)), colp, 1, _ptr(lb), _ptr(ub), _ptr(dst), stream)
                assert rc == 0, rc

            t = _measure(run_smooth, reps, turns)
            smooth[H] = dict(t, window=2 * H + 1, ns_per_output_element_and_tap=t["median"] / (N * NQ * (2 * H + 1)) * 1e9,
                             GB_per_s=2 * N * NQ * 4 / t["median"] * 1e-9)
            del dst
        for from_hz, to_hz in RATES:
            U, D = post.resample_ratio(from_hz, to_hz)
            taps = post.resample_taps(U, D, lobes=10)
            W = taps.shape[1]
            taps_dev = torch.as_tensor(taps).cuda()
            No = post.resample_rows(N, U, D)
            dst = torch.empty((No, NQ), device="cuda")
            T = post.resample_tile_rows(NQ, U, D, W)

            def run_resample():
                rc = lib.stac_post_resample(_ptr(q), N, NQ, N, U, D, (W // 2 - 1) * U, _ptr(taps_dev), colp, 1, _ptr(lb), _ptr(ub), _ptr(dst), No, stream)
                assert rc == 0, rc

            t = _measure(run_resample, reps, turns)
            nbytes = (N + No) * NQ * 4
            entry = {"rows_in": N, "rows_out": No, "nq": NQ, "from_hz": from_hz, "to_hz": to_hz, "up": U, "down": D, "lobes": 10, "taps": W,
                     "band_cols": post.resample_band_cols(NQ), "tile_outputs": T,
                     "read_amplification_of_the_tile": (((T - 1) * D) // U + W) / (T * D / U),
                     "launches_per_turn": reps, "turns": turns, "kernel_s": t, "bytes_read_plus_written": nbytes,
                     "GB_per_s": nbytes / t["median"] * 1e-9, "share_of_hbm_peak": nbytes / t["median"] / HBM_PEAK_BYTES_PER_S,
                     "ns_per_output_element_and_tap": t["median"] / (No * NQ * W) * 1e9,
                     "smooth_on_the_same_rows": {"library": smooth_from, **{f"half_window_{H}": smooth[H] for H in SMOOTH_HALF}}}
            try:
                from scipy.signal import resample_poly

                x = q.cpu().numpy()
                walls = []
                for _ in range(2):
                    t0 = time.perf_counter()
                    y = resample_poly(x, U, D, axis=0, window=("kaiser", 5.0), padtype="edge")
                    walls.append(time.perf_counter() - t0)
                entry["scipy_resample_poly_host_s"] = {"best_of_2": min(walls), "rows_out": int(y.shape[0])}
                del x, y
            except ImportError:
                entry["scipy_resample_poly_host_s"] = None
            out.append(entry)
            print(json.dumps({k: entry[k] for k in ("rows_in", "up", "down", "taps", "tile_outputs", "kernel_s", "GB_per_s", "share_of_hbm_peak",
                                                    "ns_per_output_element_and_tap", "scipy_resample_poly_host_s")}), flush=True)
            print(json.dumps({f"smooth H={H}": smooth[H]["ns_per_output_element_and_tap"] for H in SMOOTH_HALF}), flush=True)
            del dst
        del q
    return out


def regression_section(parent_tree, runs=3, limit_s=240):
    """``bench.py``'s default line in child processes: this tree and the built checkout ``parent_tree`` alternating."""
    trees = {"this_tree": ROOT, "parent_commit": Path(parent_tree).resolve()}
    lines, order = {k: [] for k in trees}, []
    for i in range(runs):
        for name in (("this_tree", "parent_commit") if i % 2 == 0 else ("parent_commit", "this_tree")):
            cmd = ["timeout", "-k", "10", str(limit_s), sys.executable, str(trees[name] / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"]
            res = subprocess.run(cmd, capture_output=True, text=True, cwd=trees[name])
            if res.returncode != 0:  # a failed or timed-out GPU step ends the measurement: nothing more is started on the device
                raise SystemExit(f"bench.py of {name} ended with status {res.returncode}:\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
            line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
            lines[name].append(line)
            order.append(name)
            print(name, json.dumps(line), flush=True)
    return {"command": "python bench.py --gpus 1 --steps 3 --warmup 1 (this tree and a checkout of the parent commit, alternating)", "order": order,
            "result_lines": lines}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10, help="kernel launches between two events")
    ap.add_argument("--turns", type=int, default=7, help="timed turns per kernel and shape")
    ap.add_argument("--parent-lib", default=None, help="a libstac_hip.so built from the parent commit: stac_post_smooth is timed through it")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: adds the bench.py comparison")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs a GPU: nothing is measured without one")
    result = {"tool": "profiles/tools/resample_bench.py", "command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
              "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "kernel": kernel_section(args.reps, args.turns, args.parent_lib)}
    if args.parent_tree:
        torch.cuda.synchronize()
        result["bench_default_line"] = regression_section(args.parent_tree)
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(result, indent=1) + "\n")
        print(f"wrote {out}")


if __name__ == "__main__":
    main()
