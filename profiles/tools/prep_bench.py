"""``stac_prep_fill`` (stac.fill_missing) on one GPU against a straightforward torch implementation of the same rule
(DESIGN.md "Filling missing keypoints", profiles/prep/prep_bench.json).

  python profiles/tools/prep_bench.py --out profiles/prep/prep_bench.json [--frames 1000000] [--kp 23] [--reps 20]

The series is seeded noise around a slow drift; holes are punched per track in runs of geometric length (mean ``--mean-run``
frames) up to 0 %, 5 % and 50 % of the frames, and, in a fourth case, as one run of 100 000 frames per track.  Each side is
timed by device events around one call on preallocated buffers (the kernel side: the three launches of ``stac_prep_fill``; the
torch side: ``torch_fill`` below, ``cummax`` / ``cummin`` for p and n, index gathers for the two values), ``--reps`` times after
three warm-up calls.  The two outputs are compared bit for bit.  Bytes: what the staged scan has to move at least (the series read
in stages 1 and 3, ``out`` and ``gap`` written once, the tile summaries and carries written once and read once), over the
kernel time, against the HBM peak.  ``--bench-this`` / ``--bench-parent``: frames/s of ``bench.py``'s default line measured
elsewhere in the same session, recorded as given.
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT)]

HBM_PEAK_SPEC = 8.0e12       # bytes/s, MI355X data sheet
HBM_PEAK_MEASURED = 6.29e12  # bytes/s, a float4 copy kernel on this part


def holes(T, K, fraction, mean_run, rng):
    """[T, K] bool, True = missing: per track alternating valid / missing runs of geometric length"""
    miss = np.zeros((T, K), bool)
    if fraction <= 0:
        return miss
    mean_valid = mean_run * (1.0 - fraction) / fraction
    for k in range(K):
        n_seg = int(2.5 * T / (mean_run + mean_valid)) + 16
        lengths = np.empty(2 * n_seg, np.int64)
        lengths[0::2] = rng.geometric(1.0 / max(mean_valid, 1.0), n_seg)
        lengths[1::2] = rng.geometric(1.0 / mean_run, n_seg)
        state = np.repeat(np.tile(np.array([False, True]), n_seg), lengths)
        assert state.size >= T
        miss[:, k] = state[:T]
    return miss


def torch_fill(kp, mode):
    """The rule in plain torch: [T, 3K] -> (out, gap).  The double arithmetic is one op per torch call, so it rounds as the kernel's."""
    T, K = kp.shape[0], kp.shape[1] // 3
    x = kp.view(T, K, 3)
    valid = torch.isfinite(x).all(dim=2)
    idx = torch.arange(T, device=kp.device).unsqueeze(1).expand(T, K)
    p = torch.cummax(torch.where(valid, idx, -1), dim=0).values
    n = torch.flip(torch.cummin(torch.flip(torch.where(valid, idx, T), (0,)), dim=0).values, (0,))
    has_p, has_n = p >= 0, n < T
    a = torch.gather(x, 0, p.clamp(min=0).unsqueeze(2).expand(T, K, 3))
    b = torch.gather(x, 0, n.clamp(max=T - 1).unsqueeze(2).expand(T, K, 3))
    if mode == "linear":
        w = ((idx - p).double() / (n - p).clamp(min=1).double()).unsqueeze(2)
        ad = a.double()
        both = (ad + (b.double() - ad) * w).float()
    else:
        both = torch.where(((idx - p) <= (n - idx)).unsqueeze(2), a, b)
    fill = torch.where((has_p & has_n).unsqueeze(2), both, torch.where(has_p.unsqueeze(2), a, b))
    out = torch.where((valid | ~(has_p | has_n)).unsqueeze(2), x, fill).reshape(T, 3 * K)
    run = torch.where(has_p & has_n, n - p - 1, torch.where(has_n, n, torch.where(has_p, T - 1 - p, T)))
    gap = torch.where(valid, 0, run).to(torch.int32)
    return out, gap


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--kp", type=int, default=23)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mean-run", type=float, default=8.0)
    ap.add_argument("--bench-this", default="")
    ap.add_argument("--bench-parent", default="")
    args = ap.parse_args()

    from stac_mjx_amd import prep
    from stac_mjx_amd.engine import load_library

    if not torch.cuda.is_available():
        raise SystemExit("prep_bench needs a GPU: nothing is measured without one")
    lib = load_library()
    T, K = args.frames, args.kp
    rng = np.random.default_rng(5)
    base = (np.cumsum(rng.standard_normal((T, 3 * K)).astype(np.float32) * np.float32(1e-3), axis=0, dtype=np.float32)
            + rng.standard_normal((T, 3 * K)).astype(np.float32) * np.float32(1e-3))
    cases = [("0 % missing", holes(T, K, 0.0, args.mean_run, rng)), ("5 % missing, geometric runs", holes(T, K, 0.05, args.mean_run, rng)),
             ("50 % missing, geometric runs", holes(T, K, 0.5, args.mean_run, rng))]
    one = np.zeros((T, K), bool)
    if T >= 1_000_000:
        for k in range(K):
            lo = 50_000 + (800_000 // K) * k
            one[lo:lo + 100_000, k] = True
        cases.append(("one run of 100 000 frames per track", one))

    nbytes = prep.workspace_bytes(T, K)
    out = torch.empty((T, 3 * K), dtype=torch.float32, device="cuda")
    gap = torch.empty((T, K), dtype=torch.int32, device="cuda")
    work = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    series_bytes = T * 3 * K * 4
    moved = {"series read in stage 1 and in stage 3": 2 * series_bytes, "out written": series_bytes, "gap written": T * K * 4,
             "tile summaries and carries written once, read once": 2 * nbytes}
    total = int(sum(moved.values()))
    result = {"tool": "profiles/tools/prep_bench.py", "command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
              "n_frames": T, "n_kp": K, "tile_frames": prep.TILE_FRAMES, "max_blocks": prep.MAX_BLOCKS, "workspace_bytes": nbytes,
              "mean_run_frames": args.mean_run, "timing": "device events around one call on preallocated buffers, after 3 warm-up calls",
              "bytes_moved_at_least": moved | {"total": total}, "hbm_peak_bytes_per_s": {"spec": HBM_PEAK_SPEC, "measured float4 copy": HBM_PEAK_MEASURED},
              "note": "the gathers of the values at p and n of missing keypoints come on top of bytes_moved_at_least; a series of "
                      f"{series_bytes / 2**20:.0f} MiB is about the size of the 256 MiB last-level cache, so part of the second read may hit it",
              "cases": []}
    for name, miss in cases:
        kp_np = base.copy()
        kp_np.reshape(T, K, 3)[miss] = np.nan
        kp = torch.as_tensor(kp_np).cuda()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        entry = {"case": name, "missing_fraction": float(miss.mean()), "longest_run": None}
        for mode in ("linear", "hold"):
            def kernel():
                rc = lib.stac_prep_fill(C.c_void_p(kp.data_ptr()), T, K, prep.MODES[mode], C.c_void_p(out.data_ptr()), C.c_void_p(gap.data_ptr()),
                                        C.c_void_p(work.data_ptr()), nbytes, stream)
                assert rc == 0, lib.stac_last_error().decode()

            k_time = timed(kernel, args.reps)
            t_time = timed(lambda: torch_fill(kp, mode), max(args.reps // 4, 3))
            ref_out, ref_gap = torch_fill(kp, mode)
            same = bool(torch.equal(out.view(torch.int32), ref_out.view(torch.int32)) and torch.equal(gap, ref_gap))
            entry["longest_run"] = int(gap.max())
            rate = total / (k_time["ms_median"] * 1e-3)
            entry[mode] = {"stac_prep_fill": k_time | {"bytes_per_s": rate, "fraction_of_hbm_peak_spec": rate / HBM_PEAK_SPEC,
                                                       "fraction_of_hbm_peak_measured": rate / HBM_PEAK_MEASURED},
                           "torch_cummax_and_gathers": t_time, "torch_over_kernel": t_time["ms_median"] / k_time["ms_median"],
                           "outputs_bit_equal": same}
            del ref_out, ref_gap
            print(json.dumps({"case": name, "mode": mode, "kernel_ms": k_time["ms_median"], "torch_ms": t_time["ms_median"],
                              "fraction_of_hbm_peak_spec": rate / HBM_PEAK_SPEC, "bit_equal": same}), flush=True)
        result["cases"].append(entry)
        del kp
    if args.bench_this or args.bench_parent:
        result["bench_py_default_line_frames_per_s"] = {
            "command": "python bench.py --gpus 1 --steps 3 --warmup 1 (the parent commit's tree, then this tree, three times alternating)",
            "parent_commit": [float(v) for v in args.bench_parent.split(",") if v], "this_tree": [float(v) for v in args.bench_this.split(",") if v]}
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1) + "\n")
        print(f"wrote {path}")


if __name__ == "__main__":
    main()
