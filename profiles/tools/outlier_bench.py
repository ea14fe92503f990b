"""``stac_prep_reject`` (stac.reject_outliers) on one GPU against a straightforward torch implementation of the same rule
(DESIGN.md "Rejecting keypoint outliers", profiles/prep/outlier_bench.json).

  python profiles/tools/outlier_bench.py --out profiles/prep/outlier_bench.json [--frames 1000000] [--kp 23] [--reps 20]

The series is seeded noise around a slow drift (that of prep_bench.py); spikes of 5 cm in one coordinate are added to 0 % and 5 %
of the (frame, keypoint) pairs.  Half-widths 2, 5 and 16, ``n_sigma`` = 3, ``min_dev`` = 0.001 (the defaults of the config keys;
``--min-dev`` changes it), and the kernel a second time with ``min_dev`` = 0, where no coordinate is decided before its deviations
are ranked.  Each side is timed by device events around one call on preallocated buffers (the kernel side: the one launch of
``stac_prep_reject``; the torch side: ``torch_reject`` below -- ``unfold`` windows, two ``sort``s, gathers -- in slabs of
``--slab`` frames so that its window tensors fit), ``--reps`` times after three warm-up calls.  ``flag`` and ``out`` are compared
bit for bit.  Bytes: what has to move at least (the series read once, ``out`` and ``flag`` written once) over the kernel time,
against the HBM peak.  ``--bench-this`` / ``--bench-parent``: frames/s of ``bench.py``'s default line measured elsewhere in the same
session, recorded as given.
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


def torch_reject(kp, h, thr, min_dev, slab):
    """The rule in plain torch: [T, 3K] -> (out, flag).  Every double operation is one torch call, so it rounds as the kernel's."""
    T, K = kp.shape[0], kp.shape[1] // 3
    W = 2 * h + 1
    x = kp.view(T, K, 3)
    nan = torch.tensor(float("nan"), dtype=torch.float32, device=kp.device)
    s = torch.where(torch.isfinite(x).all(dim=2, keepdim=True), x, nan).reshape(T, 3 * K)  # sanitized: a missing keypoint is three NaN
    s = torch.cat([nan.expand(h, 3 * K), s, nan.expand(h, 3 * K)], dim=0)                 # and so is every frame outside the series
    flag = torch.empty((T, K), dtype=torch.uint8, device=kp.device)
    for lo in range(0, T, slab):
        hi = min(lo + slab, T)
        w = s[lo:hi + 2 * h].unfold(0, W, 1)  # [rows, 3K, W]
        n = (w == w).sum(dim=2, keepdim=True)
        r0, r1 = ((n - 1) // 2).clamp(min=0), n // 2
        srt = torch.sort(w, dim=2).values  # (NaN sorts last)
        med = (srt.gather(2, r0).double() + srt.gather(2, r1).double()) * 0.5
        d = (w.double() - med).abs()
        dsrt = torch.sort(d, dim=2).values
        mad = (dsrt.gather(2, r0) + dsrt.gather(2, r1)) * 0.5
        dc = d[:, :, h:h + 1]
        outlier = (n >= 3) & (dc > mad * thr) & (dc > min_dev)  # (a missing centre has dc = NaN: false)
        flag[lo:hi] = outlier.view(hi - lo, K, 3).any(dim=2).to(torch.uint8)
    out = torch.where((flag == 1).unsqueeze(2), nan, x).reshape(T, 3 * K)
    return out, flag


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
    ap.add_argument("--min-dev", type=float, default=0.001)
    ap.add_argument("--slab", type=int, default=100_000)
    ap.add_argument("--bench-this", default="")
    ap.add_argument("--bench-parent", default="")
    args = ap.parse_args()

    from stac_mjx_amd import prep
    from stac_mjx_amd.engine import load_library

    if not torch.cuda.is_available():
        raise SystemExit("outlier_bench needs a GPU: nothing is measured without one")
    lib = load_library()
    T, K = args.frames, args.kp
    rng = np.random.default_rng(5)
    base = (np.cumsum(rng.standard_normal((T, 3 * K)).astype(np.float32) * np.float32(1e-3), axis=0, dtype=np.float32)
            + rng.standard_normal((T, 3 * K)).astype(np.float32) * np.float32(1e-3))
    _, thr, min_dev = prep.outlier_params(5, 3.0, args.min_dev)

    out = torch.empty((T, 3 * K), dtype=torch.float32, device="cuda")
    flag = torch.empty((T, K), dtype=torch.uint8, device="cuda")
    series_bytes = T * 3 * K * 4
    moved = {"series read once": series_bytes, "out written": series_bytes, "flag written": T * K}
    total = int(sum(moved.values()))
    result = {"tool": "profiles/tools/outlier_bench.py", "command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
              "n_frames": T, "n_kp": K, "tile_frames": prep.TILE_FRAMES, "max_blocks": prep.MAX_BLOCKS, "n_sigma": 3.0, "thr": thr,
              "min_dev": min_dev, "timing": "device events around one call on preallocated buffers, after 3 warm-up calls",
              "bytes_moved_at_least": moved | {"total": total}, "hbm_peak_bytes_per_s": {"spec": HBM_PEAK_SPEC, "measured float4 copy": HBM_PEAK_MEASURED},
              "note": "the halo rows of a tile (2 h of 64 + 2 h) are read a second time, mostly from cache; the kernel is bound by the rank "
                      "counting over LDS, not by these bytes", "torch_slab_frames": args.slab, "cases": []}
    for fraction in (0.0, 0.05):
        kp_np = base.copy()
        hit = rng.random((T, K)) < fraction
        t_idx, k_idx = np.nonzero(hit)
        kp_np[t_idx, 3 * k_idx + rng.integers(0, 3, t_idx.size)] += np.float32(0.05)
        kp = torch.as_tensor(kp_np).cuda()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for h in (2, 5, 16):
            def kernel(floor=min_dev):
                rc = lib.stac_prep_reject(C.c_void_p(kp.data_ptr()), T, K, h, thr, floor, C.c_void_p(out.data_ptr()), C.c_void_p(flag.data_ptr()), stream)
                assert rc == 0, lib.stac_last_error().decode()

            k0_time = timed(lambda: kernel(0.0), args.reps)
            k_time = timed(kernel, args.reps)  # (last: out and flag hold its results below)
            t_time = timed(lambda: torch_reject(kp, h, thr, min_dev, args.slab), max(args.reps // 4, 3))
            ref_out, ref_flag = torch_reject(kp, h, thr, min_dev, args.slab)
            same_flag = bool(torch.equal(flag, ref_flag))
            same_out = bool(torch.equal(out.view(torch.int32), ref_out.view(torch.int32)))
            rate = total / (k_time["ms_median"] * 1e-3)
            entry = {"spiked_fraction": float(hit.mean()), "half_window": h, "rejected_fraction": float(flag.float().mean()),
                     "stac_prep_reject": k_time | {"bytes_per_s": rate, "fraction_of_hbm_peak_spec": rate / HBM_PEAK_SPEC,
                                                   "fraction_of_hbm_peak_measured": rate / HBM_PEAK_MEASURED},
                     "stac_prep_reject_min_dev_0": k0_time, "torch_unfold_sort_gather": t_time,
                     "torch_over_kernel": t_time["ms_median"] / k_time["ms_median"], "flag_bit_equal": same_flag, "out_bit_equal": same_out}
            del ref_out, ref_flag
            result["cases"].append(entry)
            print(json.dumps({"spiked": fraction, "h": h, "kernel_ms": k_time["ms_median"], "kernel_ms_min_dev_0": k0_time["ms_median"],
                              "torch_ms": t_time["ms_median"], "fraction_of_hbm_peak_spec": rate / HBM_PEAK_SPEC,
                              "rejected": entry["rejected_fraction"], "flag_bit_equal": same_flag, "out_bit_equal": same_out}), flush=True)
        del kp
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
