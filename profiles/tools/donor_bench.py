"""``stac_prep_donor`` (stac.fill_donors) on one GPU, and ``stac_prep_fill`` on the same series: the only way the gaps were closed
before (DESIGN.md "Filling gaps from donor keypoints", profiles/prep/donor_bench.json).

  python profiles/tools/donor_bench.py --out profiles/prep/donor_bench.json [--frames 1000000] [--kp 23] [--triples 4] [--reps 20]

The series and the hole patterns are those of ``prep_bench.py`` (seeded noise around a slow drift; holes per track in runs of
geometric length up to 0 %, 5 % and 50 % of the frames, and one run of 100 000 frames per track).  The donor table names, in row d of
keypoint k, the three keypoints that follow k + d cyclically: every row is a triple, and which keypoints a row names does not change
what the kernel does per missing keypoint.  Each entry point is timed by device events around one call on preallocated buffers,
``--reps`` times after three warm-up calls.  Bytes: what the call has to move at least (the series read by the summary launch and
again by the fill launch, ``out``, ``gap`` and ``src`` written once, the tile summaries and carries written once and read once);
the donors' and the keypoint's own values at p and n, and the second read of the tile by the walk, come on top.
``--bench-this`` / ``--bench-parent``: frames/s of ``bench.py``'s default line measured elsewhere in the same session, recorded as
given.
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
sys.path[:0] = [str(ROOT), str(Path(__file__).resolve().parent)]

from prep_bench import HBM_PEAK_MEASURED, HBM_PEAK_SPEC, holes, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--kp", type=int, default=23)
    ap.add_argument("--triples", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mean-run", type=float, default=8.0)
    ap.add_argument("--bench-this", default="")
    ap.add_argument("--bench-parent", default="")
    args = ap.parse_args()

    from stac_mjx_amd import prep
    from stac_mjx_amd.engine import load_library

    if not torch.cuda.is_available():
        raise SystemExit("donor_bench needs a GPU: nothing is measured without one")
    lib = load_library()
    T, K, D = args.frames, args.kp, args.triples
    rng = np.random.default_rng(5)
    base = (np.cumsum(rng.standard_normal((T, 3 * K)).astype(np.float32) * np.float32(1e-3), axis=0, dtype=np.float32)
            + rng.standard_normal((T, 3 * K)).astype(np.float32) * np.float32(1e-3))
    cases = [("0 % missing", holes(T, K, 0.0, args.mean_run, rng)), ("5 % missing, geometric runs", holes(T, K, 0.05, args.mean_run, rng)),
             ("50 % missing, geometric runs", holes(T, K, 0.5, args.mean_run, rng))]
    if T >= 1_000_000:
        one = np.zeros((T, K), bool)
        for k in range(K):
            lo = 50_000 + (800_000 // K) * k
            one[lo:lo + 100_000, k] = True
        cases.append(("one run of 100 000 frames per track", one))
    table = np.array([[[(k + d + 1 + i) % K for i in range(3)] for d in range(D)] for k in range(K)], np.int32)

    nbytes = prep.donor_workspace_bytes(T, K)
    assert nbytes == prep.workspace_bytes(T, K)
    don = torch.as_tensor(table).cuda()
    out = torch.empty((T, 3 * K), dtype=torch.float32, device="cuda")
    gap = torch.empty((T, K), dtype=torch.int32, device="cuda")
    src = torch.empty((T, K), dtype=torch.uint8, device="cuda")
    fill_gap = torch.empty((T, K), dtype=torch.int32, device="cuda")
    work = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    series_bytes = T * 3 * K * 4
    moved = {"series read by the summary launch and by the fill launch": 2 * series_bytes, "out written": series_bytes, "gap written": T * K * 4,
             "src written": T * K, "tile summaries and carries written once, read once": 2 * nbytes}
    total = int(sum(moved.values()))
    result = {"tool": "profiles/tools/donor_bench.py", "command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
              "n_frames": T, "n_kp": K, "n_triples": D, "tile_frames": prep.TILE_FRAMES, "max_blocks": prep.MAX_BLOCKS, "workspace_bytes": nbytes,
              "mean_run_frames": args.mean_run, "timing": "device events around one call on preallocated buffers, after 3 warm-up calls",
              "bytes_moved_at_least": moved | {"total": total}, "hbm_peak_bytes_per_s": {"spec": HBM_PEAK_SPEC, "measured float4 copy": HBM_PEAK_MEASURED},
              "note": "the values of the keypoint and of its donors at p and n, and the walk's second read of the tile, come on top of "
                      "bytes_moved_at_least", "cases": []}
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for name, miss in cases:
        kp_np = base.copy()
        kp_np.reshape(T, K, 3)[miss] = np.nan
        kp = torch.as_tensor(kp_np).cuda()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def donor():
            rc = lib.stac_prep_donor(p(kp), T, K, p(don), D, p(out), p(gap), p(src), p(work), nbytes, stream)
            assert rc == 0, lib.stac_last_error().decode()

        def fill():
            rc = lib.stac_prep_fill(p(kp), T, K, prep.MODES["linear"], p(out), p(fill_gap), p(work), nbytes, stream)
            assert rc == 0, lib.stac_last_error().decode()

        f_time = timed(fill, args.reps)
        d_time = timed(donor, args.reps)
        torch.cuda.synchronize()
        counts = torch.bincount(src.reshape(-1).to(torch.int64), minlength=256).cpu().numpy()
        rate = total / (d_time["ms_median"] * 1e-3)
        entry = {"case": name, "missing_fraction": float(miss.mean()), "longest_run": int(gap.max()),
                 "gap_equals_stac_prep_fill": bool(torch.equal(gap, fill_gap)),
                 "filled_by_triple": {str(d + 1): int(counts[d + 1]) for d in range(D)}, "left_missing": int(counts[255]),
                 "stac_prep_donor": d_time | {"bytes_per_s": rate, "fraction_of_hbm_peak_spec": rate / HBM_PEAK_SPEC,
                                              "fraction_of_hbm_peak_measured": rate / HBM_PEAK_MEASURED},
                 "stac_prep_fill_linear": f_time, "donor_over_fill": d_time["ms_median"] / f_time["ms_median"]}
        result["cases"].append(entry)
        print(json.dumps({"case": name, "donor_ms": d_time["ms_median"], "fill_ms": f_time["ms_median"], "donor_over_fill": entry["donor_over_fill"],
                          "fraction_of_hbm_peak_spec": rate / HBM_PEAK_SPEC, "gap_equal": entry["gap_equals_stac_prep_fill"]}), flush=True)
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
