"""``stac_prep_swaps`` (stac.repair_swaps) on one GPU against the same rule in plain torch (DESIGN.md "Repairing keypoint swaps",
profiles/prep/swaps_bench.json).

  python profiles/tools/swaps_bench.py --out profiles/prep/swaps_bench.json [--frames 1000000] [--kp 23] [--cand 9] [--reps 10]

The series is that of pairwise_bench.py (a rigid shape of ``--kp`` points that drifts, seeded noise of 1 mm per keypoint) with
``--cand`` candidates (0, 1), (2, 3), ...; 1 % of the (frame, candidate)s are exchanged and 2 % of the (frame, keypoint)s are missing.
``n_sigma`` = 6, ``min_dev`` = 0.002, ``min_bad`` = 3 (the defaults of the config keys).  Each side is timed by device events around
ONE call on preallocated buffers (the kernel side: the two memsets and 14 launches of ``stac_prep_swaps``; the torch side:
``torch_swaps`` below -- per pair a float32 distance, two ``sort``s and gathers, then per candidate the counts as tensor operations
over all frames), ``--reps`` times after two warm-up calls (torch: ``--torch-reps`` after one).  For comparison ``stac_prep_pairwise``
is timed the same way on the same series.  The five outputs are compared bit for bit and the result is written down, not asserted.
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

from pairwise_bench import HBM_PEAK_MEASURED, HBM_PEAK_SPEC, timed  # noqa: E402


def torch_swaps(kp, cand, thr, min_dev, min_bad):
    """The rule in plain torch: [T, 3K] -> (out, flag, pair_n, pair_med, pair_mad).  Every float32 / double operation is one torch
    call, so it rounds as the kernels'."""
    T, K = kp.shape[0], kp.shape[1] // 3
    dev = kp.device
    x = kp.view(T, K, 3)
    present = torch.isfinite(x).all(dim=2)
    P = K * (K - 1) // 2
    pair_n = torch.zeros(P, dtype=torch.int64, device=dev)
    pair_med = torch.full((P,), float("nan"), dtype=torch.float64, device=dev)
    pair_mad = torch.full((P,), float("nan"), dtype=torch.float64, device=dev)
    dist = torch.empty((P, T), dtype=torch.float32, device=dev)
    ok = torch.zeros((P, T), dtype=torch.bool, device=dev)  # valid in the frame, and n >= 3
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=dev)
    index = {}
    p = 0
    for a in range(K - 1):
        for b in range(a + 1, K):
            index[(a, b)] = index[(b, a)] = p
            dx, dy, dz = x[:, a, 0] - x[:, b, 0], x[:, a, 1] - x[:, b, 1], x[:, a, 2] - x[:, b, 2]
            d = torch.sqrt((dx * dx + dy * dy) + dz * dz)
            valid = present[:, a] & present[:, b] & torch.isfinite(d)
            n = int(valid.sum())
            pair_n[p] = n
            dist[p] = d
            if n >= 3:
                r = torch.tensor([(n - 1) // 2, n // 2], device=dev)
                s = torch.sort(torch.where(valid, d, inf)).values[r].double()
                med = (s[0] + s[1]) * 0.5
                e = (d.double() - med).abs().float()
                E = torch.sort(torch.where(valid, e, inf)).values[r].double()
                mad = (E[0] + E[1]) * 0.5
                pair_med[p], pair_mad[p] = med, mad
                ok[p] = valid
            p += 1
    bound = pair_mad * thr

    def bad(d, q):
        e = (d.double() - pair_med[q]).abs().float().double()
        return (e > bound[q]) & (e > min_dev)

    flag = torch.zeros((T, len(cand)), dtype=torch.uint8, device=dev)
    for s, (a, b) in enumerate(cand):
        b0 = torch.zeros(T, dtype=torch.int32, device=dev)
        b1 = torch.zeros(T, dtype=torch.int32, device=dev)
        for k in range(K):
            if k in (a, b):
                continue
            pa, pb = index[(a, k)], index[(b, k)]
            counts = ok[pa] & ok[pb]
            da, db = dist[pa], dist[pb]
            b0 += (bad(da, pa) & counts).int() + (bad(db, pb) & counts).int()
            b1 += (bad(db, pa) & counts).int() + (bad(da, pb) & counts).int()
        flag[:, s] = ((b0 >= min_bad) & (2 * b1 <= b0)).to(torch.uint8)
    out = x.clone()
    for s, (a, b) in enumerate(cand):
        rows = flag[:, s] == 1
        out[rows, a] = x[rows, b]
        out[rows, b] = x[rows, a]
    return out.reshape(T, 3 * K), flag, pair_n, pair_med, pair_mad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--kp", type=int, default=23)
    ap.add_argument("--cand", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--bench-this", default="")
    ap.add_argument("--bench-parent", default="")
    args = ap.parse_args()

    from stac_mjx_amd import prep
    from stac_mjx_amd.engine import load_library

    if not torch.cuda.is_available():
        raise SystemExit("swaps_bench needs a GPU: nothing is measured without one")
    lib = load_library()
    T, K, S = args.frames, args.kp, args.cand
    P = K * (K - 1) // 2
    cand = prep.swaps_pairs([(2 * i, 2 * i + 1) for i in range(S)], K)
    rng = np.random.default_rng(15)
    shape = rng.uniform(-0.15, 0.15, (1, K, 3)).astype(np.float32)
    drift = np.cumsum(rng.standard_normal((T, 1, 3)).astype(np.float32) * np.float32(1e-3), axis=0, dtype=np.float32)
    x = shape + drift + rng.standard_normal((T, K, 3)).astype(np.float32) * np.float32(1e-3)
    hit = rng.random((T, S)) < 0.01
    for s, (a, b) in enumerate(cand):
        rows = np.flatnonzero(hit[:, s])
        x[rows[:, None], [a, b]] = x[rows[:, None], [b, a]]
    x[rng.random((T, K)) < 0.02] = np.nan
    present = np.isfinite(x).all(axis=2)
    both = np.stack([present[:, a] & present[:, b] for a, b in cand], axis=1)
    kp = torch.as_tensor(np.ascontiguousarray(x.reshape(T, 3 * K))).cuda()
    del x, drift
    thr, min_dev, min_bad = prep.swaps_params(6.0, 0.002, 3)

    out = torch.empty((T, 3 * K), dtype=torch.float32, device="cuda")
    flag = torch.empty((T, max(S, 1)), dtype=torch.uint8, device="cuda")
    flag_k = torch.empty((T, K), dtype=torch.uint8, device="cuda")
    pair_n = torch.empty(max(P, 1), dtype=torch.int64, device="cuda")
    pair_med = torch.empty(max(P, 1), dtype=torch.float64, device="cuda")
    pair_mad = torch.empty(max(P, 1), dtype=torch.float64, device="cuda")
    nbytes = prep.swaps_workspace_bytes(T, K)
    work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = (C.c_int32 * max(2 * S, 1))(*[v for ab in cand for v in ab])
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def pairwise():
        rc = lib.stac_prep_pairwise(p(kp), T, K, thr, min_dev, 2, p(out), p(flag_k), p(pair_n), p(pair_med), p(pair_mad), p(work), nbytes, stream)
        assert rc == 0, lib.stac_last_error().decode()

    def kernel():
        rc = lib.stac_prep_swaps(p(kp), T, K, table, S, thr, min_dev, min_bad, p(out), p(flag), p(pair_n), p(pair_med), p(pair_mad), p(work),
                                 nbytes, stream)
        assert rc == 0, lib.stac_last_error().decode()

    p_time = timed(pairwise, args.reps)
    k_time = timed(kernel, args.reps)
    t_time = timed(lambda: torch_swaps(kp, cand, thr, min_dev, min_bad), args.torch_reps, warm=1)
    ref = torch_swaps(kp, cand, thr, min_dev, min_bad)
    got = (out, flag[:, :S], pair_n[:P], pair_med[:P], pair_mad[:P])
    as_bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else (t.view(torch.int32) if t.dtype == torch.float32 else t)  # noqa: E731
    equal = {name: bool(torch.equal(as_bits(g), as_bits(r))) for name, g, r in zip(("out", "flag", "pair_n", "pair_med", "pair_mad"), got, ref)}
    found = flag[:, :S].cpu().numpy() == 1
    series_bytes, keys_bytes = T * 3 * K * 4, P * T * 4
    moved = {"series read twice (distances, then the copy to out)": 2 * series_bytes, "keys written once": keys_bytes,
             "keys read six times by the counting passes": 6 * keys_bytes,
             "key reads of the decision (2 (K - 2) per candidate and frame)": S * 2 * (K - 2) * T * 4, "out written": series_bytes,
             "flag written": T * S}
    total = int(sum(moved.values()))
    rate = total / (k_time["ms_median"] * 1e-3)
    result = {"tool": "profiles/tools/swaps_bench.py", "command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
              "n_frames": T, "n_kp": K, "n_pairs": P, "n_cand": S, "n_sigma": 6.0, "thr": thr, "min_dev": min_dev, "min_bad": min_bad,
              "workspace_bytes": nbytes, "swapped_fraction": float(hit.mean()), "missing_fraction": float(1.0 - present.mean()),
              "swaps_with_both_keypoints_present": int((hit & both).sum()), "of_those_flagged": int((found & hit & both).sum()),
              "flagged_without_a_swap": int((found & ~hit).sum()),
              "timing": "device events around one call on preallocated buffers, after 2 warm-up calls (torch: 1)",
              "bytes_moved_at_least": moved | {"total": total}, "hbm_peak_bytes_per_s": {"spec": HBM_PEAK_SPEC, "measured float4 copy": HBM_PEAK_MEASURED},
              "stac_prep_swaps": k_time | {"bytes_per_s": rate, "fraction_of_hbm_peak_spec": rate / HBM_PEAK_SPEC,
                                           "fraction_of_hbm_peak_measured": rate / HBM_PEAK_MEASURED},
              "stac_prep_pairwise_same_series": p_time, "torch_sort_per_pair": t_time,
              "torch_over_kernel": t_time["ms_median"] / k_time["ms_median"], "bit_equal_to_torch": equal}
    print(json.dumps({"kernel_ms": k_time["ms_median"], "pairwise_ms": p_time["ms_median"], "torch_ms": t_time["ms_median"],
                      "torch_over_kernel": result["torch_over_kernel"], "of_those_flagged": result["of_those_flagged"],
                      "swaps_present": result["swaps_with_both_keypoints_present"], "false": result["flagged_without_a_swap"],
                      "bit_equal_to_torch": equal}), flush=True)
    if args.bench_this or args.bench_parent:
        result["bench_py_default_line_frames_per_s"] = {
            "command": "python bench.py --gpus 1 --steps 3 --warmup 1 (the parent commit's tree and library, then this tree's, three times alternating)",
            "parent_commit": [float(v) for v in args.bench_parent.split(",") if v], "this_tree": [float(v) for v in args.bench_this.split(",") if v]}
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1) + "\n")
        print(f"wrote {path}")


if __name__ == "__main__":
    main()
