"""``stac_prep_pairwise`` (stac.reject_pairwise) on one GPU against the same rule in plain torch (DESIGN.md "Rejecting keypoints by
pairwise distances", profiles/prep/pairwise_bench.json).

  python profiles/tools/pairwise_bench.py --out profiles/prep/pairwise_bench.json [--frames 1000000] [--kp 23] [--reps 10]

The series is a rigid shape of ``--kp`` points that drifts, with seeded noise of 1 mm per keypoint; 1 % of the (frame, keypoint)
pairs are displaced by about 10 cm and 2 % are missing.  ``n_sigma`` = 6, ``min_dev`` = 0.002, ``votes`` = 2 (the defaults of the
config keys).  Each side is timed by device events around ONE call on preallocated buffers (the kernel side: the two memsets and 14
launches of ``stac_prep_pairwise``; the torch side: ``torch_pairwise`` below -- per pair a float32 distance, two ``sort``s and
gathers, then the blame as tensor operations over slabs of ``--slab`` frames), ``--reps`` times after two warm-up calls (torch:
``--torch-reps``).  The five outputs are compared bit for bit and the result is written down, not asserted.  Bytes: what has to move
at least (the series read twice, the keys written once and read seven times -- six counting passes and the decision --, ``out`` and
``flag`` written once) over the kernel time, against the HBM peak.  ``--bench-this`` / ``--bench-parent``: frames/s of ``bench.py``'s
default line measured elsewhere in the same session, recorded as given.
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


def torch_pairwise(kp, thr, min_dev, votes, slab):
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
    bad = torch.zeros((T, K, K), dtype=torch.bool, device=dev)
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=dev)
    p = 0
    for a in range(K - 1):
        for b in range(a + 1, K):
            dx, dy, dz = x[:, a, 0] - x[:, b, 0], x[:, a, 1] - x[:, b, 1], x[:, a, 2] - x[:, b, 2]
            d = torch.sqrt((dx * dx + dy * dy) + dz * dz)
            valid = present[:, a] & present[:, b] & torch.isfinite(d)
            n = int(valid.sum())
            pair_n[p] = n
            if n >= 3:
                r = torch.tensor([(n - 1) // 2, n // 2], device=dev)
                s = torch.sort(torch.where(valid, d, inf)).values[r].double()
                med = (s[0] + s[1]) * 0.5
                e = (d.double() - med).abs().float()
                E = torch.sort(torch.where(valid, e, inf)).values[r].double()
                mad = (E[0] + E[1]) * 0.5
                e64 = e.double()
                is_bad = valid & (e64 > mad * thr) & (e64 > min_dev)
                bad[:, a, b] = is_bad
                bad[:, b, a] = is_bad
                pair_med[p], pair_mad[p] = med, mad
            p += 1
    flag = torch.zeros((T, K), dtype=torch.uint8, device=dev)
    lowest_first = torch.arange(K - 1, -1, -1, device=dev)  # (a tie of c_k goes to the lowest k)
    for lo in range(0, T, slab):
        B = bad[lo:lo + slab]
        f = flag[lo:lo + slab]
        while True:
            c = B.sum(dim=2)
            best = (c * K + lowest_first).max(dim=1)
            go = (best.values // K) >= votes
            if not bool(go.any()):
                break
            rows = torch.nonzero(go).reshape(-1)
            k = best.indices[rows]
            f[rows, k] = 1
            B[rows, k, :] = False
            B[rows, :, k] = False
    nan = torch.tensor(float("nan"), dtype=torch.float32, device=dev)
    out = torch.where((flag == 1).unsqueeze(2), nan, x).reshape(T, 3 * K)
    return out, flag, pair_n, pair_med, pair_mad


def timed(fn, reps, warm=2):
    for _ in range(warm):
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--slab", type=int, default=250_000)
    ap.add_argument("--bench-this", default="")
    ap.add_argument("--bench-parent", default="")
    args = ap.parse_args()

    from stac_mjx_amd import prep
    from stac_mjx_amd.engine import load_library

    if not torch.cuda.is_available():
        raise SystemExit("pairwise_bench needs a GPU: nothing is measured without one")
    lib = load_library()
    T, K = args.frames, args.kp
    P = K * (K - 1) // 2
    rng = np.random.default_rng(14)
    shape = rng.uniform(-0.15, 0.15, (1, K, 3)).astype(np.float32)
    drift = np.cumsum(rng.standard_normal((T, 1, 3)).astype(np.float32) * np.float32(1e-3), axis=0, dtype=np.float32)
    x = shape + drift + rng.standard_normal((T, K, 3)).astype(np.float32) * np.float32(1e-3)
    hit = rng.random((T, K)) < 0.01
    x[hit] += (0.1 * rng.standard_normal((int(hit.sum()), 3))).astype(np.float32)
    x[rng.random((T, K)) < 0.02] = np.nan
    kp = torch.as_tensor(np.ascontiguousarray(x.reshape(T, 3 * K))).cuda()
    del x, drift
    thr, min_dev, votes = prep.pairwise_params(6.0, 0.002, 2)

    out = torch.empty((T, 3 * K), dtype=torch.float32, device="cuda")
    flag = torch.empty((T, K), dtype=torch.uint8, device="cuda")
    pair_n = torch.empty(max(P, 1), dtype=torch.int64, device="cuda")
    pair_med = torch.empty(max(P, 1), dtype=torch.float64, device="cuda")
    pair_mad = torch.empty(max(P, 1), dtype=torch.float64, device="cuda")
    nbytes = prep.pairwise_workspace_bytes(T, K)
    work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def kernel():
        rc = lib.stac_prep_pairwise(p(kp), T, K, thr, min_dev, votes, p(out), p(flag), p(pair_n), p(pair_med), p(pair_mad), p(work), nbytes, stream)
        assert rc == 0, lib.stac_last_error().decode()

    k_time = timed(kernel, args.reps)
    t_time = timed(lambda: torch_pairwise(kp, thr, min_dev, votes, args.slab), args.torch_reps, warm=1)
    ref = torch_pairwise(kp, thr, min_dev, votes, args.slab)
    got = (out, flag, pair_n[:P], pair_med[:P], pair_mad[:P])
    as_bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else (t.view(torch.int32) if t.dtype == torch.float32 else t)  # noqa: E731
    equal = {name: bool(torch.equal(as_bits(g), as_bits(r))) for name, g, r in zip(("out", "flag", "pair_n", "pair_med", "pair_mad"), got, ref)}
    series_bytes, keys_bytes = T * 3 * K * 4, P * T * 4
    moved = {"series read twice (distances, then the copy to out)": 2 * series_bytes, "keys written once": keys_bytes,
             "keys read seven times (six counting passes, the decision)": 7 * keys_bytes, "out written": series_bytes, "flag written": T * K}
    total = int(sum(moved.values()))
    rate = total / (k_time["ms_median"] * 1e-3)
    result = {"tool": "profiles/tools/pairwise_bench.py", "command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
              "n_frames": T, "n_kp": K, "n_pairs": P, "n_sigma": 6.0, "thr": thr, "min_dev": min_dev, "votes": votes,
              "workspace_bytes": nbytes, "displaced_fraction": float(hit.mean()), "rejected_fraction": float(flag.float().mean()),
              "timing": "device events around one call on preallocated buffers, after 2 warm-up calls (torch: 1)",
              "bytes_moved_at_least": moved | {"total": total}, "hbm_peak_bytes_per_s": {"spec": HBM_PEAK_SPEC, "measured float4 copy": HBM_PEAK_MEASURED},
              "stac_prep_pairwise": k_time | {"bytes_per_s": rate, "fraction_of_hbm_peak_spec": rate / HBM_PEAK_SPEC,
                                              "fraction_of_hbm_peak_measured": rate / HBM_PEAK_MEASURED},
              "torch_sort_per_pair": t_time | {"slab_frames": args.slab}, "torch_over_kernel": t_time["ms_median"] / k_time["ms_median"],
              "bit_equal_to_torch": equal}
    print(json.dumps({"kernel_ms": k_time["ms_median"], "torch_ms": t_time["ms_median"], "torch_over_kernel": result["torch_over_kernel"],
                      "fraction_of_hbm_peak_spec": rate / HBM_PEAK_SPEC, "rejected": result["rejected_fraction"], "bit_equal_to_torch": equal}), flush=True)
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
