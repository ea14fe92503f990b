"""``stac_select_diverse`` (stac.fit_frames: diverse) on one GPU, and the same selection written with torch tensor operations on the
same device: the thing to beat (DESIGN.md "Choosing calibration frames", profiles/select/select_bench.json).

  python profiles/tools/select_bench.py --out profiles/select/select_bench.json [--cases 1000000:1000,100000:100] [--kp 23] [--reps 5]

The series is seeded noise around a slow drift, every frame a candidate.  The entry point is one call; its parts are told apart by
device events around whole calls on preallocated buffers: a call with ``n_select = 1`` is ``describe`` plus one (sum-free) update and
one pick, a call with ``n_select = n`` adds n - 1 update / pick pairs, so the pick loop is the difference and a pick is that over
n - 1.  ``--reps`` calls each after two warm-up calls, medians.  Bytes per pick: what the update pass has to stream, the T x P
distances (4 bytes each) plus dmin read and written and the flags (9 bytes per frame); the P distances of the pick and the block
maxima are noise beside them.  The torch version keeps the same T x P distances and does per pick ``((D - D[s]) ** 2).sum(1)``,
``minimum`` and ``argmax``: it lives here only, not in the package.  Kernel names and times of one call: a separate run under
``rocprofv3 --kernel-trace --stats`` with ``--profile-only`` (no torch version, one call per case).
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

from prep_bench import HBM_PEAK_MEASURED, HBM_PEAK_SPEC  # noqa: E402


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


def torch_descriptors(kp, K):
    x = kp.reshape(kp.shape[0], K, 3)
    a, b = torch.triu_indices(K, K, 1, device=kp.device)
    out = torch.empty((kp.shape[0], a.numel()), dtype=torch.float32, device=kp.device)
    step = 1 << 16  # (in slabs: the [T, P, 3] difference of a million frames is 3 GB)
    for lo in range(0, kp.shape[0], step):
        d = x[lo:lo + step, a] - x[lo:lo + step, b]
        out[lo:lo + step] = (d * d).sum(-1).sqrt()
    return out


def torch_picks(D, n):
    """Greedy farthest-point picks over the rows of D with tensor operations; no copy to the host inside the loop"""
    T = D.shape[0]
    sel = torch.empty(n, dtype=torch.int64, device=D.device)
    dmin = torch.full((T,), float("inf"), device=D.device)
    s = torch.zeros((), dtype=torch.int64, device=D.device)
    sel[0] = s
    for i in range(1, n):
        e = D - D[s]
        dmin = torch.minimum(dmin, (e * e).sum(1))
        s = torch.argmax(dmin)
        sel[i] = s
    return sel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="1000000:1000,100000:100")
    ap.add_argument("--kp", type=int, default=23)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile-only", action="store_true")
    args = ap.parse_args()

    from stac_mjx_amd import select
    from stac_mjx_amd.engine import load_select_library

    if not torch.cuda.is_available():
        raise SystemExit("select_bench needs a GPU: nothing is measured without one")
    lib = load_select_library()
    K = args.kp
    P = K * (K - 1) // 2
    result = {"tool": "profiles/tools/select_bench.py", "command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
              "n_kp": K, "pairs": P, "timing": "device events around whole calls on preallocated buffers, after 2 warm-up calls; pick loop = "
              "call with n_select = n minus call with n_select = 1", "hbm_peak_bytes_per_s": {"spec": HBM_PEAK_SPEC, "measured float4 copy": HBM_PEAK_MEASURED},
              "cases": []}
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for case in args.cases.split(","):
        T, n = (int(v) for v in case.split(":"))
        rng = np.random.default_rng(5)
        kp_np = (np.cumsum(rng.standard_normal((T, 3 * K), dtype=np.float32) * np.float32(1e-3), axis=0, dtype=np.float32)
                 + rng.standard_normal((T, 3 * K), dtype=np.float32) * np.float32(1e-2))
        kp = torch.as_tensor(kp_np).cuda()
        nbytes = select.workspace_bytes(T, K)
        work = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
        sel = torch.empty(n, dtype=torch.int64, device="cuda")
        radius2 = torch.empty(n, dtype=torch.float32, device="cuda")
        n_selected = torch.empty(1, dtype=torch.int64, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call(m):
            rc = lib.stac_select_diverse(p(kp), T, K, None, m, p(sel), p(radius2), p(n_selected), p(work), nbytes, stream)
            assert rc == 0, lib.stac_select_last_error().decode()

        if args.profile_only:
            call(n)
            torch.cuda.synchronize()
            continue
        one = timed(lambda: call(1), args.reps)
        full = timed(lambda: call(n), args.reps)
        torch.cuda.synchronize()
        assert int(n_selected.item()) == n
        hip_sel = sel.cpu().numpy().copy()
        loop_ms = full["ms_median"] - one["ms_median"]
        per_pick_bytes = T * P * 4 + T * 9
        rate = per_pick_bytes / (loop_ms * 1e-3 / (n - 1))
        entry = {"n_frames": T, "n_select": n, "workspace_bytes": nbytes, "call_n1_describe_and_first_pick": one, "call_n": full,
                 "pick_loop_ms": loop_ms, "ms_per_pick": loop_ms / (n - 1), "bytes_streamed_per_pick": per_pick_bytes, "update_pass_bytes_per_s": rate,
                 "fraction_of_hbm_peak_spec": rate / HBM_PEAK_SPEC, "fraction_of_hbm_peak_measured": rate / HBM_PEAK_MEASURED,
                 "distances_fit_the_256_MiB_last_level_cache": T * P * 4 <= 256 * 2**20}
        # the same selection with tensor operations
        t_desc = timed(lambda: torch_descriptors(kp, K), max(args.reps // 2, 1), warm=1)
        D = torch_descriptors(kp, K)
        t_loop = timed(lambda: torch_picks(D, n), max(args.reps // 2, 1), warm=1)
        torch_sel = torch_picks(D, n).cpu().numpy()
        same = int(np.count_nonzero(torch_sel == hip_sel))
        entry["torch"] = {"descriptors": t_desc, "pick_loop": t_loop, "ms_per_pick": t_loop["ms_median"] / (n - 1),
                          "picks_equal_to_the_kernels": same, "note": "torch sums the squares in another order: a pick may differ where two "
                          "candidates are within rounding of each other, and every later pick with it"}
        entry["torch_over_hip_whole_selection"] = (t_desc["ms_median"] + t_loop["ms_median"]) / full["ms_median"]
        result["cases"].append(entry)
        print(json.dumps({"T": T, "n": n, "hip_call_ms": full["ms_median"], "describe_and_first_pick_ms": one["ms_median"], "ms_per_pick": entry["ms_per_pick"],
                          "fraction_of_hbm_peak_spec": entry["fraction_of_hbm_peak_spec"], "torch_ms": t_desc["ms_median"] + t_loop["ms_median"],
                          "picks_equal": same}), flush=True)
        del kp, work, D
        torch.cuda.empty_cache()
    if args.out and not args.profile_only:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1) + "\n")
        print(f"wrote {path}")


if __name__ == "__main__":
    main()
