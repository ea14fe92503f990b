"""``stac.smooth`` on one GPU: the kernel against a ``torch.clone`` of the same tensor, ``Stac.ik_only`` of a continuous run with
and without smoothing, and what the smoothing does to the trajectory (DESIGN.md "Smoothing fitted poses",
profiles/smooth/smooth_bench.json).

  python profiles/tools/smooth_bench.py --out profiles/smooth/smooth_bench.json [--clips 4000] [--runs 3]
        [--parent-lib PATH/libstac_hip.so]

Kernel: qpos of 1 000 000 x 74 (rodent) and 200 000 x 230 (mouse), one clip each, half-widths 3 and 16, Savitzky-Golay taps.  Per
shape the kernel and the clone alternate (smooth clone clone smooth ...), ``--reps`` launches each per turn between two device
events, after a warm-up of both; medians over the turns.  Bytes moved: one read and one write of the tensor (what the clone moves as
well); the read amplification of the tile the host picks is stated beside it.  The random input is a stand-in: the kernel's time
does not depend on the values.

End to end: the synthetic rodent recording of ``bench.py --mode run`` (clips of 250 frames, seeds 11 / 12), ``continuous`` and
``infer_qvels`` on, ``postprocess: gpu``; ``smooth: off`` and ``smooth: savgol`` (half-width 3, order 2) alternate, ``--runs``
times each after one warm-up each, every run timed by the host clock around work that ends in a device synchronise, its phases by
``Stac.timings``.  Effect: the rms of the second difference of qpos and of qvel and the overall marker rms of ``Stac.fit_report``,
of the last run of each.

``--parent-lib``: the default line of ``bench.py`` (``--gpus 1 --steps 3 --warmup 1``) as child processes, this tree's library and
the given one alternating, three runs each.  Every GPU step of a child process runs under ``timeout``.
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

KERNEL_SHAPES = [("rodent", 1_000_000, 74), ("mouse", 200_000, 230)]
HALF_WINDOWS = (3, 16)


def kernel_section(reps, turns):
    from stac_mjx_amd import post

    out = []
    for model, N, nq in KERNEL_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        q = torch.randn((N, nq), device="cuda", generator=g)
        q[:, 3:7] /= q[:, 3:7].norm(dim=1, keepdim=True)
        lb = torch.full((nq,), -3.0, device="cuda")
        ub = torch.full((nq,), 3.0, device="cuda")
        nbytes = 2 * N * nq * 4
        for H in HALF_WINDOWS:
            taps = post.smooth_taps("savgol", H)
            T = post.smooth_tile_frames(nq, H)
            work = {"smooth": lambda: post.smooth(q, N, taps, [3], lb=lb, ub=ub), "clone": lambda: q.clone()}

            def timed(fn):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    fn()
                b.record()
                b.synchronize()
                return a.elapsed_time(b) * 1e-3 / reps

            for fn in work.values():
                timed(fn)
            times, order = {"smooth": [], "clone": []}, []
            for i in range(turns):
                for name in (("smooth", "clone") if i % 2 == 0 else ("clone", "smooth")):
                    times[name].append(timed(work[name]))
                    order.append(name)
            med = {k: float(np.median(v)) for k, v in times.items()}
            entry = {"model": model, "rows": N, "nq": nq, "half_window": H, "window": 2 * H + 1, "tile_frames": T,
                     "read_amplification_of_the_tile": (T + 2 * H) / T, "bytes_read_plus_written": nbytes, "launches_per_turn": reps,
                     "order": order,
                     "smooth_s": {"median": med["smooth"], "min_max": [min(times["smooth"]), max(times["smooth"])], "includes": "the tap upload and its stream-ordered allocation, and the output tensor's allocation"},
                     "clone_s": {"median": med["clone"], "min_max": [min(times["clone"]), max(times["clone"])]},
                     "smooth_GB_per_s": nbytes / med["smooth"] * 1e-9, "clone_GB_per_s": nbytes / med["clone"] * 1e-9,
                     "bandwidth_ratio_smooth_over_clone": med["clone"] / med["smooth"],
                     "ratio_predicted_by_the_tile": 2.0 / (1.0 + (T + 2 * H) / T)}
            out.append(entry)
            print(json.dumps({k: entry[k] for k in ("model", "half_window", "tile_frames", "smooth_GB_per_s", "clone_GB_per_s",
                                                    "bandwidth_ratio_smooth_over_clone", "ratio_predicted_by_the_tile")}), flush=True)
        del q
    return out


def end_to_end_section(clips, F, runs):
    import bench
    from stac_mjx_amd import utils
    from stac_mjx_amd.config import smooth_options, validate_config
    from stac_mjx_amd.stac import Stac
    from stac_mjx_amd.synth import synth_keypoints, synth_offsets

    fs, mcfg = bench.load_setup("rodent")
    cfg = validate_config({"model": dict(mcfg), "stac": dict(
        fit_offsets_path="fit.h5", ik_only_path="ik.h5", data_path="synthetic", continuous=True, n_fit_frames=F,
        skip_fit_offsets=True, skip_ik_only=False, infer_qvels=True, n_frames_per_clip=F, gather="none", postprocess="gpu", smooth="savgol",
        mujoco=dict(solver="newton", iterations=1, ls_iterations=4))})
    stac = Stac(None, cfg, fs.kp_names, setup=fs, device="cuda:0", verbose=False)
    eng = stac.engine
    offsets = synth_offsets(fs)
    eng.set_site_pos(offsets)
    fk = lambda q: eng.fk(q, want=("site_xpos",))["site_xpos"].cpu().numpy()  # noqa: E731
    kp, _ = synth_keypoints(fs, fk, clips, F, seed=11, noise_seed=12)
    kp_flat = kp.reshape(clips * F, -1)
    base = {"continuous": True, "n_frames_per_clip": F, "infer_qvels": True}
    posts = {"off": base, "savgol": dict(base, smooth=smooth_options(cfg.stac))}

    def run(mode):
        stac.timings = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data = stac.ik_only(kp_flat, offsets, post=posts[mode])
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        phases = {k: round(v, 4) for k, v in stac.timings.items()}
        stac.timings = None
        return data, {"wall_s": round(wall, 4), "phases_s": phases}

    recs, last = {"off": [], "savgol": []}, {}
    for mode in posts:
        run(mode)
    prev = "savgol"
    for i in range(runs):
        for mode in (("off", "savgol") if i % 2 == 0 else ("savgol", "off")):
            last[mode], rec = run(mode)
            rec["after"] = prev
            prev = mode
            recs[mode].append(rec)
    np.testing.assert_array_equal(last["savgol"].qpos_raw, last["off"].qpos)

    def rms(a):
        return float(np.sqrt(np.mean(np.square(a, dtype=np.float64))))

    def second_difference(a):
        a = np.asarray(a, dtype=np.float64)
        return a[2:] - 2.0 * a[1:-1] + a[:-2]

    entry = {"clips": clips, "n_frames_per_clip": F, "frames_out": int(last["off"].qpos.shape[0]),
             "frames_solved": clips * (F + utils.CONTINUOUS_BATCH_OVERLAP), "smooth": smooth_options(cfg.stac), "runs_per_mode": runs,
             "order": "one warm-up each, then off savgol savgol off off savgol ...: every run records which mode ran before it"}
    for mode in posts:
        walls = [r["wall_s"] for r in recs[mode]]
        pp = [r["phases_s"]["postprocess_s"] for r in recs[mode]]
        d = last[mode]
        summary = stac.fit_report(d)
        entry[mode] = {"runs": recs[mode], "wall_s_median": float(np.median(walls)), "wall_s_min_max": [min(walls), max(walls)],
                       "postprocess_s_median": float(np.median(pp)), "postprocess_s_min_max": [min(pp), max(pp)],
                       "rms_second_difference_qpos": rms(second_difference(d.qpos)),
                       "rms_second_difference_qpos_joint_columns": rms(second_difference(d.qpos[:, 7:])),
                       "rms_second_difference_qvel": rms(second_difference(d.qvel)),
                       "rms_qvel": rms(d.qvel), "overall_marker_rms": summary["overall"]["rms"]}
    entry["postprocess_s_added_by_smoothing"] = entry["savgol"]["postprocess_s_median"] - entry["off"]["postprocess_s_median"]
    entry["wall_s_ratio_savgol_over_off"] = entry["savgol"]["wall_s_median"] / entry["off"]["wall_s_median"]
    print(json.dumps({m: {k: entry[m][k] for k in ("wall_s_median", "postprocess_s_median", "rms_second_difference_qpos",
                                                   "rms_second_difference_qvel", "overall_marker_rms")} for m in posts}), flush=True)
    return entry


def regression_section(parent_lib, runs=3, limit_s=240):
    """``bench.py``'s default line in child processes: this tree's library and ``parent_lib`` alternating."""
    cmd = ["timeout", "-k", "10", str(limit_s), sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"]
    libs = {"this_tree": None, "parent": str(Path(parent_lib).resolve())}
    lines, order = {k: [] for k in libs}, []
    for i in range(runs):
        for name in (("this_tree", "parent") if i % 2 == 0 else ("parent", "this_tree")):
            env = dict(os.environ)
            if libs[name]:
                env["STAC_HIP_LIB"] = libs[name]
            res = subprocess.run(cmd, capture_output=True, text=True, env=env)
            if res.returncode != 0:  # a failed or timed-out GPU step ends the measurement: nothing more is started on the device
                raise SystemExit(f"bench.py with the library of {name} ended with status {res.returncode}:\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
            line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
            lines[name].append(line)
            order.append(name)
            print(name, json.dumps(line), flush=True)
    return {"command": "python bench.py " + " ".join(cmd[6:]), "order": order, "result_lines": lines}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--clips", type=int, default=4000)
    ap.add_argument("--frames-per-clip", type=int, default=250)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10, help="kernel launches between two events")
    ap.add_argument("--turns", type=int, default=6, help="timed turns per kernel and shape")
    ap.add_argument("--skip", default="", help="comma-separated sections to leave out: kernel, end_to_end")
    ap.add_argument("--parent-lib", default=None, help="a libstac_hip.so built from the parent commit: adds the bench.py comparison")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("smooth_bench needs a GPU: nothing is measured without one")
    skip = set(filter(None, args.skip.split(",")))
    result = {"tool": "profiles/tools/smooth_bench.py", "command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0)}
    if "kernel" not in skip:
        result["kernel"] = kernel_section(args.reps, args.turns)
    if "end_to_end" not in skip:
        result["end_to_end"] = end_to_end_section(args.clips, args.frames_per_clip, args.runs)
    if args.parent_lib:
        torch.cuda.synchronize()
        result["bench_default_line"] = regression_section(args.parent_lib)
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(result, indent=1) + "\n")
        print(f"wrote {out}")


if __name__ == "__main__":
    main()
