"""``Stac.ik_only`` plus post-processing of a continuous run, host path against ``stac.postprocess: gpu``, on one GPU
(DESIGN.md "Post-processing on the GPU", profiles/post/postprocess_bench.json).

  python profiles/tools/postprocess_bench.py --out profiles/post/postprocess_bench.json [--clips 40,4000] [--runs 3]

The recording is the synthetic rodent one of ``bench.py --mode run`` (clips of 250 frames, seeds 11 / 12), run with
``continuous`` and ``infer_qvels`` on: windows of 260 frames are solved, cross-faded and stitched, then ``qvel`` is inferred per
clip.  Per size the two paths alternate (host gpu gpu host ...), ``--runs`` times each after one warm-up each; every run is timed by the host clock
around work that ends in a device synchronise, its phases by ``Stac.timings``.  The host path is what ``main.run_stac`` does
after ``ik_only`` (``utils.handle_edge_effects``, then ``utils.compute_velocity_from_kinematics`` per clip) and is unchanged
code, so its figure is the parent commit's.  The outputs of the last run of each path are compared (tests/post_cases.py).
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--clips", default="40,4000")
    ap.add_argument("--frames-per-clip", type=int, default=250)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()

    import bench
    import post_cases as pc
    from stac_mjx_amd import utils
    from stac_mjx_amd.config import validate_config
    from stac_mjx_amd.stac import Stac
    from stac_mjx_amd.synth import synth_keypoints, synth_offsets

    if not torch.cuda.is_available():
        raise SystemExit("postprocess_bench needs a GPU: nothing is measured without one")
    fs, mcfg = bench.load_setup("rodent")
    F = args.frames_per_clip
    cfg = validate_config({"model": dict(mcfg), "stac": dict(
        fit_offsets_path="fit.h5", ik_only_path="ik.h5", data_path="synthetic", continuous=True, n_fit_frames=F,
        skip_fit_offsets=True, skip_ik_only=False, infer_qvels=True, n_frames_per_clip=F, gather="none",
        mujoco=dict(solver="newton", iterations=1, ls_iterations=4))})
    stac = Stac(None, cfg, fs.kp_names, setup=fs, device="cuda:0", verbose=False)
    eng = stac.engine
    offsets = synth_offsets(fs)
    eng.set_site_pos(offsets)
    fk = lambda q: eng.fk(q, want=("site_xpos",))["site_xpos"].cpu().numpy()
    post = {"continuous": True, "n_frames_per_clip": F, "infer_qvels": True}

    def run(path, kp_flat):
        stac.timings = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if path == "gpu":
            data = stac.ik_only(kp_flat, offsets, post=post)
        else:  # main.run_stac after ik_only, line by line
            data = stac.ik_only(kp_flat, offsets)
            t1 = time.perf_counter()
            data = utils.handle_edge_effects(data, F)
            batched = data.qpos.reshape((-1, F, data.qpos.shape[-1]))
            qvels = [utils.compute_velocity_from_kinematics(c, dt=stac._timestep, freejoint=stac._freejoint) for c in batched]
            data.qvel = np.stack(qvels).reshape(-1, qvels[0].shape[-1])
            stac.timings["postprocess_s"] = time.perf_counter() - t1
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        phases = {k: round(v, 4) for k, v in stac.timings.items()}
        stac.timings = None
        return data, {"wall_s": round(wall, 4), "phases_s": phases}

    result = {"tool": "profiles/tools/postprocess_bench.py", "command": "python " + " ".join(sys.argv),
              "device": torch.cuda.get_device_name(0), "n_frames_per_clip": F, "overlap": utils.CONTINUOUS_BATCH_OVERLAP,
              "continuous": True, "infer_qvels": True, "runs_per_path": args.runs, "order": "one warm-up each, then host gpu gpu host host gpu ...: every run records which path ran before it",
              "sizes": []}
    for C in [int(c) for c in args.clips.split(",")]:
        kp, _ = synth_keypoints(fs, fk, C, F, seed=11, noise_seed=12)
        kp_flat = kp.reshape(C * F, -1)
        runs, last = {"host": [], "gpu": []}, {}
        for path in ("host", "gpu"):
            run(path, kp_flat)
        prev = "gpu"
        for i in range(args.runs):
            for path in (("host", "gpu") if i % 2 == 0 else ("gpu", "host")):  # host gpu gpu host host gpu ...
                last[path], rec = run(path, kp_flat)
                rec["after"] = prev
                prev = path
                runs[path].append(rec)
        h, g = last["host"], last["gpu"]
        for name in ("qpos", "xpos", "xquat", "marker_sites", "kp_data"):
            np.testing.assert_array_equal(getattr(g, name), getattr(h, name), err_msg=name)
        differ, total = pc.check_qvel(g.qvel, h.qvel, True, label=f"{C} clips")
        entry = {"clips": C, "frames_out": int(h.qpos.shape[0]), "frames_solved": C * (F + utils.CONTINUOUS_BATCH_OVERLAP),
                 "outputs": {"stitched arrays": "bit-equal", "qvel outside the gyro columns": "bit-equal",
                             "gyro values not bit-equal (at most 2 float32 ulp)": differ, "gyro values": total}}
        for path in ("host", "gpu"):
            walls = [r["wall_s"] for r in runs[path]]
            posts = [r["phases_s"]["postprocess_s"] for r in runs[path]]
            entry[path] = {"runs": runs[path], "wall_s_median": float(np.median(walls)), "wall_s_min_max": [min(walls), max(walls)],
                           "postprocess_s_median": float(np.median(posts)),
                           "frames_per_s_end_to_end": h.qpos.shape[0] / float(np.median(walls))}
        entry["postprocess_speedup_gpu_over_host"] = entry["host"]["postprocess_s_median"] / entry["gpu"]["postprocess_s_median"]
        entry["end_to_end_speedup_gpu_over_host"] = entry["host"]["wall_s_median"] / entry["gpu"]["wall_s_median"]
        result["sizes"].append(entry)
        print(json.dumps({k: entry[k] for k in ("clips", "frames_out", "postprocess_speedup_gpu_over_host", "end_to_end_speedup_gpu_over_host")}
                         | {p: {k: entry[p][k] for k in ("wall_s_median", "postprocess_s_median", "frames_per_s_end_to_end")} for p in ("host", "gpu")}),
              flush=True)
        del kp, kp_flat, last, h, g
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(result, indent=1) + "\n")
        print(f"wrote {out}")


if __name__ == "__main__":
    main()
