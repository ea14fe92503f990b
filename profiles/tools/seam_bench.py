"""Warm-started clips and pose steps on one GPU (DESIGN.md "Warm-started clips and pose steps", profiles/seam/seam_bench.json):

  1. the q_phase of ``Stac.ik_only`` at 1, 2 and 3 passes (``stac.seam_passes``) on the golden rodent recording, repeated to 250 000
     rows, as 1000 clips x 250 and as 5000 clips x 50, with the mean seam jump and the solver iterations per frame of every pass;
  2. ``stac_seam_steps`` on 10^6 x 74 against the same six quantities written with torch tensor operations.

  python profiles/tools/seam_bench.py --out profiles/seam/seam_bench.json [--reps 10] [--rows 1000000]

Device events around whole calls, medians of ``--reps`` calls after 2 warm-up calls.  There is no gate: P passes cost about P times
one by construction, and the instrument reads its input once.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(Path(__file__).resolve().parent)]

from select_bench import timed  # noqa: E402


def run_cfg(mcfg, **over):
    from stac_mjx_amd.config import validate_config

    stac = dict(fit_offsets_path="fit.h5", ik_only_path="ik.h5", data_path="d.mat", continuous=False, n_fit_frames=4, skip_fit_offsets=False,
                skip_ik_only=False, infer_qvels=False, n_frames_per_clip=2, mujoco=dict(solver="newton", iterations=1, ls_iterations=4))
    stac.update(over)
    return validate_config({"model": dict(mcfg), "stac": stac})


def torch_steps(q, L, cols, n_lin, scalar):
    """The six outputs of stac_seam_steps as torch tensor operations (values that are not finite are not treated: timing only)"""
    N, nq = q.shape
    d = (q[1:] - q[:-1]).abs()
    ds = d[:, scalar]
    best, arg = ds.max(dim=1)
    measure = d.clone()
    rot = None
    for c in cols:
        a, b = q[:-1, c:c + 4], q[1:, c:c + 4]
        dot = ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]) + a[:, 3] * b[:, 3]
        r = 1.0 - dot.abs()
        measure[:, c] = r
        measure[:, c + 1:c + 4] = 0
        rot = r if rot is None else torch.maximum(rot, r)
    lin2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] if n_lin == 3 else torch.zeros(N - 1, device=q.device)
    seam = (torch.arange(1, N, device=q.device) % L) == 0
    measure = measure.clamp_min(0.0)
    zero = torch.zeros((), device=q.device)
    col_seam = torch.where(seam[:, None], measure, zero).amax(dim=0)
    col_in = torch.where(seam[:, None], zero, measure).amax(dim=0)
    z = torch.zeros(1, device=q.device)
    return {"step_joint": torch.cat([z, best]), "step_col": torch.cat([torch.full((1,), -1, device=q.device, dtype=torch.int32), scalar[arg].to(torch.int32)]),
            "step_rot": torch.cat([z, rot if rot is not None else torch.zeros(N - 1, device=q.device)]), "step_lin2": torch.cat([z, lin2]),
            "col_max_in": col_in, "col_max_seam": col_seam}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--frames", type=int, default=250_000)
    ap.add_argument("--skip-passes", action="store_true")
    args = ap.parse_args()

    from stac_mjx_amd import seam
    from stac_mjx_amd.fit_model import finish_fit_setup
    from stac_mjx_amd.mjcf import ModelTables
    from stac_mjx_amd.stac import Stac

    if not torch.cuda.is_available():
        raise SystemExit("seam_bench needs a GPU: nothing is measured without one")
    golden = ROOT / "tests" / "golden"
    mcfg = json.loads((golden / "rodent_model_cfg.json").read_text())
    fs = finish_fit_setup(ModelTables.load(golden / "rodent_tables.npz"), mcfg, list(mcfg["KEYPOINT_MODEL_PAIRS"].keys()))
    nq = fs.tables.nq
    scalar_np = seam.scalar_columns(nq, (3,), 3)
    result = {"tool": "profiles/tools/seam_bench.py", "command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
              "timing": f"device events around whole calls, medians of {args.reps} calls after 2 warm-up calls", "passes": [], "steps": None}

    def save():
        if args.out:
            path = Path(args.out)
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_text(json.dumps(result, indent=1) + "\n")

    # ---- the instrument (first: it is quick) -----------------------------------------------------------------------------------------------------------
    N, L, cols, n_lin = args.rows, 250, (3,), 3
    gen = torch.Generator(device="cuda").manual_seed(3)
    q = torch.cumsum(0.01 * torch.randn(N, nq, device="cuda", generator=gen), dim=0).contiguous()
    quat = torch.randn(N, 4, device="cuda", generator=gen)
    q[:, 3:7] = quat / quat.norm(dim=1, keepdim=True)
    scalar = torch.as_tensor(scalar_np).cuda()
    t_hip = timed(lambda: seam.seam_steps(q, L, cols, n_lin), args.reps, warm=2)
    t_torch = timed(lambda: torch_steps(q, L, cols, n_lin, scalar), args.reps, warm=2)
    a, b = seam.seam_steps(q, L, cols, n_lin), torch_steps(q, L, cols, n_lin, scalar)
    same = {k: bool(torch.equal(a[k], b[k])) for k in a}
    nbytes = 4 * N * nq + 16 * N
    result["steps"] = {"n_rows": N, "nq": nq, "clip_len": L, "stac_seam_steps": t_hip, "torch_tensor_operations": t_torch,
                       "speedup": t_torch["ms_median"] / t_hip["ms_median"], "bytes_read_and_written_once": nbytes,
                       "GB_per_s": nbytes / (t_hip["ms_median"] * 1e-3) / 1e9, "outputs_equal_torch_bits": same}
    print(json.dumps(result["steps"]), flush=True)
    save()
    del q, a, b

    # ---- the passes ---------------------------------------------------------------------------------------------------------------
    mocap = np.load(golden / "rodent_mocap_1000.npy").astype(np.float32)
    series = np.tile(mocap, (args.frames // mocap.shape[0], 1))
    if not args.skip_passes:  # offsets of a short calibration on the device, so that the poses are those of a real run
        cal = Stac(None, run_cfg(mcfg, n_fit_frames=60), fs.kp_names, setup=fs, verbose=False)
        cal.cfg.model.N_ITERS = 3
        offsets = cal.fit_offsets(mocap[0:1000:16][:60]).offsets
    for F in (() if args.skip_passes else (250, 50)):
        stac = Stac(None, run_cfg(mcfg, n_frames_per_clip=F), fs.kp_names, setup=fs, verbose=False)
        stac.engine.set_site_pos(torch.as_tensor(offsets))
        C = series.shape[0] // F
        kp = torch.as_tensor(series[: C * F].reshape(C, F, -1)).cuda()
        scalar = torch.as_tensor(scalar_np).cuda()
        for P in (1, 2, 3):
            keep = {}

            def run():
                res = stac._q_phase(kp, do_root_opt=fs.do_root_opt)
                if P > 1:
                    stac._seam_passes(res, kp, C, 0, P)
                keep["res"] = res

            t = timed(run, args.reps, warm=2)
            res = keep["res"]
            q = res["qpos"]
            jump = (q[1:, 0][:, scalar] - q[:-1, F - 1][:, scalar]).abs().amax(dim=1)
            cnt = res["counters"].to(torch.int64)
            entry = {"n_clips": C, "n_frames_per_clip": F, "passes": P, "q_phase": t, "frames_per_s": C * F / (t["ms_median"] * 1e-3),
                     "seam_jump_mean_rad": float(jump.mean()), "seam_jump_max_rad": float(jump.max()),
                     "frame_error_mean": float(res["frame_error"].mean()),
                     # of the LAST pass's launch: clip 0 is pass 1's, the clips behind it are pass P's
                     "solver_iterations_per_frame_clip0": float(cnt[0, :, 0].sum()) / F,
                     "solver_iterations_per_frame_clips1": float(cnt[1:, :, 0].sum()) / ((C - 1) * F)}
            result["passes"].append(entry)
            print(json.dumps(entry), flush=True)
            save()  # (after every case: a run that is cut short keeps what it measured)

    if args.out:
        print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
