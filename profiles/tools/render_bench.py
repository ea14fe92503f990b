"""Render throughput on one GPU (DESIGN.md "Rendering", profiles/render/render_bench.json).

  python profiles/tools/render_bench.py --out profiles/render/render_bench.json [--quick]

* kernel frames/s of stac_render (device events, after a warm-up, over a window of at least 1 s): the rodent's stored fit
  (tests/golden/demo_viz_golden.npz, 50 poses) tiled to 2000 frames at 1920 x 1200, cameras close_profile and -1, with and
  without the error segments; bytes written per frame over kernel time as a share of HBM peak;
* the split of a 1000-frame Stac.render-style job to .avi: FK + cameras + render, device-to-host copy, JPEG encode + write;
* the f32 C restatement of the kernel (tests/tools/render_ref.c) on the CPU threads of the run: a CPU restatement figure,
  not a baseline of the reference (whose renderer is MuJoCo's OpenGL one).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import tarfile
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tests" / "tools")]
HBM_PEAK_BPS = 8.0e12  # MI355X HBM3E peak


def _io_threads():
    from stac_mjx_amd.io import _n_threads

    return _n_threads()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--viz-frames", type=int, default=1000)
    ap.add_argument("--quick", action="store_true", help="small sizes (a smoke run of this script)")
    args = ap.parse_args()
    from render_cases import kp_rgba, rodent_scene
    from stac_mjx_amd.engine import Engine
    from stac_mjx_amd.fit_model import finish_fit_setup
    from stac_mjx_amd.mjcf import ModelTables
    from stac_mjx_amd.render import Renderer
    from stac_mjx_amd.video import encode_jpegs, write_avi

    g = ROOT / "tests" / "golden"
    cfg = json.load(open(g / "rodent_model_cfg.json"))
    pairs = cfg["KEYPOINT_MODEL_PAIRS"]
    fs = finish_fit_setup(ModelTables.load(g / "rodent_tables_legacy.npz"), cfg, list(pairs))
    tmp = Path(tempfile.mkdtemp())
    with tarfile.open(g / "reference_fixtures.tar.xz") as tf:
        tf.extractall(tmp)
    scene = rodent_scene(tmp, cfg)
    eng = Engine(fs.tables, fs.lb, fs.ub, device="cuda:0")
    r = Renderer(eng, scene, list(pairs), list(pairs.values()), kp_rgba(cfg), float(cfg["MARKER_SIZE"]), memory_budget=16 << 30)
    dv = dict(np.load(g / "demo_viz_golden.npz"))
    W, H = (480, 300) if args.quick else (1920, 1200)
    N = 100 if args.quick else args.frames
    reps = (N + 49) // 50
    qpos = np.tile(dv["qpos"], (reps, 1))[:N]
    kp = np.tile(dv["kp_data"], (reps, 1))[:N]
    t = fs.tables
    res = {"width": W, "height": H, "frames": N, "primitives": r.P + 3 * r.K, "kernel": {}}
    xpos, xquat, markers = r.poses(torch.as_tensor(qpos).cuda(), dv["offsets"])
    kpt = torch.as_tensor(kp, dtype=torch.float32).cuda().reshape(N, r.K, 3)
    rgb = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda:0")
    for camera in ("close_profile", -1):
        cam, tanh = r.cameras(camera, xpos, xquat, t.qpos0, t.body_parentid)
        for show in (False, True):
            launch = lambda: r.handle.render(xpos, xquat, kpt, markers, show, cam, tanh, W, H, rgb)
            launch()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n, elapsed = 0, 0.0
            e0.record()
            while elapsed < 1.0 or n < 2:
                launch()
                n += 1
                e1.record()
                e1.synchronize()
                elapsed = e0.elapsed_time(e1) / 1e3
            fps = n * N / elapsed
            bytes_per_frame = W * H * 3
            key = f"{camera}_{'segments' if show else 'plain'}"
            res["kernel"][key] = {"frames_per_s": fps, "ms_per_frame": 1e3 / fps, "launches": n, "window_s": elapsed,
                                  "write_GBps": fps * bytes_per_frame / 1e9,
                                  "write_share_of_hbm_peak": fps * bytes_per_frame / HBM_PEAK_BPS}
            print(key, json.dumps(res["kernel"][key]), flush=True)
    del rgb
    torch.cuda.empty_cache()

    # a viz job: FK + cameras + render, copy to the host, JPEG encode + AVI write
    V = 50 if args.quick else args.viz_frames
    qv, kv = np.tile(dv["qpos"], (V // 50 + 1, 1))[:V], np.tile(dv["kp_data"], (V // 50 + 1, 1))[:V]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    xp, xq, mk = r.poses(torch.as_tensor(qv).cuda(), dv["offsets"])
    cam, tanh = r.cameras("close_profile", xp, xq, t.qpos0, t.body_parentid)
    dbuf = torch.empty((V, H, W, 3), dtype=torch.uint8, device="cuda:0")
    r.handle.render(xp, xq, torch.as_tensor(kv, dtype=torch.float32).cuda().reshape(V, r.K, 3), mk, False, cam, tanh, W, H, dbuf)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    host = torch.empty((V, H, W, 3), dtype=torch.uint8, pin_memory=True)
    host.copy_(dbuf)
    t2 = time.perf_counter()
    frames = list(host.numpy())
    jp = encode_jpegs(frames)
    write_avi(tmp / "v.avi", frames, fps=float(cfg["RENDER_FPS"]), jpegs=jp)
    t3 = time.perf_counter()
    res["viz_avi"] = {"frames": V, "render_s": t1 - t0, "d2h_s": t2 - t1, "jpeg_and_write_s": t3 - t2,
                      "io_threads": _io_threads(), "avi_bytes": (tmp / "v.avi").stat().st_size}
    print("viz_avi", json.dumps(res["viz_avi"]), flush=True)

    # the f32 C restatement on the CPU
    from build_render_ref import RenderRef

    ref = RenderRef("float")
    nc = 2 if args.quick else 4
    c = cam[:nc].cpu().numpy()
    t0 = time.perf_counter()
    ref.render(r.tables, t.nbody, xp[:nc].cpu().numpy(), xq[:nc].cpu().numpy(), kv[:nc], mk[:nc].cpu().numpy(), False, c, tanh, W, H)
    dt = time.perf_counter() - t0
    res["cpu_restatement_f32"] = {"frames": nc, "frames_per_s": nc / dt, "threads": int(os.environ.get("OMP_NUM_THREADS", "0") or 0)}
    print("cpu_restatement_f32", json.dumps(res["cpu_restatement_f32"]), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
