"""Render throughput on one GPU (DESIGN.md "Rendering", profiles/render/render_bench.json).

  python profiles/tools/render_bench.py --out profiles/render/render_bench.json [--quick]

* kernel frames/s of stac_render (device events, after a warm-up, over a window of at least 1 s): the rodent's stored fit
  (tests/golden/demo_viz_golden.npz, 50 poses) tiled to 2000 frames at 1920 x 1200, cameras close_profile and -1, with and
  without the error segments; bytes written per frame over kernel time as a share of HBM peak;
* the split of a 1000-frame Stac.render-style job to .avi: FK + cameras + render, device-to-host copy, JPEG encode + write;
* the f32 C restatement of the kernel (tests/tools/render_ref.c) on the CPU threads of the run: a CPU restatement figure,
  not a baseline of the reference (whose renderer is MuJoCo's OpenGL one).

Mesh geoms (profiles/render/render_mesh_bench.json):

  python profiles/tools/render_bench.py --sections kernel            # the mesh-free rodent lines only (parent comparison)
  python profiles/tools/render_bench.py --sections mesh,hierarchy --out profiles/render/render_mesh_bench.json

* ``mesh``: the rodent's stored fit with icospheres attached to its bodies (procedural, so the scene exists wherever the
  script runs): 100 instances of 4 shared meshes, 214 400 triangles in all, about the reference's mouse; kernel frames/s at
  1920 x 1200 from device events over at least 1 s, and the f32 restatement (the same file) on the mesh scene;
* ``hierarchy``: one 20 480-triangle icosphere filling the frame, with the hierarchy and with the developer switch
  STAC_RENDER_MESH_SINGLE_LEAF=1 (read at scene creation): equal pictures, and the time of one launch each.

The JPEG encoder (profiles/render/render_jpeg_bench.json):

  python profiles/tools/render_bench.py --sections encoder --encoders pil,gpu,gpu_noframes --out <file>
  python profiles/tools/render_bench.py --sections encoder --encoders pil --tree <checkout of the parent commit>

* ``encoder``: the 1000-frame rodent job at 1920 x 1200 to ``.avi`` as ``Stac.render`` runs it (a Renderer with the default
  memory budget, so chunks of frames), ``--runs`` times per encoder, the encoders alternating: wall time end to end and its
  parts (FK + cameras + render + copies to the host as far as the encoder needs them; PIL encode; file write).  The GPU
  encoders get one more, instrumented pass with a device synchronisation between the steps of every chunk: render, the
  encode kernels, the copy of the compressed bytes (and of the raw frames) to the host; and the ``.avi`` size against
  Pillow's files without restart markers.  ``--tree``: import the package from another checkout (only ``pil`` there).
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
if "--tree" in sys.argv:  # before the package is imported
    ROOT = Path(sys.argv[sys.argv.index("--tree") + 1]).resolve()
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
    ap.add_argument("--sections", default="kernel,viz,cpu", help="comma list of kernel, viz, cpu, mesh, hierarchy")
    ap.add_argument("--mesh-frames", type=int, default=200)
    ap.add_argument("--encoders", default="pil,gpu,gpu_noframes", help="encoder section: comma list of pil, gpu, gpu_noframes")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tree", default=None, help="import the package from this checkout instead of the script's own")
    args = ap.parse_args()
    sections = set(args.sections.split(","))
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
    for camera in ("close_profile", -1) if "kernel" in sections else ():
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

    if "mesh" in sections:
        res["mesh"] = mesh_section(args, r, fs, scene, cfg, dv, W, H)
    if "hierarchy" in sections:
        res["hierarchy"] = hierarchy_section(args, eng, W, H)
    if "encoder" in sections:
        res["encoder"] = encoder_section(args, eng, scene, fs, cfg, dv, W, H, tmp)
    if not {"viz", "cpu"} & sections:
        return finish(args, res)

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
    finish(args, res)


def encoder_section(args, eng, scene, fs, cfg, dv, W, H, tmp):
    """The viz job end to end, per encoder (see the module docstring)."""
    from render_cases import kp_rgba
    from stac_mjx_amd.render import Renderer
    from stac_mjx_amd.video import JPEG_QUALITY, encode_jpegs, read_avi, write_avi

    pairs = cfg["KEYPOINT_MODEL_PAIRS"]
    r = Renderer(eng, scene, list(pairs), list(pairs.values()), kp_rgba(cfg), float(cfg["MARKER_SIZE"]))  # default budget
    V = 50 if args.quick else args.viz_frames
    qv, kv = np.tile(dv["qpos"], (V // 50 + 1, 1))[:V], np.tile(dv["kp_data"], (V // 50 + 1, 1))[:V]
    t = fs.tables
    fps = float(cfg["RENDER_FPS"])
    kw = dict(qpos0=t.qpos0, parent=t.body_parentid, camera="close_profile", width=W, height=H)
    encoders = args.encoders.split(",")
    out = {"frames": V, "width": W, "height": H, "quality": JPEG_QUALITY, "io_threads": _io_threads(), "runs": {e: [] for e in encoders}}

    def job(enc):
        path = tmp / f"{enc}.avi"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if enc == "pil":
            o = r.render(qv, kv, dv["offsets"], **kw)
            frames = list(o["rgb"].numpy())
            t1 = time.perf_counter()
            jp = encode_jpegs(frames)
            t2 = time.perf_counter()
            write_avi(path, frames, fps, jpegs=jp)
            t3 = time.perf_counter()
            return {"total_s": t3 - t0, "render_and_d2h_s": t1 - t0, "encode_s": t2 - t1, "write_s": t3 - t2, "avi_bytes": path.stat().st_size}
        o = r.render(qv, kv, dv["offsets"], want_jpeg=True, want_rgb=enc == "gpu", **kw)
        frames = list(o["rgb"].numpy()) if enc == "gpu" else []
        t1 = time.perf_counter()
        write_avi(path, None, fps, jpegs=o["jpeg"], size=(W, H))
        t3 = time.perf_counter()
        return {"total_s": t3 - t0, "render_encode_d2h_s": t1 - t0, "write_s": t3 - t1, "avi_bytes": path.stat().st_size,
                "frames_returned": len(frames)}

    for enc in encoders:  # warm-up: allocator, page cache, thread pool
        job(enc)
    for k in range(args.runs):
        for enc in encoders:
            out["runs"][enc].append(job(enc))
            print("encoder", enc, json.dumps(out["runs"][enc][-1]), flush=True)
    for enc in encoders:
        tot = [x["total_s"] for x in out["runs"][enc]]
        out[enc + "_total_s_range"] = [min(tot), max(tot)]
    if any(e.startswith("gpu") for e in encoders):
        out["gpu_split"] = {e: gpu_split(r, qv, kv, dv, kw, W, H, e == "gpu") for e in encoders if e.startswith("gpu")}
        print("encoder gpu_split", json.dumps(out["gpu_split"]), flush=True)
        # bytes against Pillow's files without restart markers (what encoder="pil" writes), over the first 50 frames
        o = r.render(qv[:50], kv[:50], dv["offsets"], want_jpeg=True, **kw)
        pil = encode_jpegs(list(o["rgb"].numpy()))
        out["bytes_first_50_frames"] = {"gpu_restart_one_mcu_row": sum(len(j) for j in o["jpeg"]), "pil_no_restart": sum(len(j) for j in pil),
                                        "raw": 50 * W * H * 3}
        print("encoder bytes", json.dumps(out["bytes_first_50_frames"]), flush=True)
    r.close()
    return out


def gpu_split(r, qv, kv, dv, kw, W, H, want_rgb):
    """One instrumented pass of the GPU-encoder job: a device synchronisation after every step of every chunk."""
    from stac_mjx_amd import jpeg

    dev = r.engine.device
    t = {"fk_cameras_s": 0.0, "render_s": 0.0, "encode_kernels_s": 0.0, "jpeg_d2h_s": 0.0, "raw_d2h_s": 0.0}
    sync = torch.cuda.synchronize
    sync()
    t0 = time.perf_counter()
    N = len(qv)
    q = torch.as_tensor(np.asarray(qv, np.float32)).to(dev)
    kpt = torch.as_tensor(np.asarray(kv, np.float32)).to(dev).reshape(N, r.K, 3)
    xpos, xquat, markers = r.poses(q, dv["offsets"])
    cam, tanh = r.cameras(kw["camera"], xpos, xquat, kw["qpos0"], kw["parent"])
    sync()
    t["fk_cameras_s"] = time.perf_counter() - t0
    R = jpeg.default_restart_mcus(W)
    per_frame = H * W * 3 + jpeg.workspace_bytes(1, W, H, R) + jpeg.JpegEncoder.first_guess(1, W, H)
    chunk = int(max(1, min(N, r.memory_budget // per_frame)))
    enc = jpeg.JpegEncoder(chunk, W, H, jpeg.JPEG_QUALITY, R, dev)
    dbuf = torch.empty((chunk, H, W, 3), dtype=torch.uint8, device=dev)
    host = torch.empty((N, H, W, 3), dtype=torch.uint8) if want_rgb else None
    total = 0
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        n = hi - lo
        t0 = time.perf_counter()
        r.handle.render(xpos[lo:hi], xquat[lo:hi], kpt[lo:hi], markers[lo:hi], False, cam[lo:hi], tanh, W, H, dbuf[:n])
        sync()
        t1 = time.perf_counter()
        jpeg.encode_raw(dbuf[:n], enc.out, enc.frame_offset, enc.workspace, enc.quality, enc.R)
        sync()
        t2 = time.perf_counter()
        off = enc.frame_offset[: n + 1].cpu().tolist()
        assert off[n] <= enc.out.numel(), "first output buffer too small for these pictures"
        data = enc.out[: off[n]].cpu().numpy().tobytes()
        total += len(data)
        t3 = time.perf_counter()
        if want_rgb:
            host[lo:hi].copy_(dbuf[:n])
        t4 = time.perf_counter()
        t["render_s"] += t1 - t0
        t["encode_kernels_s"] += t2 - t1
        t["jpeg_d2h_s"] += t3 - t2
        t["raw_d2h_s"] += t4 - t3
    t.update(chunk_frames=chunk, jpeg_bytes=total, restart_mcus=R)
    return t


def finish(args, res):
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


def timed(launch, min_s=1.0):
    """(launches, seconds) of ``launch`` repeated for at least ``min_s`` of device time, after one warm-up."""
    launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, elapsed = 0, 0.0
    e0.record()
    while elapsed < min_s or n < 2:
        launch()
        n += 1
        e1.record()
        e1.synchronize()
        elapsed = e0.elapsed_time(e1) / 1e3
    return n, elapsed


def mesh_bench_scene(scene, n_inst=100):
    """The rodent's scene with ``n_inst`` icospheres on its bodies: 4 shared meshes (subdivisions 2 to 5, radius 6 to 12 mm;
    30, 60, 5 and 5 instances of 100: 214 400 triangles, the reference's mouse has 207 k in 100 files), instance k on body
    1 + k % (nbody - 1), offset by a few mm; see-through like every geom of a moving body.  Returns the scene, the triangle
    count over the instances and the time to build the hierarchies."""
    import copy

    from render_mesh_cases import icosphere
    from stac_mjx_amd.mesh import make_mesh
    from stac_mjx_amd.mjcf import GEOM_MESH

    t0 = time.perf_counter()
    meshes = [make_mesh(f"ico{s}", icosphere(s, 0.006 + 0.002 * i)) for i, s in enumerate((2, 3, 4, 5))]
    build_s = time.perf_counter() - t0
    sc = copy.copy(scene)
    rng = np.random.default_rng(0)
    G = len(scene.geom_names)
    body = 1 + np.arange(n_inst) % (scene.nbody - 1)
    which = rng.permutation(np.repeat([0, 1, 2, 3], [30, 60, 5, 5]))[:n_inst]
    add = lambda a, b: np.concatenate([a, b])
    sc.geom_names = list(scene.geom_names) + [f"ico_{k}" for k in range(n_inst)]
    sc.geom_type = add(scene.geom_type, np.full(n_inst, GEOM_MESH, np.int32))
    sc.geom_body = add(scene.geom_body, body.astype(np.int32))
    sc.geom_group = add(scene.geom_group, np.zeros(n_inst, np.int32))
    sc.geom_size = add(scene.geom_size, np.zeros((n_inst, 3)))
    sc.geom_pos = add(scene.geom_pos, rng.uniform(-0.004, 0.004, size=(n_inst, 3)))
    sc.geom_quat = add(scene.geom_quat, np.tile([1.0, 0, 0, 0], (n_inst, 1)))
    sc.geom_rgba = add(scene.geom_rgba, np.concatenate([rng.uniform(0.2, 1, size=(n_inst, 3)), np.ones((n_inst, 1))], 1))
    sc.geom_checker = add(scene.geom_checker, np.zeros(n_inst, bool))
    sc.geom_rgb2 = add(scene.geom_rgb2, np.zeros((n_inst, 3)))
    sc.geom_texrepeat = add(scene.geom_texrepeat, np.ones((n_inst, 2)))
    sc.geom_texuniform = add(scene.geom_texuniform, np.zeros(n_inst, bool))
    sc.geom_mass = add(scene.geom_mass, np.zeros(n_inst))
    sc.geom_mesh = add(scene.geom_mesh if scene.geom_mesh is not None else np.full(G, -1, np.int32), which.astype(np.int32))
    sc.meshes = meshes
    return sc, int(sum(meshes[m].n_tris for m in which)), build_s


def mesh_section(args, r, fs, scene, cfg, dv, W, H):
    from render_cases import kp_rgba
    from stac_mjx_amd.render import Renderer

    n_inst = 20 if args.quick else 100
    sc, tris, build_s = mesh_bench_scene(scene, n_inst)
    meshes = sc.meshes
    pairs = cfg["KEYPOINT_MODEL_PAIRS"]
    rm = Renderer(r.engine, sc, list(pairs), list(pairs.values()), kp_rgba(cfg), float(cfg["MARKER_SIZE"]), memory_budget=16 << 30)
    N = 20 if args.quick else args.mesh_frames
    reps = (N + 49) // 50
    qpos, kp = np.tile(dv["qpos"], (reps, 1))[:N], np.tile(dv["kp_data"], (reps, 1))[:N]
    xpos, xquat, markers = rm.poses(torch.as_tensor(qpos).cuda(), dv["offsets"])
    kpt = torch.as_tensor(kp, dtype=torch.float32).cuda().reshape(N, rm.K, 3)
    rgb = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda:0")
    t = fs.tables
    out = {"instances": n_inst, "meshes": len(meshes), "triangles_over_instances": tris, "build_s": build_s, "frames": N,
           "primitives": rm.P + 3 * rm.K, "kernel": {}}
    for camera in ("close_profile", -1):
        cam, tanh = rm.cameras(camera, xpos, xquat, t.qpos0, t.body_parentid)
        n, elapsed = timed(lambda: rm.handle.render(xpos, xquat, kpt, markers, False, cam, tanh, W, H, rgb))
        fps = n * N / elapsed
        out["kernel"][f"{camera}_plain"] = {"frames_per_s": fps, "ms_per_frame": 1e3 / fps, "launches": n, "window_s": elapsed}
        print("mesh", camera, json.dumps(out["kernel"][f"{camera}_plain"]), flush=True)
    from build_render_ref import RenderRef

    ref = RenderRef("float")
    nc = 1 if args.quick else 2
    t0 = time.perf_counter()
    ref.render(rm.tables, t.nbody, xpos[:nc].cpu().numpy(), xquat[:nc].cpu().numpy(), kp[:nc], markers[:nc].cpu().numpy(), False,
               cam[:nc].cpu().numpy(), tanh, W, H)
    dt = time.perf_counter() - t0
    out["cpu_restatement_f32"] = {"frames": nc, "frames_per_s": nc / dt, "threads": int(os.environ.get("OMP_NUM_THREADS", "0") or 0)}
    print("mesh cpu_restatement_f32", json.dumps(out["cpu_restatement_f32"]), flush=True)
    rm.close()
    return out


def hierarchy_section(args, eng, W, H):
    """One icosphere of 20 480 triangles filling the frame: the hierarchy against the single-leaf upload."""
    from render_cases import look_at
    from render_mesh_cases import icosphere, static_scene
    from stac_mjx_amd.mesh import make_mesh
    from stac_mjx_amd.render import RenderSceneHandle

    m = make_mesh("ico5", icosphere(5, 0.5))
    sc = static_scene([m], [(0, [0, 0, 0.6], [1, 0, 0, 0], [0.7, 0.7, 0.9, 1], 0)], [look_at([1.3, 0.2, 0.9], [0, 0, 0.6])], K=eng.K)
    t = dict(sc[0])
    t["kp_rgba"] = np.ones((eng.K, 4), np.float32)
    xpos = np.zeros((1, eng.nbody, 3), np.float32)
    xquat = np.zeros((1, eng.nbody, 4), np.float32)
    xquat[..., 0] = 1
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    out = {"triangles": m.n_tris, "width": W, "height": H}
    pics = {}
    for name, val in (("hierarchy", "0"), ("single_leaf", "1")):
        os.environ["STAC_RENDER_MESH_SINGLE_LEAF"] = val  # read by stac_render_scene_create_with_meshes
        h = RenderSceneHandle(eng, t)
        rgb = torch.empty((1, H, W, 3), dtype=torch.uint8, device="cuda:0")
        seg = torch.empty((1, H, W), dtype=torch.int32, device="cuda:0")
        depth = torch.empty((1, H, W), dtype=torch.float32, device="cuda:0")
        a = (d(xpos), d(xquat), d(sc[3]), d(sc[4]), False, d(sc[5]), sc[6], W, H, rgb, seg, depth)
        n, elapsed = timed(lambda: h.render(*a), min_s=0.2)
        out[name + "_ms_per_launch"] = 1e3 * elapsed / n
        pics[name] = (rgb.cpu().numpy(), seg.cpu().numpy(), depth.cpu().numpy().view(np.uint32))
        h.close()
    os.environ.pop("STAC_RENDER_MESH_SINGLE_LEAF", None)
    out["pictures_equal"] = bool(all((x == y).all() for x, y in zip(pics["hierarchy"], pics["single_leaf"])))
    out["mesh_share_of_pixels"] = float((pics["hierarchy"][1] >= 0).mean())
    print("hierarchy", json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
