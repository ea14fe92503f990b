"""Ground clearance on one GPU (DESIGN.md "Ground clearance", profiles/ground/ground_bench.json): ``stac_ground_clearance`` on 10^6
rodent frames (the poses of the reference's stored fit, 50 frames, by the engine's forward kinematics, repeated) with the rodent's
table of 100 geoms and two tracked feet, and the same with one synthetic mesh geom of 10 000 vertices added, each against the same five
quantities written with torch tensor operations.

  python profiles/tools/ground_bench.py --out profiles/ground/ground_bench.json [--reps 10] [--frames 1000000]

Device events around whole calls, medians of ``--reps`` calls after 2 warm-up calls.  There is no gate.  The bytes "read and
written once" are those of both inputs whole (28 per body and frame) and of the outputs: the rule needs only the z third of ``xpos``,
but a cache line of it arrives whole.
"""

from __future__ import annotations

import argparse
import json
import sys
import tarfile
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(Path(__file__).resolve().parent)]

from select_bench import timed  # noqa: E402

SLAB = 1 << 16  # frames of a slab of the torch statement (a [frames, geoms] intermediate of 10^6 frames is 400 MB, a mesh's 40 GB)


def torch_clearance(xpos, xquat, table, z_ref):
    """The five outputs of stac_ground_clearance as torch tensor operations, in slabs of frames (values that are not finite and the
    order of -0 and +0 are not treated: timing and a comparison of bits on finite data only)"""
    meta, data, verts = table.on(xpos.device)
    body, typ = meta[:, 1].long(), meta[:, 0]
    G, S, N = meta.shape[0], table.n_slots, xpos.shape[0]
    s0, s1, s2, p0, p1, p2 = (data[None, :, i] for i in range(6))
    R = data[:, 6:].reshape(G, 3, 3)
    inc = meta[:, 2] != 0
    inf = torch.full((), float("inf"), device=xpos.device)
    index = torch.arange(G, device=xpos.device)
    out = {"low_z": torch.empty(N, device=xpos.device), "low_geom": torch.empty(N, dtype=torch.int32, device=xpos.device),
           "track_z": torch.empty((N, S), device=xpos.device), "geom_min": torch.full((G,), float("inf"), device=xpos.device),
           "geom_below": torch.zeros(G, dtype=torch.int64, device=xpos.device)}
    for lo in range(0, N, SLAB):
        q, pz = xquat[lo:lo + SLAB][:, body], xpos[lo:lo + SLAB][:, body, 2]
        w, x, y, z = q.unbind(-1)
        b0, b1, b2 = 2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)
        cz = pz + ((b0 * p0 + b1 * p1) + b2 * p2)
        r0, r1, r2 = ((b0 * R[None, :, 0, j] + b1 * R[None, :, 1, j]) + b2 * R[None, :, 2, j] for j in range(3))
        zg = cz - s0
        zg = torch.where(typ == 3, cz - (s0 + r2.abs() * s1), zg)
        zg = torch.where(typ == 4, cz - torch.sqrt(((r0 * s0) * (r0 * s0) + (r1 * s1) * (r1 * s1)) + (r2 * s2) * (r2 * s2)), zg)
        zg = torch.where(typ == 5, cz - (r2.abs() * s1 + s0 * torch.sqrt(r0 * r0 + r1 * r1)), zg)
        zg = torch.where(typ == 6, cz - ((r0.abs() * s0 + r1.abs() * s1) + r2.abs() * s2), zg)
        for g in torch.nonzero(typ == 7).flatten().tolist():
            v = verts[int(meta[g, 4]): int(meta[g, 4]) + int(meta[g, 5])]
            d = (r0[:, g, None] * v[None, :, 0] + r1[:, g, None] * v[None, :, 1]) + r2[:, g, None] * v[None, :, 2]
            zg[:, g] = cz[:, g] + d.amin(dim=1)
        masked = torch.where(inc, zg, inf)
        low = masked.amin(dim=1)
        arg = torch.where(masked == low[:, None], index, G).amin(dim=1)  # (the first index among equals, which min(dim) does not promise)
        out["low_z"][lo:lo + SLAB], out["low_geom"][lo:lo + SLAB] = low, arg.to(torch.int32)
        for s in range(S):
            out["track_z"][lo:lo + SLAB, s] = torch.where(meta[:, 3] == s, zg, inf).amin(dim=1)
        out["geom_min"] = torch.minimum(out["geom_min"], zg.amin(dim=0))
        out["geom_below"] += (zg < z_ref).sum(dim=0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--mesh-verts", type=int, default=10_000)
    args = ap.parse_args()

    from stac_mjx_amd import ground
    from stac_mjx_amd.engine import Engine
    from stac_mjx_amd.fit_model import finish_fit_setup
    from stac_mjx_amd.mjcf import ModelTables, compile_render_scene

    if not torch.cuda.is_available():
        raise SystemExit("ground_bench needs a GPU: nothing is measured without one")
    golden = ROOT / "tests" / "golden"
    mcfg = json.loads((golden / "rodent_model_cfg.json").read_text())
    fs = finish_fit_setup(ModelTables.load(golden / "rodent_tables_legacy.npz"), mcfg, list(mcfg["KEYPOINT_MODEL_PAIRS"].keys()))
    with tempfile.TemporaryDirectory() as tmp, tarfile.open(golden / "reference_fixtures.tar.xz") as tf:
        tf.extractall(tmp, **({"filter": "data"} if hasattr(tarfile, "data_filter") else {}))
        scene = compile_render_scene(Path(tmp) / "models" / "rodent.xml", scale=float(mcfg["SCALE_FACTOR"]), log=lambda *a: None)
    with np.load(golden / "demo_viz_golden.npz") as d:
        qpos, offsets = d["qpos"].astype(np.float32), d["offsets"].astype(np.float32)
    eng = Engine(fs.tables, fs.lb, fs.ub, tol=float(mcfg["FTOL"]), maxiter=int(mcfg["N_ITER_Q"]), device="cuda:0")
    eng.set_site_pos(torch.as_tensor(offsets))
    fk = eng.fk(torch.as_tensor(qpos), want=("xpos", "xquat"))
    reps = -(-args.frames // qpos.shape[0])
    xpos = fk["xpos"].repeat(reps, 1, 1)[: args.frames].contiguous()
    xquat = fk["xquat"].repeat(reps, 1, 1)[: args.frames].contiguous()
    N, nbody = int(xpos.shape[0]), int(xpos.shape[1])
    result = {"tool": "profiles/tools/ground_bench.py", "command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
              "timing": f"device events around whole calls, medians of {args.reps} calls after 2 warm-up calls", "cases": []}
    table = ground.ground_table(scene, fs.tables, "fitted", track=("foot_L", "foot_R"))
    rng = np.random.default_rng(4)
    meshed = ground.GroundTable(
        meta=np.concatenate([table.meta, np.array([[7, int(table.meta[0, 1]), 0, -1, 0, args.mesh_verts]], np.int32)]),
        data=np.concatenate([table.data, table.data[:1]]), verts=rng.normal(0.0, 0.01, (args.mesh_verts, 3)).astype(np.float32), nbody=nbody,
        names=table.names + ["synthetic_mesh"], body_names=table.body_names + [table.body_names[0]], track=list(table.track))
    for name, tab in (("rodent_100_geoms", table), (f"rodent_100_geoms_and_a_mesh_of_{args.mesh_verts}", meshed)):
        G, S, V = tab.n_geoms, tab.n_slots, int(tab.verts.shape[0])
        t_hip = timed(lambda: ground.ground_clearance(xpos, xquat, tab, 0.0), args.reps, warm=2)
        t_torch = timed(lambda: torch_clearance(xpos, xquat, tab, 0.0), max(2, args.reps // 3), warm=1)
        a, b = ground.ground_clearance(xpos, xquat, tab, 0.0), torch_clearance(xpos, xquat, tab, 0.0)
        same = {k: bool(torch.equal(a[k], b[k])) for k in a}
        nbytes = N * nbody * 28 + N * (8 + 4 * S) + G * (12 + 84) + V * 12
        entry = {"case": name, "n_frames": N, "nbody": nbody, "n_geoms": G, "n_slots": S, "n_verts": V, "stac_ground_clearance": t_hip,
                 "torch_tensor_operations": t_torch, "speedup": t_torch["ms_median"] / t_hip["ms_median"], "bytes_read_and_written_once": nbytes,
                 "GB_per_s": nbytes / (t_hip["ms_median"] * 1e-3) / 1e9, "GB_per_s_torch": nbytes / (t_torch["ms_median"] * 1e-3) / 1e9,
                 "outputs_equal_torch_bits": same, "floor_z": float(ground.floor_level(a["low_z"], 50)),
                 "frames_lowest": {tab.names[g]: int(c) for g, c in enumerate(torch.bincount(a["low_geom"].long(), minlength=G).tolist()) if c}}
        result["cases"].append(entry)
        print(json.dumps(entry), flush=True)
        if args.out:
            path = Path(args.out)
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_text(json.dumps(result, indent=1) + "\n")
    if args.out:
        print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
