"""Ground clearance (stac.ground) on the GPU: the kernel of csrc/ground/stac_ground.hip against the CPU build of its rule
(tests/ground_cases.py) at tolerance 0 on every output word, twice; on many workgroups, at its capacities and one past them, and behind
element 2^31 of xquat; Stac.ground_clearance on an ik_only run of the rodent; and run_stac with stac.ground: level."""

import json
import shutil

import numpy as np
import pytest
import torch

import ground_cases as gc
import host_scaffold as hs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return gc.cpu_rule(tmp_path_factory)


def _table(meta, data, verts, nbody, S):
    from stac_mjx_amd import ground

    return ground.GroundTable(meta=np.ascontiguousarray(meta, dtype=np.int32), data=np.ascontiguousarray(data, dtype=np.float32),
                              verts=np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3), nbody=nbody, names=[f"g{i}" for i in range(len(meta))],
                              body_names=[f"b{b}" for b in meta[:, 1]], track=[f"t{s}" for s in range(S)])


def gpu_clearance(xpos, xquat, meta, data, verts, S, z_ref, poison=float("nan")):
    """ground.ground_clearance of host arrays -> the five outputs as numpy; the allocator's blocks are filled with ``poison`` first,
    so an output word that the call leaves unwritten shows"""
    from stac_mjx_amd import ground

    N, G = xpos.shape[0], meta.shape[0]
    junk = [torch.full((n,), poison, dtype=torch.float32, device="cuda") for n in (N, N, max(N * S, 1), G, 2 * G)]
    del junk
    out = ground.ground_clearance(torch.as_tensor(xpos).cuda(), torch.as_tensor(xquat).cuda(), _table(meta, data, verts, xpos.shape[1], S), z_ref)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _twice(rule, label, *args):
    clearance, _ = rule
    want = clearance(*args)
    gc.same(gpu_clearance(*args, poison=float("nan")), want, label)
    gc.same(gpu_clearance(*args, poison=1e30), want, label + " (second call)")


# ---- kernel against the CPU rule, tolerance 0 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbody", gc.NBODIES)
def test_kernel_equals_the_rule(rule, nbody):
    for label, *args in gc.cases(nbody):
        _twice(rule, label, *args)


def test_kernel_on_the_special_cases(rule):
    for label, *args in gc.special_cases():
        _twice(rule, label, *args)


@pytest.mark.parametrize("value,where,body", gc.POISONS)
def test_kernel_with_values_that_are_not_finite(rule, value, where, body):
    label, *args = gc.poisoned(value, where, body)
    _twice(rule, label, *args)


def test_kernel_on_many_workgroups_and_body_chunks(rule):
    """512 frames are 8 workgroups of one tile, whose minima and counts meet in the atomics; 524 358 frames are 8194 tiles, three to a
    workgroup, the last one of 6 frames; 100 and 150 bodies pass through the staging rows in 3 and 4 chunks of 48"""
    _, lib = rule
    assert lib.ground_tiles(512) == 1 and lib.ground_tiles(524358) == 3
    for N, nbody, G, S, aligned in ((512, 67, 101, 2, False), (520, 5, 30, 1, True), (524358, 3, 12, 2, False), (200, 100, 150, 3, False), (70, 150, 64, 0, True)):
        xpos, xquat = gc.poses(N, nbody, N + nbody, aligned)
        meta, data, verts = gc.table(G, nbody, N + G, S, mesh_counts=(3, 17), aligned=aligned, quantised=aligned)
        _twice(rule, f"N{N}_nbody{nbody}_G{G}", xpos, xquat, meta, data, verts, S, 0.01)


def test_kernel_at_its_capacities_and_one_past_them(rule):
    """4096 geoms (with 32 slots and 67 bodies: 90 KiB of LDS, more than a launch gets by default), 4096 bodies, 2^20 vertices; one
    more of each is refused"""
    from stac_mjx_amd import ground
    from stac_mjx_amd.engine import StacHipError

    xpos, xquat = gc.poses(130, 67, 5)
    meta, data, verts = gc.table(ground.MAX_GEOMS, 67, 5, S=32, mesh_counts=(2, 5), share=True)
    _twice(rule, "G4096", xpos, xquat, meta, data, verts, 32, 0.0)
    more = np.concatenate([meta, meta[:1]]), np.concatenate([data, data[:1]])
    with pytest.raises(StacHipError, match="n_geoms = 4097 exceeds"):
        gpu_clearance(xpos, xquat, *more, verts, 32, 0.0)
    xpos, xquat = gc.poses(3, ground.MAX_BODIES, 6)
    meta, data, verts = gc.table(40, ground.MAX_BODIES, 6, S=2)
    meta[:4, 1] = (1, 47, 48, ground.MAX_BODIES - 1)
    _twice(rule, "nbody4096", xpos, xquat, meta, data, verts, 2, 0.0)
    xpos, xquat = gc.poses(3, ground.MAX_BODIES + 1, 6)
    with pytest.raises(StacHipError, match="nbody = 4097 exceeds"):
        gpu_clearance(xpos, xquat, meta, data, verts, 2, 0.0)
    xpos, xquat = gc.poses(2, 3, 7)
    meta, data, _ = gc.table(3, 3, 7, S=1)
    verts = np.random.default_rng(7).normal(0.0, 0.05, (ground.MAX_VERTS, 3)).astype(np.float32)
    meta[:, 0], meta[:, 4], meta[:, 5] = gc.MESH, (0, 1, ground.MAX_VERTS - 5), (ground.MAX_VERTS, 7, 5)
    _twice(rule, "V2^20", xpos, xquat, meta, data, verts, 1, 0.0)
    with pytest.raises(StacHipError, match="n_verts = 1048577 exceeds"):
        gpu_clearance(xpos, xquat, meta, data, np.concatenate([verts, verts[:1]]), 1, 0.0)


def test_kernel_past_2_31_elements(rule):
    """4 194 432 frames of 128 bodies: the quaternions of the last frames lie behind element 2^31 of xquat (8.6 GB; xpos 6.4 GB).
    Spheres at their bodies' origins have z_g = xpos z - size exactly, one torch subtraction: every frame's low_z and both per-geom
    outputs against torch, in slabs; the last frames against the CPU rule with every type"""
    from stac_mjx_amd import ground

    clearance, _ = rule
    N, nbody = (1 << 22) + 128, 128
    assert (N - 100) * nbody * 4 > 2**31
    xpos = torch.empty((N, nbody, 3), dtype=torch.float32, device="cuda")
    xquat = torch.empty((N, nbody, 4), dtype=torch.float32, device="cuda")
    torch.manual_seed(9)
    slab = 1 << 16
    for lo in range(0, N, slab):
        xpos[lo:lo + slab].normal_(0.0, 0.1)
        xquat[lo:lo + slab].normal_(0.0, 0.5)
    meta, data, verts = gc.table(12, nbody, 9, S=1, mesh_counts=(4,))
    meta[:3, 0], meta[:3, 1], meta[:3, 2], meta[:3, 3] = gc.SPHERE, (1, 60, 127), 1, -1
    meta[3:, 2] = 0
    data[:3, 3:6] = 0.0
    out = ground.ground_clearance(xpos, xquat, _table(meta, data, verts, nbody, 1), 0.05)
    size = torch.as_tensor(data[:3, 0]).cuda()
    gmin = torch.full((3,), float("inf"), device="cuda")
    below = torch.zeros(3, dtype=torch.int64, device="cuda")
    for lo in range(0, N, slab):
        z = xpos[lo:lo + slab][:, [1, 60, 127], 2] - size
        low, arg = z.min(dim=1)
        assert torch.equal(out["low_z"][lo:lo + slab], low), lo
        assert torch.equal(z.gather(1, out["low_geom"][lo:lo + slab].to(torch.int64)[:, None])[:, 0], low), lo
        gmin, below = torch.minimum(gmin, z.amin(dim=0)), below + (z < 0.05).sum(dim=0)
    assert torch.equal(out["geom_min"][:3], gmin) and torch.equal(out["geom_below"][:3], below)
    tail = slice(N - 70, N)
    want = clearance(xpos[tail].cpu().numpy(), xquat[tail].cpu().numpy(), meta, data, verts, 1, 0.05)
    for k in ("low_z", "low_geom", "track_z"):
        assert np.array_equal(gc.bits(out[k][tail].cpu().numpy()), gc.bits(want[k])), k


def test_wrapper_refusals_on_the_device(rule):
    from stac_mjx_amd import ground
    from stac_mjx_amd.engine import StacHipError

    xpos, xquat = gc.poses(10, 5, 3)
    meta, data, verts = gc.table(8, 5, 3, S=1)
    tab = _table(meta, data, verts, 5, 1)
    p, q = torch.as_tensor(xpos).cuda(), torch.as_tensor(xquat).cuda()
    with pytest.raises(ValueError, match="CUDA tensor"):
        ground.ground_clearance(p.cpu(), q, tab)
    with pytest.raises(ValueError, match="same frames and bodies"):
        ground.ground_clearance(p[:5], q, tab)
    bad = meta.copy()
    bad[2, 1] = 5
    with pytest.raises(StacHipError, match="geom 2: body 5 is outside"):
        ground.ground_clearance(p, q, _table(bad, data, verts, 5, 1))
    out = ground.ground_clearance(p, q, tab)  # (the refusals leave the library usable)
    clearance, _ = rule
    gc.same({k: v.cpu().numpy() for k, v in out.items()}, clearance(xpos, xquat, meta, data, verts, 1, 0.0), "after refusals")


# ---- Stac.ground_clearance and run_stac -----------------------------------------------------------------------------------------------
def _stac(xml, rodent_setup, rodent_cfg, **over):
    from stac_mjx_amd.stac import Stac

    return Stac(xml, hs.stage_cfg(rodent_cfg, **over), rodent_setup.kp_names, setup=rodent_setup, verbose=False)


def test_stac_ground_clearance_on_an_ik_only_run(rule, reference_dir, rodent_setup, rodent_cfg, rodent_mocap):
    """The rodent, 3 clips x 4 frames: the arrays and the summary against the CPU rule over the same xpos / xquat"""
    from stac_mjx_amd import ground

    clearance, _ = rule
    kp = rodent_mocap[300:312].astype(np.float32)
    stac = _stac(reference_dir / "models" / "rodent.xml", rodent_setup, rodent_cfg, n_frames_per_clip=4, ground_track=["foot_L", "foot_R"])
    data = stac.ik_only(kp, rodent_setup.tables.site_pos)
    got = stac.ground_clearance(data)
    table = stac.ground_table("fitted", None, ["foot_L", "foot_R"])
    assert table.n_geoms == 100 and int(table.include.sum()) == 47 and got["names"] == table.names
    want = clearance(data.xpos, data.xquat, table.meta, table.data, table.verts, 2, 0.0)
    gc.same(got, want, "fitted")
    summary = got["summary"]
    assert summary["n_frames"] == 12 and summary["floor_z"] == float(np.sort(want["low_z"])[0])  # (rank ceil(50 * 12 / 1000) = 1)
    assert summary == ground.summarize({k: torch.as_tensor(v) for k, v in want.items()}, table, 0.0, 50, 0.002)
    assert [t["body"] for t in summary["tracks"]] == ["foot_L", "foot_R"]
    every = stac.ground_clearance(data, geoms="all", track=[], z_ref=-0.01, permille=500)
    table = stac.ground_table("all", None, [])
    gc.same(every, clearance(data.xpos, data.xquat, table.meta, table.data, table.verts, 0, -0.01), "all")
    assert every["summary"]["floor_z"] == float(np.sort(every["low_z"])[5]) and (every["low_z"] <= got["low_z"]).all()
    with pytest.raises(ValueError, match="neither a geom nor a body"):
        stac.ground_clearance(data, geoms=["no_such_geom"])
    with pytest.raises(ValueError, match="needs the model's MJCF file"):
        _stac(None, rodent_setup, rodent_cfg).ground_clearance(data)


def _datasets(path_a, path_b):
    """(name, array in a, array in b) of every dataset of two result files of one kind"""
    if path_a.suffix == ".npz":
        with np.load(path_a, allow_pickle=False) as fa, np.load(path_b, allow_pickle=False) as fb:
            return [(n, np.asarray(fa[n]), np.asarray(fb[n])) for n in fa.files]
    from stac_mjx_amd import io

    with io.h5py.File(path_a, "r") as fa, io.h5py.File(path_b, "r") as fb:
        return [(n, np.asarray(fa[n][()]), np.asarray(fb[n][()])) for n in fa.keys()]


def test_run_stac_levels_the_result(tmp_path, reference_dir, rodent_setup, rodent_cfg, rodent_mocap):
    """ground: level against the same run without it: the sidecar is read back, the z columns of the file are the unlevelled run's
    minus floor_z in float32, and every other dataset is the unlevelled run's byte for byte"""
    from stac_mjx_amd.io import load_stac_data
    from stac_mjx_amd.main import ground_path, run_stac

    fs = rodent_setup
    (tmp_path / "models").mkdir()
    shutil.copy(reference_dir / "models" / "rodent.xml", tmp_path / rodent_cfg["MJCF_PATH"])
    kp = rodent_mocap[300:312].astype(np.float32)
    over = dict(n_fit_frames=4, n_frames_per_clip=4, postprocess="gpu", infer_qvels=True)
    cfg = hs.stage_cfg(rodent_cfg, ground="level", ground_track=["foot_L", "foot_R"], **over)
    cfg.model.N_ITERS = 1
    fit_path, ik_path = run_stac(cfg, kp, fs.kp_names, base_path=tmp_path, setup=fs)
    cfg0 = hs.stage_cfg(rodent_cfg, skip_fit_offsets=True, ik_only_path="ik0.h5", **over)
    _, ik0_path = run_stac(cfg0, kp, fs.kp_names, base_path=tmp_path, setup=fs)
    assert not ground_path(ik0_path).exists()
    stored, ik = load_stac_data(ik_path)
    stored0, ik0 = load_stac_data(ik0_path)
    summary = json.loads(ground_path(ik_path).read_text())
    floor = np.float32(summary["floor_z"])
    assert summary["mode"] == "level" and summary["level"]["floor_z"] == float(floor) and stored.stac.ground == "level"
    assert stored.stac.ground_floor_z == float(floor) and stored.stac.ground_track == ["foot_L", "foot_R"] and "ground_floor_z" not in stored0.stac
    assert summary["n_frames"] == 12 and summary["n_included"] == 47 and [t["body"] for t in summary["tracks"]] == ["foot_L", "foot_R"]
    assert float(floor) == summary["low_z"]["min"]  # (rank ceil(50 * 12 / 1000) = 1 of 12: the minimum)
    assert all(g["frames_below"] == 0 for g, h in zip(summary["level"]["geoms"], summary["geoms"]) if h["included"])  # (nothing fitted is below the minimum)
    np.testing.assert_array_equal(ik.qpos[:, 2], ik0.qpos[:, 2] - floor)
    np.testing.assert_array_equal(np.delete(ik.qpos, 2, axis=1), np.delete(ik0.qpos, 2, axis=1))
    for name in ("xpos", "marker_sites"):
        a, b = getattr(ik, name), getattr(ik0, name)
        np.testing.assert_array_equal(a[..., 2], b[..., 2] - floor, err_msg=name)
        np.testing.assert_array_equal(a[..., :2], b[..., :2], err_msg=name)
    np.testing.assert_array_equal(ik.kp_data[:, 2::3], ik0.kp_data[:, 2::3] - floor)
    np.testing.assert_array_equal(ik.kp_data[:, 0::3], ik0.kp_data[:, 0::3])
    np.testing.assert_array_equal(ik.kp_data[:, 1::3], ik0.kp_data[:, 1::3])
    # every other dataset of the file, whatever it is, byte for byte: all but the stored config and the four with a z column
    assert hs.dataset_names(ik_path) == hs.dataset_names(ik0_path) and ik_path.suffix == ik0_path.suffix
    levelled = {"qpos", "xpos", "marker_sites", "kp_data"}
    others = 0
    for name, a, b in _datasets(ik_path, ik0_path):
        if name in levelled or "config" in name.lower():
            continue
        others += 1
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert others >= 6 and levelled <= hs.dataset_names(ik_path)  # (xquat, offsets, qvel and the three name lists at the least)
    # the fit file is not touched by the stage: the same run with ground: report writes the same fit and an unlevelled result
    cfg1 = hs.stage_cfg(rodent_cfg, ground="report", skip_fit_offsets=True, ik_only_path="ik1.h5", **over)
    _, ik1_path = run_stac(cfg1, kp, fs.kp_names, base_path=tmp_path, setup=fs)
    _, ik1 = load_stac_data(ik1_path)
    for name in ("qpos", "xpos", "xquat", "marker_sites", "kp_data", "qvel"):
        np.testing.assert_array_equal(getattr(ik1, name), getattr(ik0, name), err_msg=name)
    report = json.loads(ground_path(ik1_path).read_text())
    assert report["mode"] == "report" and "level" not in report and report["floor_z"] == float(floor)
    with pytest.raises(ValueError, match="neither a geom nor a body"):
        run_stac(hs.stage_cfg(rodent_cfg, ground="report", ground_geoms=["no_such"], skip_fit_offsets=True, **over), kp, fs.kp_names, base_path=tmp_path, setup=fs)
