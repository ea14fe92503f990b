"""Mesh geoms in the render kernel (csrc/stac_render.hip, render_kernel<true>) against the float build of
tests/tools/render_ref.c: rgb, seg and depth equal bit for bit, on random scenes that mix every primitive type with
mesh instances, the awkward cases, C. elegans with a few of its own mesh files, the primitive cap, every refusal of
stac_render_scene_create_with_meshes, one mesh of 327 680 triangles in full HD, the single-leaf developer switch, and
Stac.render / viz_stac end to end on a model with mesh geoms."""

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from render_cases import RenderRef, assert_same, gpu_render, random_scene
from render_mesh_cases import (add_meshes, awkward_scene, icosphere, library, pad_bodies, random_mesh_scene, torus, write_obj,
                               write_stl_binary)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref32():
    return RenderRef("float")


@pytest.fixture(scope="module")
def eng(rodent_setup_legacy):
    from stac_mjx_amd.engine import Engine

    fs = rodent_setup_legacy
    return Engine(fs.tables, fs.lb, fs.ub, device="cuda:0")


def check_tables(ref32, eng, scene, sizes, shows=(False, True), what=""):
    from stac_mjx_amd.render import RenderSceneHandle

    t, xpos, xquat, kp, markers, cams, tanh = scene
    h = RenderSceneHandle(eng, t)
    out = None
    for W, H in sizes:
        for show in shows:
            got = gpu_render(h, xpos, xquat, kp, markers, show, cams, tanh, W, H)
            want = ref32.render(t, xpos.shape[1], xpos, xquat, kp, markers, show, cams, tanh, W, H)
            assert_same(got, want[:3], f"{what} {W}x{H} show_error={show}")
            out = got
    h.close()
    return out


@pytest.mark.parametrize("seed,n_mesh,subdivs", [(0, 1, (0,)), (1, 12, (0, 1, 2, 3)), (2, 40, (0, 2, 4, 5)), (3, 25, (1, 3, 5))])
def test_random_scenes_with_meshes(ref32, eng, seed, n_mesh, subdivs):
    sc = random_mesh_scene(seed, eng.nbody, eng.K, n_mesh=n_mesh, subdivs=subdivs, n_frames=3)
    got = check_tables(ref32, eng, sc, ((160, 120), (97, 61)), what=f"seed {seed}")
    assert np.isin(got[1], np.flatnonzero(sc[0]["prim_type"] == 7)).any()


def test_awkward_cases(ref32, eng):
    sc = awkward_scene(3)
    t = dict(sc[0])
    t["kp_rgba"] = np.ones((eng.K, 4), np.float32)
    N = sc[1].shape[0]
    kp = np.full((N, eng.K, 3), np.nan, np.float32)
    sc = pad_bodies((t, sc[1], sc[2], kp, kp.copy(), sc[5], sc[6]), eng.nbody)
    got = check_tables(ref32, eng, sc, ((160, 120), (33, 47)), shows=(False,), what="awkward")
    assert (got[1][0] >= 0).all()  # the camera inside the shell sees its inside everywhere


def _worm(reference_dir, tmp_path):
    """C. elegans of the packed fixtures, with the five mesh files that are committed put where its XML looks for them."""
    import shutil

    from stac_mjx_amd.fit_model import finish_fit_setup
    from stac_mjx_amd.mjcf import compile_mjcf, compile_render_scene

    d = tmp_path / "celegans"
    (d / "meshes").mkdir(parents=True)
    shutil.copy(reference_dir / "models" / "celegans" / "celegans.xml", d / "celegans.xml")
    for p in sorted((GOLDEN / "meshes" / "celegans").glob("*.stl")):
        shutil.copy(p, d / "meshes" / p.name)
    bodies = ["torso1_body", "torso3_body", "torso5_body"]
    sites = {f"kp{i}": (b, [0.0, 0.0, 0.01]) for i, b in enumerate(bodies)}
    tables = compile_mjcf(d / "celegans.xml", sites=sites)
    cfg = dict(KEYPOINT_MODEL_PAIRS={k: v[0] for k, v in sites.items()})
    fs = finish_fit_setup(tables, cfg, list(sites))
    msgs = []
    scene = compile_render_scene(d / "celegans.xml", log=msgs.append)
    return fs, scene, msgs, sites


def test_celegans_with_its_own_meshes(ref32, reference_dir, tmp_path):
    from stac_mjx_amd.engine import Engine
    from stac_mjx_amd.mjcf import GEOM_MESH
    from stac_mjx_amd.render import Renderer

    fs, scene, msgs, sites = _worm(reference_dir, tmp_path)
    n_files = len(list((GOLDEN / "meshes" / "celegans").glob("*.stl")))
    assert n_files == 5 and len(scene.meshes) == 5 and (scene.geom_type == GEOM_MESH).sum() == 5
    assert scene.n_skipped == 20 and len(msgs) == 1 and "20 mesh" in msgs[0]  # 25 mesh geoms, 5 files
    e = Engine(fs.tables, fs.lb, fs.ub, device="cuda:0")
    r = Renderer(e, scene, list(sites), [v[0] for v in sites.values()], np.tile([0.0, 0.5, 1.0, 1.0], (3, 1)), 0.004)
    q = np.repeat(fs.tables.qpos0[None], 2, 0).astype(np.float32)
    q[1, 7:12] = [0.4, -0.5, 0.6, -0.4, 0.3]
    out0 = Engine.fk(e, torch.as_tensor(q), want=("site_xpos",))["site_xpos"].cpu().numpy()
    kp = (out0 + 0.002).reshape(2, -1)
    W, H = 320, 200
    res = r.render(q, kp, fs.tables.site_pos, qpos0=fs.tables.qpos0, parent=fs.tables.body_parentid, camera=-1, width=W, height=H,
                   show_marker_error=True, want_seg=True, want_depth=True)
    want = ref32.render(r.tables, fs.tables.nbody, res["xpos"].cpu().numpy(), res["xquat"].cpu().numpy(), res["kp"].cpu().numpy(),
                        res["markers"].cpu().numpy(), True, res["cam"].cpu().numpy(), res["tan_half_fovy"], W, H)
    assert_same((res["rgb"].numpy(), res["seg"].numpy(), res["depth"].numpy()), want[:3], "celegans")
    # the worm's mesh geoms are see-through (moving bodies): make them opaque to find them in seg
    t = dict(r.tables)
    t["prim_flags"] = np.zeros_like(t["prim_flags"])
    from stac_mjx_amd.render import RenderSceneHandle

    h = RenderSceneHandle(e, t)
    got = gpu_render(h, res["xpos"].cpu().numpy(), res["xquat"].cpu().numpy(), res["kp"].cpu().numpy(), res["markers"].cpu().numpy(),
                     False, res["cam"].cpu().numpy(), res["tan_half_fovy"], W, H)
    h.close()
    for i in np.flatnonzero(t["prim_type"] == 7):
        assert r.names[i].startswith("torso") and (got[1] == i).any(), r.names[i]
    r.close()


def test_the_last_of_512_primitives_is_a_mesh(ref32, eng):
    from stac_mjx_amd.render import MAX_PRIMS

    n_static = MAX_PRIMS - 3 * eng.K
    t, xpos, xquat, kp, markers, cams, tanh = random_scene(7, eng.nbody, eng.K, n_static=n_static - 16, n_frames=1)
    lib = library((2,))
    c0 = cams[0].astype(np.float64)
    fwd = -c0[3:].reshape(3, 3)[:, 2]
    t = add_meshes(t, lib, [0], [0], [c0[:3] + 0.3 * fwd], [[1, 0, 0, 0]], [[0.9, 0.2, 0.2, 1]], [0])
    assert len(t["prim_type"]) + 3 * eng.K == MAX_PRIMS and t["prim_type"][-1] == 7
    got = check_tables(ref32, eng, (t, xpos, xquat, kp, markers, cams, tanh), ((64, 48),), shows=(True,), what="at the cap")
    assert (got[1] == len(t["prim_type"]) - 1).any()


def test_refusals(eng):
    from stac_mjx_amd.engine import StacHipError
    from stac_mjx_amd.render import MAX_PRIMS, RenderSceneHandle

    base = random_mesh_scene(5, eng.nbody, eng.K, n_mesh=3, subdivs=(1, 2), n_static=10, n_frames=1)[0]

    def refused(edit, code, word):
        t = dict(base)
        t["meshes"] = {k: np.array(v, copy=True) for k, v in base["meshes"].items()}
        edit(t)
        with pytest.raises(StacHipError) as ei:
            RenderSceneHandle(eng, t)
        assert f"error {code}" in str(ei.value) and word in str(ei.value), str(ei.value)
        assert eng.lib.stac_last_error_code() == code

    RenderSceneHandle(eng, base).close()  # the unedited scene is accepted
    first_mesh_prim = int(np.flatnonzero(base["prim_type"] == 7)[0])
    m0 = base["meshes"]
    leaf = int(np.flatnonzero(m0["node_link"][:, 2] > 0)[0])
    inner = int(np.flatnonzero(m0["node_link"][: m0["node_offset"][1], 2] == 0)[0])

    def no_meshes(t):
        del t["meshes"]  # stac_render_scene_create keeps refusing type 7

    refused(no_meshes, -1, "bad type")
    refused(lambda t: t["meshes"]["prim_mesh"].__setitem__(first_mesh_prim, -1), -1, "mesh index")
    refused(lambda t: t["meshes"]["prim_mesh"].__setitem__(first_mesh_prim, 99), -1, "mesh index")
    refused(lambda t: t["meshes"]["node_link"].__setitem__((inner, 0), inner), -1, "skip link")  # not forward
    refused(lambda t: t["meshes"]["node_link"].__setitem__((inner, 0), 10**6), -1, "skip link")  # past the mesh's nodes
    refused(lambda t: t["meshes"]["node_link"].__setitem__((leaf, 0), leaf + 2), -1, "skip link")  # a leaf's is the next node
    refused(lambda t: t["meshes"]["node_link"].__setitem__((leaf, 1), 10**6), -1, "leaf range")
    refused(lambda t: t["meshes"]["node_link"].__setitem__((leaf, 1), -1), -1, "leaf range")
    refused(lambda t: t["meshes"]["node_link"].__setitem__((leaf, 2), 10**6), -1, "leaf range")

    def too_many_triangles(t):  # one mesh of 2^20 + 1 (zero-area) triangles under a single leaf
        n = (1 << 20) + 1
        t["meshes"] = dict(node_offset=np.array([0, 1], np.int32), tri_offset=np.array([0, n], np.int32),
                           node_box=np.array([[0, 0, 0, 1, 1, 1]], np.float32), node_link=np.array([[1, 0, n]], np.int32),
                           tri_vertex=np.zeros((n, 3, 3), np.float32), prim_mesh=np.where(base["prim_type"] == 7, 0, -1).astype(np.int32))

    refused(too_many_triangles, -3, "STAC_RENDER_MAX_MESH_TRIS")
    # a mesh instance is one primitive: the cap counts instances, not triangles
    t, *_ = random_scene(7, eng.nbody, eng.K, n_static=MAX_PRIMS - 3 * eng.K - 15, n_frames=1)
    t = add_meshes(t, library((0,)), [0], [0], [[0, 0, 0]], [[1, 0, 0, 0]], [[1, 1, 1, 1]], [0])
    with pytest.raises(StacHipError) as ei:
        RenderSceneHandle(eng, t)
    assert "error -3" in str(ei.value)


def test_one_large_mesh_in_full_hd_through_the_renderer(ref32, rodent_setup_legacy, rodent_cfg, tmp_path):
    """Icosphere at subdivision 7 (327 680 triangles) on the rodent's torso, 1920 x 1200, through Renderer.render."""
    from stac_mjx_amd.engine import Engine
    from stac_mjx_amd.mesh import MAX_TRIS
    from stac_mjx_amd.mjcf import compile_render_scene
    from stac_mjx_amd.render import Renderer

    tri = icosphere(7, 0.05)
    assert len(tri) == 327680 <= MAX_TRIS
    write_stl_binary(tmp_path / "big.stl", tri)
    xml = ('<mujoco><asset><mesh name="big" file="big.stl"/></asset><worldbody><light dir="0 0 -1"/>'
           '<geom type="plane" size="1 1 0.1"/><camera name="c" pos="0 -0.3 0.1" xyaxes="1 0 0 0 0 1"/>'
           '<body name="b" pos="0 0 0.1"><freejoint/><geom type="mesh" mesh="big" rgba="0.3 0.6 0.9 1"/><site name="s" pos="0 0 0.06"/>'
           '</body></worldbody></mujoco>')
    (tmp_path / "big.xml").write_text(xml)
    from stac_mjx_amd.fit_model import finish_fit_setup
    from stac_mjx_amd.mjcf import compile_mjcf

    tables = compile_mjcf(tmp_path / "big.xml", sites={"kp0": ("b", [0, 0, 0.06])})
    fs = finish_fit_setup(tables, dict(KEYPOINT_MODEL_PAIRS={"kp0": "b"}), ["kp0"])
    e = Engine(fs.tables, fs.lb, fs.ub, device="cuda:0")
    scene = compile_render_scene(tmp_path / "big.xml", log=lambda *a: None)
    r = Renderer(e, scene, ["kp0"], ["b"], [[1, 0, 0, 1]], 0.004)
    q = np.array([[0, 0, 0.1, 1, 0, 0, 0], [0.02, 0, 0.12, 0.9, 0.1, 0.3, 0.2]], np.float32)
    kp = np.array([[0, 0, 0.17], [0.02, 0.0, 0.19]], np.float32)
    W, H = 1920, 1200
    res = r.render(q, kp, fs.tables.site_pos, qpos0=fs.tables.qpos0, parent=fs.tables.body_parentid, camera="c", width=W, height=H,
                   show_marker_error=True, want_seg=True, want_depth=True)
    want = ref32.render(r.tables, fs.tables.nbody, res["xpos"].cpu().numpy(), res["xquat"].cpu().numpy(), res["kp"].cpu().numpy(),
                        res["markers"].cpu().numpy(), True, res["cam"].cpu().numpy(), res["tan_half_fovy"], W, H)
    assert_same((res["rgb"].numpy(), res["seg"].numpy(), res["depth"].numpy()), want[:3], "subdivision 7")
    assert (res["rgb"].numpy()[..., 2] > 60).mean() > 0.05  # the (see-through) sphere is in the picture
    r.close()


SINGLE_LEAF_SCRIPT = """
import sys, time, json
import numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests"); sys.path.insert(0, {root!r} + "/tests/tools")
from stac_mjx_amd.engine import Engine
from stac_mjx_amd.fit_model import finish_fit_setup
from stac_mjx_amd.mjcf import ModelTables
from stac_mjx_amd.render import RenderSceneHandle
from render_cases import gpu_render
from render_mesh_cases import big_sphere_scene
cfg = json.load(open({golden!r} + "/rodent_model_cfg.json"))
fs = finish_fit_setup(ModelTables.load({golden!r} + "/rodent_tables_legacy.npz"), cfg, list(cfg["KEYPOINT_MODEL_PAIRS"]))
eng = Engine(fs.tables, fs.lb, fs.ub, device="cuda:0")
t, xpos, xquat, kp, markers, cams, tanh = big_sphere_scene(eng, 5)
h = RenderSceneHandle(eng, t)
W, H = 640, 400
got = gpu_render(h, xpos, xquat, kp, markers, False, cams, tanh, W, H)
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
rgb = torch.empty((2, H, W, 3), dtype=torch.uint8, device="cuda:0")
d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")
a = [d(xpos), d(xquat), d(kp), d(markers), False, d(cams), tanh, W, H, rgb, None, None]
h.render(*a); torch.cuda.synchronize()
ev0.record(); h.render(*a); ev1.record(); torch.cuda.synchronize()
np.savez({out!r}, rgb=got[0], seg=got[1], depth=got[2], ms=ev0.elapsed_time(ev1))
"""


def test_the_hierarchy_prunes(tmp_path):
    """One 20 480-triangle icosphere filling the frame: with STAC_RENDER_MESH_SINGLE_LEAF=1 (every mesh uploaded as one leaf
    over all its triangles) the pictures are the same and the launch is slower.  The switch is read at scene creation in a
    process of its own, so each variant runs in a fresh child process."""
    res = {}
    for name, env in (("bvh", {}), ("single", {"STAC_RENDER_MESH_SINGLE_LEAF": "1"})):
        out = tmp_path / f"{name}.npz"
        script = tmp_path / f"{name}.py"
        script.write_text(SINGLE_LEAF_SCRIPT.format(root=str(ROOT), golden=str(GOLDEN), out=str(out)))
        p = subprocess.run([sys.executable, str(script)], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout + p.stderr
        res[name] = np.load(out)
    for k in ("rgb", "seg", "depth"):
        a, b = res["bvh"][k], res["single"][k]
        assert (a.view(np.uint32) != b.view(np.uint32)).sum() == 0 if k == "depth" else (a != b).sum() == 0, k
    print(f"640 x 400 x 2 frames, 20 480 triangles: hierarchy {float(res['bvh']['ms']):.3f} ms, single leaf {float(res['single']['ms']):.3f} ms")
    assert (res["bvh"]["seg"] >= 0).mean() > 0.5
    assert float(res["bvh"]["ms"]) < float(res["single"]["ms"])


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def _mesh_synth_model(reference_dir, tmp_path):
    """The synth model with a mesh asset, a mesh geom in group 0 and one in group 1; its config."""
    from stac_mjx_amd.config import validate_config

    xml = (reference_dir / "models" / "synth_model.xml").read_text()
    xml = xml.replace("<worldbody>", '<asset><mesh name="blob" file="blob.stl"/><mesh file="ring.obj"/></asset>\n  <worldbody>')
    xml = xml.replace('<geom fromto="0 0 0 0 0 -.25" rgba="1 1 0 1"/>',
                      '<geom fromto="0 0 0 0 0 -.25" rgba="1 1 0 1"/>\n      <geom name="blob" type="mesh" mesh="blob" pos="0 0 0.05" rgba="0 1 0 1"/>'
                      '\n      <geom name="ring" type="mesh" mesh="ring" group="1" pos="0 0 -0.1" rgba="1 0 1 1"/>')
    assert xml.count("mesh=") == 2
    (tmp_path / "models").mkdir()
    (tmp_path / "models" / "synth_mesh.xml").write_text(xml)
    write_stl_binary(tmp_path / "models" / "blob.stl", icosphere(2, 0.05))
    write_obj(tmp_path / "models" / "ring.obj", torus(0.08, 0.015))
    cfg = json.load(open(GOLDEN / "synth_model_cfg.json"))
    cfg["model"]["MJCF_PATH"] = "models/synth_mesh.xml"
    return tmp_path / "models" / "synth_mesh.xml", validate_config({"model": cfg["model"], "stac": dict(cfg["stac"], continuous=False)})


def test_stac_render_and_viz_stac_with_mesh_geoms(ref32, tmp_path, reference_dir):
    from stac_mjx_amd import viz_stac
    from stac_mjx_amd.io import save_data_to_h5
    from stac_mjx_amd.stac import Stac
    from stac_mjx_amd.video import read_avi

    xml, cfg = _mesh_synth_model(reference_dir, tmp_path)
    names = list(cfg.model.KEYPOINT_MODEL_PAIRS)
    stac = Stac(xml, cfg, names, verbose=False)
    kp = np.repeat(np.load(GOLDEN / "synth_kp_1.npy").reshape(-1, 3 * len(names))[:1], 4, 0)
    kp = kp + np.linspace(0, 0.03, 4)[:, None].astype(kp.dtype)
    off = stac.setup.tables.site_pos
    a = stac.ik_only(kp, off)
    frames = stac.render(a.qpos, a.kp_data, a.offsets, 3, tmp_path / "v.avi", camera="fixed", height=120, width=160, show_marker_error=True)
    assert len(frames) == 3 and frames[0].shape == (120, 160, 3)
    r = stac._get_renderer()
    assert "blob" in r.names and "ring" not in r.names and r.tables["prim_type"][r.names.index("blob")] == 7
    t = stac.setup.tables
    out = r.render(a.qpos[:3], a.kp_data[:3], a.offsets, qpos0=t.qpos0, parent=t.body_parentid, camera="fixed", width=160, height=120,
                   show_marker_error=True, want_seg=True, want_depth=True)
    np.testing.assert_array_equal(np.stack(frames), out["rgb"].numpy())
    want = ref32.render(r.tables, t.nbody, out["xpos"].cpu().numpy(), out["xquat"].cpu().numpy(), out["kp"].cpu().numpy(),
                        out["markers"].cpu().numpy(), True, out["cam"].cpu().numpy(), out["tan_half_fovy"], 160, 120)
    assert_same((out["rgb"].numpy(), out["seg"].numpy(), out["depth"].numpy()), want[:3], "synth model with meshes")
    green = (frames[0][..., 1].astype(int) - frames[0][..., 0].astype(int)) > 20  # the see-through green blob
    assert green.mean() > 0.005
    b = stac.ik_only(kp, off)  # the fit state is as it was
    for k in ("qpos", "xpos", "xquat", "marker_sites", "offsets"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)
    # geom_groups: the group-1 ring appears, ids shift by document order
    frames1 = stac.render(a.qpos, a.kp_data, a.offsets, 3, tmp_path / "v1.avi", camera="fixed", height=120, width=160, geom_groups=(0, 1, 2))
    r1 = stac._get_renderer((0, 1, 2))
    assert r1.names.index("ring") == r1.names.index("blob") + 1
    magenta = lambda f: ((f[..., 0].astype(int) - f[..., 1].astype(int)) > 20) & ((f[..., 2].astype(int) - f[..., 1].astype(int)) > 20)
    assert magenta(frames1[0]).mean() > 0.002 and magenta(frames[0]).sum() == 0
    # viz_stac end to end, default groups and geom_groups
    path = save_data_to_h5(cfg, names, a.names_qpos, a.names_xpos, a.kp_data, a.marker_sites, a.offsets, a.qpos, a.xpos, a.xquat,
                           np.zeros((len(a.qpos), 6), np.float32), tmp_path / "ik.h5")
    _, vf = viz_stac(path, 3, tmp_path / "out.avi", camera="fixed", height=120, width=160, base_path=tmp_path, show_marker_error=True)
    np.testing.assert_array_equal(np.stack(vf), np.stack(frames))
    avi = read_avi(tmp_path / "out.avi")
    assert avi["n_frames"] == 3 and (avi["width"], avi["height"]) == (160, 120)
    _, vf1 = viz_stac(path, 3, tmp_path / "out1.avi", camera="fixed", height=120, width=160, base_path=tmp_path, geom_groups=(0, 1, 2))
    np.testing.assert_array_equal(np.stack(vf1), np.stack(frames1))
