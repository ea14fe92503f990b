"""The render kernel (csrc/stac_render.hip) against its CPU restatement tests/tools/render_ref.c built with float: every
output (rgb, seg, depth) equal bit for bit, on the rodent's stored fit through every camera, the synth model, random scenes
of every primitive type, NaN keypoints, the primitive cap, chunked and very long batches.  Then the Python surface:
FK consistency of the pictures, Stac.render leaving the fit state alone, and viz_stac end to end."""

import math

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from render_cases import RenderRef, assert_same, gpu_render, kp_rgba, random_scene, rodent_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref32():
    return RenderRef("float")


@pytest.fixture(scope="module")
def rodent(reference_dir, rodent_cfg, rodent_setup_legacy):
    from stac_mjx_amd.engine import Engine
    from stac_mjx_amd.render import Renderer

    fs = rodent_setup_legacy
    eng = Engine(fs.tables, fs.lb, fs.ub, device="cuda:0")
    scene = rodent_scene(reference_dir, rodent_cfg)
    pairs = rodent_cfg["KEYPOINT_MODEL_PAIRS"]
    r = Renderer(eng, scene, list(pairs), list(pairs.values()), kp_rgba(rodent_cfg), float(rodent_cfg["MARKER_SIZE"]))
    return eng, scene, r, fs.tables


def check_renderer(ref32, r, tables, qpos, kp, offsets, camera, W, H, show):
    out = r.render(qpos, kp, offsets, qpos0=tables.qpos0, parent=tables.body_parentid, camera=camera, width=W, height=H,
                   show_marker_error=show, want_seg=True, want_depth=True)
    want = ref32.render(r.tables, tables.nbody, out["xpos"].cpu().numpy(), out["xquat"].cpu().numpy(), out["kp"].cpu().numpy(),
                        out["markers"].cpu().numpy(), show, out["cam"].cpu().numpy(), out["tan_half_fovy"], W, H)
    got = (out["rgb"].numpy(), out["seg"].numpy(), out["depth"].numpy())
    assert_same(got, want[:3], f"camera {camera} {W}x{H} show_error={show}")
    return out


@pytest.mark.parametrize("show", [False, True])
def test_rodent_every_camera_full_hd(ref32, rodent, demo_viz, show):
    eng, scene, r, tables = rodent
    idx = [0, 37]
    for camera in list(range(len(scene.cam_names))) + [-1]:
        out = check_renderer(ref32, r, tables, demo_viz["qpos"][idx], demo_viz["kp_data"][idx], demo_viz["offsets"], camera, 1920, 1200, show)
        assert (out["seg"].numpy() >= 0).mean() > 0.05  # the picture is not empty


@pytest.mark.parametrize("W,H", [(97, 61), (17, 300), (1, 1)])
def test_rodent_sizes_off_the_tile_grid(ref32, rodent, demo_viz, W, H):
    eng, scene, r, tables = rodent
    idx = list(range(5))
    for camera in list(range(len(scene.cam_names))) + [-1]:
        for show in (False, True):
            check_renderer(ref32, r, tables, demo_viz["qpos"][idx], demo_viz["kp_data"][idx], demo_viz["offsets"], camera, W, H, show)


def test_nan_keypoints_draw_neither_sphere_nor_segment(ref32, rodent, demo_viz):
    eng, scene, r, tables = rodent
    kp = demo_viz["kp_data"][:3].copy()
    kp[0, 0:3] = np.nan
    kp[1, 3 * 5 + 1] = np.nan
    kp[2, :] = np.nan
    out = check_renderer(ref32, r, tables, demo_viz["qpos"][:3], kp, demo_viz["offsets"], 0, 480, 300, True)
    seg = out["seg"].numpy()
    P, K = r.P, r.K
    for f, ks in ((0, [0]), (1, [5]), (2, list(range(K)))):
        for k in ks:
            assert not (seg[f] == P + k).any() and not (seg[f] == P + 2 * K + k).any()


def test_synth_model(ref32, reference_dir):
    import json

    from stac_mjx_amd.engine import Engine
    from stac_mjx_amd.fit_model import finish_fit_setup
    from stac_mjx_amd.mjcf import ModelTables, compile_render_scene
    from stac_mjx_amd.render import Renderer

    cfg = json.load(open(GOLDEN / "synth_model_cfg.json"))["model"]
    names = list(cfg["KEYPOINT_MODEL_PAIRS"].keys())
    fs = finish_fit_setup(ModelTables.load(GOLDEN / "synth_tables.npz"), cfg, names)
    eng = Engine(fs.tables, fs.lb, fs.ub, device="cuda:0")
    scene = compile_render_scene(reference_dir / "models" / "synth_model.xml", scale=float(cfg["SCALE_FACTOR"]), log=lambda *a: None)
    r = Renderer(eng, scene, names, list(cfg["KEYPOINT_MODEL_PAIRS"].values()), kp_rgba(cfg), float(cfg["MARKER_SIZE"]))
    kp = np.load(GOLDEN / "synth_kp_1.npy").reshape(-1, 3 * len(names))[:1]
    q = np.repeat(fs.tables.qpos0[None], 3, 0)
    q[1, 3:7] = [math.cos(0.3), math.sin(0.3), 0, 0]
    q[2, :3] += [0.05, 0.0, 0.02]
    kp3 = np.repeat(kp, 3, 0)
    for camera in (0, -1):
        out = check_renderer(ref32, r, fs.tables, q, kp3, fs.tables.site_pos, camera, 160, 120, True)
        if camera == 0:  # the (see-through) capsule is in the fixed camera's picture
            assert (out["rgb"].numpy()[..., 0] > 0).mean() > 0.01


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_scenes(ref32, rodent, seed):
    from stac_mjx_amd.render import RenderSceneHandle

    eng = rodent[0]
    t, xpos, xquat, kp, markers, cams, tanh = random_scene(seed, eng.nbody, eng.K, n_frames=3)
    h = RenderSceneHandle(eng, t)
    for W, H in ((160, 120), (97, 61)):
        for show in (False, True):
            got = gpu_render(h, xpos, xquat, kp, markers, show, cams, tanh, W, H)
            want = ref32.render(t, eng.nbody, xpos, xquat, kp, markers, show, cams, tanh, W, H)
            assert_same(got, want[:3], f"seed {seed} {W}x{H} show_error={show}")
    h.close()


def test_capacity_cap(ref32, rodent):
    from stac_mjx_amd.engine import StacHipError
    from stac_mjx_amd.render import MAX_PRIMS, RenderSceneHandle

    eng = rodent[0]
    n_static = MAX_PRIMS - 3 * eng.K
    t, xpos, xquat, kp, markers, cams, tanh = random_scene(7, eng.nbody, eng.K, n_static=n_static - 15, n_frames=1)
    assert len(t["prim_type"]) + 3 * eng.K == MAX_PRIMS
    h = RenderSceneHandle(eng, t)
    got = gpu_render(h, xpos, xquat, kp, markers, True, cams, tanh, 64, 48)
    assert_same(got, ref32.render(t, eng.nbody, xpos, xquat, kp, markers, True, cams, tanh, 64, 48)[:3], "at the cap")
    h.close()
    t2, *_ = random_scene(7, eng.nbody, eng.K, n_static=n_static - 14, n_frames=1)
    with pytest.raises(StacHipError) as ei:
        RenderSceneHandle(eng, t2)
    assert "error -3" in str(ei.value) and eng.lib.stac_last_error_code() == -3


def test_chunk_seams_leave_no_trace(ref32, rodent, demo_viz, rodent_cfg):
    from stac_mjx_amd.render import Renderer

    eng, scene, r, tables = rodent
    idx = list(range(7))
    args = dict(qpos0=tables.qpos0, parent=tables.body_parentid, camera=1, width=97, height=61, show_marker_error=True,
                want_seg=True, want_depth=True)
    whole = r.render(demo_viz["qpos"][idx], demo_viz["kp_data"][idx], demo_viz["offsets"], **args)
    pairs = rodent_cfg["KEYPOINT_MODEL_PAIRS"]
    small = Renderer(eng, scene, list(pairs), list(pairs.values()), kp_rgba(rodent_cfg), float(rodent_cfg["MARKER_SIZE"]),
                     memory_budget=3 * 97 * 61 * 11)  # 3 frames per launch
    chunked = small.render(demo_viz["qpos"][idx], demo_viz["kp_data"][idx], demo_viz["offsets"], **args)
    for k in ("rgb", "seg", "depth"):
        assert torch.equal(whole[k], chunked[k]), k
    check_renderer(ref32, small, tables, demo_viz["qpos"][idx], demo_viz["kp_data"][idx], demo_viz["offsets"], 1, 97, 61, True)
    small.close()


def test_more_frames_than_the_grid_z_limit(ref32, rodent):
    from stac_mjx_amd.render import RenderSceneHandle

    eng = rodent[0]
    t, xpos, xquat, kp, markers, cams, tanh = random_scene(11, eng.nbody, eng.K, n_static=20, n_frames=1, layered=False, near=False)
    N = 65535 + 5
    rng = np.random.default_rng(5)
    xpos = np.ascontiguousarray(np.repeat(xpos, N, 0) + rng.normal(scale=0.05, size=(N, 1, 3)).astype(np.float32))
    xquat, kp, markers = (np.ascontiguousarray(np.repeat(a, N, 0)) for a in (xquat, kp, markers))
    cams = np.ascontiguousarray(np.repeat(cams, N, 0))
    h = RenderSceneHandle(eng, t)
    got = gpu_render(h, xpos, xquat, kp, markers, True, cams, tanh, 8, 8)
    want = ref32.render(t, eng.nbody, xpos, xquat, kp, markers, True, cams, tanh, 8, 8)
    assert_same(got, want[:3], "N = 65540")
    assert (got[1][65535:] >= 0).any()
    h.close()


def test_outputs_fully_written_and_null_outputs(rodent):
    from stac_mjx_amd.render import RenderSceneHandle

    eng = rodent[0]
    t, xpos, xquat, kp, markers, cams, tanh = random_scene(3, eng.nbody, eng.K, n_frames=2)
    h = RenderSceneHandle(eng, t)
    rgb, seg, depth = gpu_render(h, xpos, xquat, kp, markers, True, cams, tanh, 37, 29)
    assert (seg >= -1).all() and (seg < len(t["prim_type"]) + 3 * eng.K).all()  # no sentinel int left
    assert not (depth.view(np.uint32) == 0xABABABAB).any() and not np.isnan(depth).any()
    assert (seg == -1).sum() == np.isinf(depth).sum()
    rgb_only, _, _ = gpu_render(h, xpos, xquat, kp, markers, True, cams, tanh, 37, 29, want_seg=False, want_depth=False)
    np.testing.assert_array_equal(rgb_only, rgb)
    h.close()


def test_markers_in_the_picture_are_where_fk_puts_them(rodent, demo_viz):
    eng, scene, r, tables = rodent
    idx = list(range(0, 50, 10))
    W, H = 640, 400
    for camera in (0, 2, -1):
        out = r.render(demo_viz["qpos"][idx], demo_viz["kp_data"][idx], demo_viz["offsets"], qpos0=tables.qpos0,
                       parent=tables.body_parentid, camera=camera, width=W, height=H, want_seg=True, want_depth=True)
        cam, tanh = out["cam"].double().cpu().numpy(), out["tan_half_fovy"]
        mk = out["markers"].double().cpu().numpy()
        seg, depth = out["seg"].numpy(), out["depth"].numpy()
        checked = 0
        for f in range(len(idx)):
            R = cam[f, 3:].reshape(3, 3)
            for k in range(r.K):
                q = R.T @ (mk[f, k] - cam[f, :3])
                if q[2] >= 0:
                    continue
                u, v = q[0] / -q[2], q[1] / -q[2]
                x = (u / (tanh * W / H) + 1) * W / 2 - 0.5
                y = (1 - v / tanh) * H / 2 - 0.5
                xi, yi = int(round(x)), int(round(y))
                if not (0 <= xi < W and 0 <= yi < H):
                    continue
                checked += 1
                dist = np.linalg.norm(mk[f, k] - cam[f, :3])
                assert seg[f, yi, xi] == r.P + r.K + k or depth[f, yi, xi] < dist, (camera, f, k, seg[f, yi, xi])
        assert checked > 0


def _stac_cfg(rodent_cfg, **over):
    from stac_mjx_amd.config import validate_config

    stac = dict(fit_offsets_path="fit.h5", ik_only_path="ik.h5", data_path="d.mat", continuous=False, n_fit_frames=10,
                skip_fit_offsets=False, skip_ik_only=False, infer_qvels=False, n_frames_per_clip=2,
                mujoco=dict(solver="newton", iterations=1, ls_iterations=4))
    stac.update(over)
    model = dict(rodent_cfg, MJCF_PATH="models/rodent.xml")
    return validate_config({"model": model, "stac": stac})


def test_stac_render_leaves_the_fit_state_alone(tmp_path, reference_dir, rodent_cfg, rodent_mocap):
    from stac_mjx_amd.stac import Stac

    cfg = _stac_cfg(rodent_cfg)
    stac = Stac(reference_dir / "models" / "rodent.xml", cfg, list(rodent_cfg["KEYPOINT_MODEL_PAIRS"]), verbose=False)
    kp = rodent_mocap[:4]
    off = stac.setup.tables.site_pos + 0.001
    a = stac.ik_only(kp, off)
    frames = stac.render(a.qpos, a.kp_data, a.offsets + 0.002, 3, tmp_path / "v.avi", camera="side", height=61, width=97,
                         show_marker_error=True)
    assert len(frames) == 3 and frames[0].shape == (61, 97, 3) and frames[0].dtype == np.uint8
    b = stac.ik_only(kp, off)
    for k in ("qpos", "xpos", "xquat", "marker_sites", "offsets"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)


def test_viz_stac_end_to_end(tmp_path, reference_dir, rodent_cfg, rodent_mocap):
    from stac_mjx_amd import viz_stac
    from stac_mjx_amd.io import save_data_to_h5
    from stac_mjx_amd.stac import Stac
    from stac_mjx_amd.video import read_avi

    cfg = _stac_cfg(rodent_cfg)
    names = list(rodent_cfg["KEYPOINT_MODEL_PAIRS"])
    stac = Stac(reference_dir / "models" / "rodent.xml", cfg, names, verbose=False)
    kp = rodent_mocap[:6]
    d = stac.ik_only(kp, stac.setup.tables.site_pos)
    path = save_data_to_h5(cfg, names, d.names_qpos, d.names_xpos, d.kp_data, d.marker_sites, d.offsets, d.qpos, d.xpos,
                           d.xquat, np.zeros((len(d.qpos), 73), np.float32), tmp_path / "ik.h5")
    cfg2, frames = viz_stac(path, 4, tmp_path / "out.avi", start_frame=1, camera="close_profile", height=61, width=97,
                            base_path=reference_dir, show_marker_error=True)
    avi = read_avi(tmp_path / "out.avi")
    assert avi["n_frames"] == len(avi["frames"]) == 4 and (avi["width"], avi["height"]) == (97, 61)
    t = stac.setup.tables
    want = stac._get_renderer().render(d.qpos[1:5], d.kp_data[1:5], d.offsets, qpos0=t.qpos0, parent=t.body_parentid,
                                       camera="close_profile", width=97, height=61, show_marker_error=True)
    np.testing.assert_array_equal(np.stack(frames), want["rgb"].numpy())
