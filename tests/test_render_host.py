"""Rendering on the CPU: the scene compile, the camera rule, the two builds of the CPU restatement of the render kernel
(tests/tools/render_ref.c, float and double) against each other and against closed forms, the AVI writer, and the argument
checks of Stac.render / viz_stac.  No GPU."""

import math
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from render_cases import (AMB_CAP, RenderRef, compare_builds, load_demo_viz, picture_digests, qpos0_pose, random_scene,
                          rodent_frames, rodent_render_args, rodent_scene)


@pytest.fixture(scope="module")
def refs():
    return RenderRef("float"), RenderRef("double")


@pytest.fixture(scope="module")
def rodent(reference_dir, rodent_cfg):
    return rodent_scene(reference_dir, rodent_cfg)


# ---- scene compile -----------------------------------------------------------------------------------------------------------
def test_rodent_scene_contents(reference_dir, rodent, rodent_cfg):
    from stac_mjx_amd.mjcf import compile_mjcf

    s = rodent
    types_, counts = np.unique(s.geom_type, return_counts=True)
    assert dict(zip(types_.tolist(), counts.tolist())) == {0: 1, 2: 46, 3: 25, 4: 22, 6: 7}  # plane, sphere, capsule, ellipsoid, box
    groups, counts = np.unique(s.geom_group, return_counts=True)
    assert dict(zip(groups.tolist(), counts.tolist())) == {0: 1, 1: 6, 2: 94}
    assert len(s.geom_names) == 101 and s.n_skipped == 0
    assert np.isin(s.geom_group, (0, 2)).sum() == 95
    t = compile_mjcf(reference_dir / "models" / "rodent.xml", scale=float(rodent_cfg["SCALE_FACTOR"]))
    assert s.body_names == t.body_names and s.nbody == t.nbody
    gi = s.geom_names.index("collision_torso")
    assert s.body_names[s.geom_body[gi]] == "torso" and s.geom_type[gi] == 4
    a = 0.1745329251994329 / 2  # euler="0 0.1745329251994329 0" (radians): a rotation about y
    np.testing.assert_allclose(s.geom_quat[gi], [math.cos(a), 0, math.sin(a), 0], atol=1e-15)
    assert s.geom_group[s.geom_names.index("vertebra_1_collision")] == 2  # class no_collision -> group 2
    assert s.geom_group[s.geom_names.index("floor")] == 0 and s.geom_checker[s.geom_names.index("floor")]
    assert s.cam_names == ["close_profile", "back", "side", "side_alt", "top", "egocentric"]
    assert s.cam_mode == ["trackcom"] * 5 + ["fixed"] and s.cam_fovy[4] == 100.0 and s.cam_fovy[0] == 45.0
    assert (s.azimuth, s.elevation, s.alpha) == (120.0, -20.0, 0.3)
    np.testing.assert_array_equal(s.light_dir, [[0.0, 0.0, -1.0]])


def test_synth_capsule_fromto_and_mass(reference_dir):
    from stac_mjx_amd.mjcf import compile_render_scene

    s = compile_render_scene(reference_dir / "models" / "synth_model.xml")
    assert len(s.geom_names) == 1 and s.geom_type[0] == 3 and s.body_names[s.geom_body[0]] == "base"
    np.testing.assert_allclose(s.geom_pos[0], [0, 0, -0.125], atol=1e-15)
    assert s.geom_size[0, 0] == 0.02 and abs(s.geom_size[0, 1] - 0.125) < 1e-15
    # the capsule's axis (local z rotated by its quat) is along the fromto direction (up to sign)
    w, x, y, z = s.geom_quat[0]
    axis = [2 * (x * z + w * y), 2 * (y * z - w * x), w * w - x * x - y * y + z * z]
    np.testing.assert_allclose(np.abs(axis), [0, 0, 1], atol=1e-15)
    r, h = 0.02, 0.125
    assert abs(s.geom_mass[0] - 1000.0 * (math.pi * r * r * 2 * h + 4.0 / 3.0 * math.pi * r ** 3)) < 1e-12
    assert abs(s.body_mass[1] - s.geom_mass[0]) < 1e-15
    assert s.cam_names == ["fixed"] and s.cam_body[0] == 0 and len(s.light_dir) == 1


def test_scale_factor_scales_exactly_the_geoms_of_scaled_bodies(reference_dir):
    from stac_mjx_amd.mjcf import compile_render_scene

    a = compile_render_scene(reference_dir / "models" / "rodent.xml", scale=1.0)
    b = compile_render_scene(reference_dir / "models" / "rodent.xml", scale=0.9)
    scaled = a.geom_body >= 2  # dm_scale_spec: every body strictly below the first top-level body ("walker" = 1)
    assert scaled.sum() == 100 and not scaled[a.geom_names.index("floor")]
    np.testing.assert_array_equal(b.geom_size[scaled], a.geom_size[scaled] * 0.9)
    np.testing.assert_array_equal(b.geom_pos[scaled], a.geom_pos[scaled] * 0.9)
    np.testing.assert_array_equal(b.geom_size[~scaled], a.geom_size[~scaled])
    np.testing.assert_array_equal(b.geom_pos[~scaled], a.geom_pos[~scaled])
    np.testing.assert_array_equal(b.geom_quat, a.geom_quat)


def test_other_geom_types_and_camera_modes_are_refused():
    from stac_mjx_amd.mjcf import MjcfError, compile_render_scene

    msgs = []
    s = compile_render_scene('<mujoco><worldbody><geom type="mesh" mesh="m"/><geom type="hfield"/><geom size="0.1"/></worldbody></mujoco>',
                             from_string=True, log=msgs.append)
    assert s.n_skipped == 2 and len(s.geom_names) == 1 and len(msgs) == 1
    with pytest.raises(MjcfError):
        compile_render_scene('<mujoco><worldbody><geom type="sdf"/></worldbody></mujoco>', from_string=True)
    with pytest.raises(MjcfError, match="targetbody"):
        compile_render_scene('<mujoco><worldbody><camera mode="targetbody"/></worldbody></mujoco>', from_string=True)


# ---- cameras ---------------------------------------------------------------------------------------------------------------------
CAM_XML = """
<mujoco><worldbody>
  <body name="a" pos="0 0 1"><freejoint/>
    <geom type="sphere" size="0.1" mass="2"/>
    <camera name="cf" mode="fixed" pos="1 0 0" xyaxes="0 1 0 0 0 1"/>
    <camera name="ct" mode="track" pos="1 0 0" xyaxes="0 1 0 0 0 1"/>
    <camera name="cc" mode="trackcom" pos="1 0 0" xyaxes="0 1 0 0 0 1"/>
    <body name="b" pos="1 0 0"><joint type="hinge"/><geom type="sphere" size="0.1" mass="2"/></body>
  </body>
</worldbody></mujoco>"""


def test_fixed_track_trackcom_against_hand_derived_poses():
    from stac_mjx_amd.mjcf import compile_render_scene
    from stac_mjx_amd.render import camera_frames

    s = compile_render_scene(CAM_XML, from_string=True)
    parent = np.array([0, 0, 1])
    x0 = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 1]], np.float64)
    q0 = np.array([[1, 0, 0, 0]] * 3, np.float64)
    h = math.sqrt(0.5)
    xpos = torch.tensor([[[0, 0, 0], [2, 3, 1], [2, 4, 1]]], dtype=torch.float64)  # body a rotated 90 deg about z
    xquat = torch.tensor([[[1, 0, 0, 0], [h, 0, 0, h], [h, 0, 0, h]]], dtype=torch.float64)
    Rl = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float64)  # columns x = (0 1 0), y = (0 0 1), z = (1 0 0)
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    want = {0: ([2, 4, 1], Rz @ Rl), 1: ([3, 3, 1], Rl), 2: ([2.5, 3.5, 1], Rl)}
    for c, (p, R) in want.items():
        cam, tanh = camera_frames(s, parent, c, xpos, xquat, x0, q0)
        np.testing.assert_allclose(cam[0, :3].numpy(), p, atol=1e-12)
        np.testing.assert_allclose(cam[0, 3:].numpy().reshape(3, 3), R, atol=1e-12)
        assert abs(tanh - math.tan(math.radians(22.5))) < 1e-15


def test_trackcom_follows_a_translated_root(rodent, rodent_cfg):
    from stac_mjx_amd.mjcf import ModelTables
    from stac_mjx_amd.render import camera_frames

    tables = ModelTables.load(GOLDEN / "rodent_tables_legacy.npz")
    dv = load_demo_viz()
    xpos, xquat, _, _ = rodent_frames(tables, dv, [3])
    x0, q0 = qpos0_pose(tables)
    xp = torch.tensor(xpos, dtype=torch.float64)
    xq = torch.tensor(xquat, dtype=torch.float64)
    shift = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)
    for c in range(5):  # the five trackcom cameras
        a, _ = camera_frames(rodent, tables.body_parentid, c, xp, xq, x0, q0)
        b, _ = camera_frames(rodent, tables.body_parentid, c, xp + shift, xq, x0, q0)
        np.testing.assert_allclose((b[0, :3] - a[0, :3]).numpy(), [1, 0, 0], rtol=0, atol=1e-12)
        assert torch.equal(a[0, 3:], b[0, 3:])


def test_free_camera_rule(rodent):
    from stac_mjx_amd.mjcf import ModelTables
    from stac_mjx_amd.render import FREE_CAMERA_DISTANCE, camera_frames

    tables = ModelTables.load(GOLDEN / "rodent_tables_legacy.npz")
    xpos, xquat, _, _ = rodent_frames(tables, load_demo_viz(), [0, 20])
    cam, tanh = camera_frames(rodent, tables.body_parentid, -1, torch.tensor(xpos), torch.tensor(xquat))
    assert torch.equal(cam[0], cam[1])  # fixed for the call, from the first frame
    pts = torch.tensor(xpos[0, 1:], dtype=torch.float64)
    c = pts.mean(0)
    s = float((pts - c).norm(dim=-1).max())
    R = cam[0, 3:].reshape(3, 3)
    az, el = math.radians(120.0), math.radians(-20.0)
    fwd = torch.tensor([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)], dtype=torch.float64)
    np.testing.assert_allclose(R[:, 2].numpy(), (-fwd).numpy(), atol=1e-12)
    np.testing.assert_allclose(cam[0, :3].numpy(), (c - FREE_CAMERA_DISTANCE * s / tanh * fwd).numpy(), atol=1e-12)
    np.testing.assert_allclose((R.T @ R).numpy(), np.eye(3), atol=1e-12)
    assert abs(float(R[2, 0])) < 1e-12  # no roll: the x axis is horizontal
    assert abs(tanh - math.tan(math.radians(22.5))) < 1e-15


# ---- the checker: float build vs double build -------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_f32_checker_matches_f64_on_random_scenes(refs, seed):
    t, xpos, xquat, kp, markers, cams, tanh = random_scene(seed, 67, 23, n_frames=3)
    for show in (False, True):
        compare_builds(refs, (t, 67, xpos, xquat, kp, markers, show, cams, tanh, 320, 240))


@pytest.mark.parametrize("camera", [0, 2, 4, 5, -1])
def test_f32_checker_matches_f64_on_rodent_frames(refs, rodent, rodent_cfg, camera):
    a, _ = compare_builds(refs, rodent_render_args(rodent, rodent_cfg, camera))
    assert (a[1] >= 0).mean() > 0.05


def test_pictures_of_the_mesh_free_scenes_are_pinned(rodent, rodent_cfg):
    """rgb, seg, depth and amb of ``render_cases.pinned_scenes``, float and double build, against the SHA-256 digests of
    tests/golden/render_ref_digests.json: the pictures of the mesh-free restatement that the mesh-free kernel was validated
    against, before it and the mesh-aware one became one file.  The restatement uses only IEEE + - * /, sqrt, floor, fmax
    and fmin with contraction off and nothing is reduced across threads, so the bytes do not depend on the machine.  The
    random scenes pin the checker alone; the rodent frames also pin ``compile_render_scene`` and ``render_tables`` on the
    rodent, on purpose: a change there is a change of the pictures.  The file is regenerated
    (tests/golden/make_fixtures.py --only render_digests) only when the frame rule is changed on purpose."""
    import json

    want = json.load(open(GOLDEN / "render_ref_digests.json"))
    want.pop("_made_by")
    got = picture_digests(rodent, rodent_cfg)
    assert sorted(got) == sorted(want)
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{len(bad)} of {len(want)} digests differ: {bad[:8]}"


# ---- closed forms --------------------------------------------------------------------------------------------------------------
def _single(prim_type, size, pos, rgb=(0.8, 0.3, 0.9), lights=False):
    f32 = lambda v: np.asarray(v, np.float32)
    return dict(
        prim_type=np.array([prim_type], np.int32), prim_body=np.array([0], np.int32), prim_flags=np.array([0], np.int32),
        prim_size=f32([size]), prim_pos=f32([pos]), prim_quat=f32([[1, 0, 0, 0]]), prim_rgba=f32([list(rgb) + [1]]),
        prim_rgb2=f32([[0, 0, 0]]), prim_texrepeat=f32([[1, 1]]), kp_rgba=np.zeros((0, 4), np.float32),
        marker_rgba=f32([0, 0, 0, 1]), segment_rgba=f32([1, 0, 0, 1]), marker_radius=np.float32(0.005),
        segment_radius=np.float32(0.001), light_dir=f32([[0, 0, -1]] if lights else np.zeros((0, 3))),
        light_diffuse=f32([[0.7] * 3] if lights else np.zeros((0, 3))), head_ambient=f32([0.1] * 3), head_diffuse=f32([0.4] * 3),
        alpha=np.float32(0.3), background=f32([0, 0, 0]),
    )


def _axis_camera(W, H, fovy=45.0):
    cam = np.concatenate([[0, 0, 0], np.eye(3).reshape(9)]).astype(np.float32)[None]  # at the origin, looking along -z
    return cam, math.tan(math.radians(fovy) / 2)


def _pixel_dirs(W, H, tanh):
    x = (np.arange(W) + 0.5) * 2 / W - 1
    y = 1 - (np.arange(H) + 0.5) * 2 / H
    return np.meshgrid(x * tanh * W / H, y * tanh)  # u [H, W], v [H, W]


BODY0 = (np.zeros((1, 1, 3), np.float32), np.array([[[1, 0, 0, 0]]], np.float32))


@pytest.mark.parametrize("real", ["float", "double"])
def test_sphere_on_the_axis(refs, real):
    ref = refs[0] if real == "float" else refs[1]
    W, H, D, r = 161, 121, 1.0, 0.05
    t = _single(2, [r, 0, 0], [0, 0, -D])
    cam, tanh = _axis_camera(W, H)
    rgb, seg, depth, _ = ref.render(t, 1, *BODY0, None, None, False, cam, tanh, W, H)
    amb = refs[1].render(t, 1, *BODY0, None, None, False, cam, tanh, W, H)[3][0].astype(bool)
    u, v = _pixel_dirs(W, H, tanh)
    inside = (u * u + v * v) / (1 + u * u + v * v) < (r / D) ** 2  # the pixel-centre ray's angle to the axis < asin(r / D)
    assert inside.sum() > 100
    np.testing.assert_array_equal((seg[0] == 0)[~amb], inside[~amb])
    assert amb.mean() <= AMB_CAP
    cy, cx = H // 2, W // 2
    assert abs(float(depth[0, cy, cx]) - (D - r)) <= 1e-6 * D
    # headlight only: ambient 0.1 + diffuse 0.4 x cos(0)
    want = np.floor(np.array([0.8, 0.3, 0.9]) * 0.5 * 255 + 0.5)
    np.testing.assert_array_equal(rgb[0, cy, cx], want)


def test_face_on_box_covers_its_projected_rectangle(refs):
    W, H, D = 201, 151, 1.5
    a, b, c = 0.2, 0.1, 0.05
    t = _single(6, [a, b, c], [0, 0, -D])
    cam, tanh = _axis_camera(W, H)
    u, v = _pixel_dirs(W, H, tanh)
    want = (np.abs(u) <= a / (D - c)) & (np.abs(v) <= b / (D - c))
    amb = refs[1].render(t, 1, *BODY0, None, None, False, cam, tanh, W, H)[3][0].astype(bool)
    for ref in refs:
        seg = ref.render(t, 1, *BODY0, None, None, False, cam, tanh, W, H)[1][0]
        np.testing.assert_array_equal((seg == 0)[~amb], want[~amb])
    assert want.sum() > 1000 and amb.mean() <= AMB_CAP


# ---- video ------------------------------------------------------------------------------------------------------------------------
def test_avi_writer_round_trip(tmp_path):
    from stac_mjx_amd.video import _jpeg, read_avi, write_avi

    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, size=(61, 97, 3), dtype=np.uint8) for _ in range(7)]
    write_avi(tmp_path / "v.avi", frames, fps=50)
    avi = read_avi(tmp_path / "v.avi")
    assert (avi["width"], avi["height"], avi["n_frames"], avi["fps"], avi["us_per_frame"]) == (97, 61, 7, 50.0, 20000)
    assert len(avi["frames"]) == len(avi["index"]) == 7
    for f, (off, size), jb in zip(frames, avi["index"], avi["frames"]):
        assert jb == _jpeg(f) and size == len(jb)


def test_other_suffixes_fall_back_to_avi_without_imageio(tmp_path, monkeypatch):
    from stac_mjx_amd import video

    monkeypatch.setitem(sys.modules, "imageio", None)
    logs = []
    out = video.write_video(tmp_path / "v.mp4", [np.zeros((8, 8, 3), np.uint8)] * 2, fps=30, log=logs.append)
    assert out == tmp_path / "v.avi" and out.exists() and logs
    assert video.read_avi(out)["n_frames"] == 2


# ---- Python surface ---------------------------------------------------------------------------------------------------------------
def test_viz_stac_wiring(monkeypatch, tmp_path):
    import stac_mjx_amd
    from stac_mjx_amd import viz

    calls = {}
    cfg = types.SimpleNamespace(model=types.SimpleNamespace(MJCF_PATH="models/m.xml"))
    d = types.SimpleNamespace(qpos=np.zeros((5, 7)), kp_data=np.ones((5, 3)), kp_names=["a"], offsets=np.full((1, 3), 2.0))

    class FakeStac:
        def __init__(self, xml_path, cfg_, kp_names):
            calls["init"] = (xml_path, cfg_, kp_names)

        def render(self, *a):
            calls["render"] = a
            return ["frame"]

    monkeypatch.setattr(viz.io, "load_stac_data", lambda p: (calls.setdefault("path", p), (cfg, d))[1])
    monkeypatch.setattr("stac_mjx_amd.stac.Stac", FakeStac)
    out = stac_mjx_amd.viz_stac(tmp_path / "r.h5", 3, tmp_path / "o.avi", 1, "side", 10, 20, base_path=tmp_path,
                                show_marker_error=True)
    assert out == (cfg, ["frame"]) and calls["path"] == tmp_path / "r.h5"
    assert calls["init"] == (tmp_path / "models/m.xml", cfg, ["a"])
    a = calls["render"]
    assert a[0] is d.qpos and a[1] is d.kp_data and a[2] is d.offsets and a[3:] == (3, tmp_path / "o.avi", 1, "side", 10, 20, True)


def test_stac_render_argument_errors_before_any_device_work(tmp_path):
    from stac_mjx_amd.stac import Stac

    s = object.__new__(Stac)  # no engine: every check below must fire before one would be used
    s._xml_path, s._renderer = None, None
    q, kp = np.zeros((10, 7)), np.zeros((10, 3))
    with pytest.raises(ValueError, match="is not equal to the length of kp_data"):
        s.render(q, kp[:9], None, 2, tmp_path / "v.avi")
    with pytest.raises(ValueError, match="must be non-negative"):
        s.render(q, kp, None, 2, tmp_path / "v.avi", start_frame=-1)
    with pytest.raises(ValueError, match="start_frame \\+ n_frames"):
        s.render(q, kp, None, 8, tmp_path / "v.avi", start_frame=3)
    with pytest.raises(ValueError, match="MJCF"):
        s.render(q, kp, None, 2, tmp_path / "v.avi")
    assert not (tmp_path / "v.avi").exists()


def test_unknown_camera_lists_the_models_cameras(rodent):
    from stac_mjx_amd.render import Renderer

    r = object.__new__(Renderer)
    r.scene = rodent
    assert r.camera_index("side") == 2 and r.camera_index(-1) == -1 and r.camera_index(5) == 5
    with pytest.raises(ValueError, match="close_profile"):
        r.camera_index("nope")
    with pytest.raises(ValueError, match="egocentric"):
        r.camera_index(6)
