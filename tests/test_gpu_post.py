"""Post-processing on the GPU (stac.postprocess: gpu): the stitch and qvel kernels against the host functions of
``stac_mjx_amd.utils``, and ``run_stac`` end to end with both settings.  Cases and tolerances: tests/post_cases.py."""

import ctypes as C

import numpy as np
import pytest
import torch

import host_scaffold as hs
import post_cases as pc

pytestmark = pytest.mark.gpu

PATTERN = -12345.0


def _lib():
    return hs.loaded_library()


def _raw_stitch(lib, src, Cn, F, D, dst, rows, stream=None):
    from stac_mjx_amd.post import crossfade_mask

    m = np.ascontiguousarray(crossfade_mask(pc.OV))
    rc = lib.stac_post_stitch(C.c_void_p(src.data_ptr()), Cn, F, pc.OV, D, m.ctypes.data_as(C.POINTER(C.c_double)),
                              C.c_void_p(dst.data_ptr()), rows, C.c_void_p(stream) if stream else None)
    assert rc == 0, lib.stac_last_error().decode()


def _gpu_stitch_prefilled(lib, x):
    """The entry point on a destination pre-filled with a pattern: a row it does not write shows."""
    Cn, F = x.shape[0], x.shape[1] - pc.OV
    R = pc.stitch_rows(Cn, F)
    src = torch.as_tensor(x).cuda()
    dst = torch.full((R,) + x.shape[2:], PATTERN, dtype=torch.float32, device="cuda")
    _raw_stitch(lib, src, Cn, F, int(np.prod(x.shape[2:])), dst, R)
    return src, dst.cpu().numpy()


@pytest.mark.parametrize("trailing", pc.STITCH_TRAILING, ids=str)
def test_stitch_equals_handle_edge_effects(trailing):
    from stac_mjx_amd import post

    lib = _lib()
    for Cn, F in pc.STITCH_CF:
        x = pc.stitch_input(Cn, F, trailing)
        want = pc.host_stitch(x, F)
        src, got = _gpu_stitch_prefilled(lib, x)
        np.testing.assert_array_equal(got, want, err_msg=f"C={Cn} F={F}")
        out = post.stitch(src, F)  # the Python wrapper: same kernel, its own output tensor
        assert out.shape == want.shape and out.is_cuda
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"post.stitch C={Cn} F={F}")


def test_stitch_many_rows():
    """300 clips of 50: 15 000 rows, more than one sweep of the grid (2 048 workgroups of 4 rows)."""
    from stac_mjx_amd import post

    Cn, F, trailing = pc.STITCH_BIG
    x = pc.stitch_input(Cn, F, trailing)
    want = pc.host_stitch(x, F)
    assert want.shape[0] == Cn * F > 2048 * 4
    src, got = _gpu_stitch_prefilled(_lib(), x)
    np.testing.assert_array_equal(got, want)
    # a non-contiguous float64 view is made contiguous float32 first
    wide = torch.as_tensor(np.concatenate([x, x], axis=2)).cuda().double()[:, :, : x.shape[2]]
    np.testing.assert_array_equal(post.stitch(wide, F).cpu().numpy(), want)


def test_stitch_through_ctypes_guard_alignment_and_stream():
    lib = _lib()
    Cn, F, D = 5, 11, 23
    x = pc.stitch_input(Cn, F, (D,))
    want = pc.host_stitch(x, F)
    R, n = pc.stitch_rows(Cn, F), x.size
    sbuf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    src = sbuf[1 : 1 + n]
    assert src.data_ptr() % 4 == 0 and src.data_ptr() % 16 != 0
    dbuf = torch.full((R * D + 64,), PATTERN, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        src.copy_(torch.as_tensor(x.reshape(-1)).cuda())
        _raw_stitch(lib, src, Cn, F, D, dbuf, R, stream=stream.cuda_stream)
    stream.synchronize()
    got = dbuf.cpu().numpy()
    np.testing.assert_array_equal(got[: R * D].reshape(R, D), want)
    np.testing.assert_array_equal(got[R * D :], np.full(64, PATTERN, np.float32))  # the guard floats behind dst


@pytest.mark.parametrize("freejoint,nq", pc.QVEL_NQ)
@pytest.mark.parametrize("dt", pc.QVEL_DT, ids=lambda d: f"dt{d:.4g}")
def test_qvel_equals_compute_velocity_from_kinematics(freejoint, nq, dt):
    from stac_mjx_amd import post

    differ = total = 0
    for F, Cn in pc.QVEL_FC:
        q = pc.qvel_input(F, Cn, nq, freejoint, dt)
        if freejoint:
            pc.assert_host_gyro_is_meaningful(q, F)
        want = pc.host_qvel(q, F, dt, freejoint)
        got = post.infer_qvel(torch.as_tensor(q).cuda(), F, dt, freejoint, max_qvel=pc.MAX_QVEL)
        assert got.is_cuda and tuple(got.shape) == want.shape
        a, b = pc.check_qvel(got.cpu().numpy(), want, freejoint, label=f"F={F} C={Cn} nq={nq} dt={dt:.4g}")
        differ, total = differ + a, total + b
        if freejoint and F >= 7 and dt < 1.0:
            assert np.nanmax(np.abs(want[:, 3:6])) > pc.MAX_QVEL  # a gyro above max_qvel, not clipped
    print(f"GPU qvel nq={nq} dt={dt:.4g}: {differ} of {total} gyro values are not bit-equal to the host's")
    with pytest.raises(ValueError):
        post.infer_qvel(torch.zeros(7, nq, device="cuda"), 2, dt, freejoint)  # 7 rows are not clips of 2


# ---- run_stac end to end: postprocess host vs gpu ------------------------------------------------------------------------
def _cfg(rodent_cfg, **stac_over):
    from stac_mjx_amd.config import validate_config

    stac = dict(fit_offsets_path="fit.h5", ik_only_path="ik.h5", data_path="d.mat", continuous=False, n_fit_frames=4,
                skip_fit_offsets=False, skip_ik_only=False, infer_qvels=False, n_frames_per_clip=12,
                mujoco=dict(solver="newton", iterations=1, ls_iterations=4))
    stac.update(stac_over)
    cfg = validate_config({"model": dict(rodent_cfg), "stac": stac})
    cfg.model.N_ITER_Q = 30
    cfg.model.N_ITERS = 1
    return cfg


@pytest.fixture(scope="module")
def one_fit(tmp_path_factory, rodent_setup, rodent_cfg, rodent_mocap):
    from stac_mjx_amd.io import load_stac_data
    from stac_mjx_amd.main import run_stac

    d = tmp_path_factory.mktemp("post_fit")
    fit_path, _ = run_stac(_cfg(rodent_cfg, skip_ik_only=True), rodent_mocap[200:236], rodent_setup.kp_names, base_path=d, setup=rodent_setup)
    return load_stac_data(fit_path)[1]


def _run_both(tmp_path, one_fit, rodent_setup, rodent_cfg, kp, **decides):
    """run_stac with skip_fit_offsets into two directories; the fit file (whose config decides the post-processing) is the one
    fit, stored with this case's config."""
    from stac_mjx_amd import io
    from stac_mjx_amd.main import run_stac

    out = {}
    for mode in ("host", "gpu"):
        d = tmp_path / mode
        d.mkdir()
        io.save_data_to_h5(config=_cfg(rodent_cfg, **decides), file_path=d / "fit.h5", **one_fit.as_dict())
        cfg = _cfg(rodent_cfg, skip_fit_offsets=True, postprocess=mode, **decides)
        out[mode] = lambda d=d, cfg=cfg: io.load_stac_data(run_stac(cfg, kp, rodent_setup.kp_names, base_path=d, setup=rodent_setup)[1])[1]
    return out


@pytest.mark.parametrize("continuous,infer_qvels", [(True, True), (True, False), (False, True)])
def test_run_stac_postprocess_gpu_equals_host(tmp_path, one_fit, rodent_setup, rodent_cfg, rodent_mocap, continuous, infer_qvels):
    from stac_mjx_amd.io import _DATASETS

    kp = rodent_mocap[200:236]
    runs = _run_both(tmp_path, one_fit, rodent_setup, rodent_cfg, kp, continuous=continuous, infer_qvels=infer_qvels)
    host, gpu = runs["host"](), runs["gpu"]()
    assert host.qpos.shape == (36, 74) and host.xquat.shape == (36, 67, 4) and host.kp_data.shape == (36, 69)
    for name in _DATASETS:
        h, g = np.asarray(getattr(host, name)), np.asarray(getattr(gpu, name))
        assert h.shape == g.shape and h.dtype == g.dtype, (name, h.shape, g.shape, h.dtype, g.dtype)
        if name == "qvel" and infer_qvels:
            assert h.shape == (36, 73)
            pc.assert_host_gyro_is_meaningful(host.qpos, 12)
            pc.check_qvel(g, h, True, label=f"run_stac continuous={continuous}")
        else:
            np.testing.assert_array_equal(g, h, err_msg=name)
    if not infer_qvels:
        assert np.asarray(host.qvel).size == 0 and np.asarray(gpu.qvel).size == 0
    if continuous:  # the fade of equal values: the stitched keypoints are the input again
        np.testing.assert_allclose(gpu.kp_data, kp, rtol=1e-6, atol=1e-7)


def test_run_stac_rows_that_are_not_whole_clips_raise_on_both_paths(tmp_path, one_fit, rodent_setup, rodent_cfg, rodent_mocap):
    """continuous + infer_qvels with n_frames_per_clip = 4 < 10: 9 windows stitch to 42 rows, which 4 does not divide."""
    runs = _run_both(tmp_path, one_fit, rodent_setup, rodent_cfg, rodent_mocap[200:236], continuous=True, infer_qvels=True,
                     n_frames_per_clip=4)
    for mode in ("host", "gpu"):
        with pytest.raises(ValueError):
            runs[mode]()


def test_ik_only_post_argument(rodent_setup, rodent_cfg, rodent_mocap):
    """Checked before any work; the phase clock gains exactly one key; without ``post`` nothing changes."""
    from stac_mjx_amd.stac import Stac

    kp, off = rodent_mocap[300:304], rodent_setup.tables.site_pos + 0.002
    post = {"continuous": True, "n_frames_per_clip": 2, "infer_qvels": True}
    bad = Stac(None, _cfg(rodent_cfg, n_frames_per_clip=2, continuous=True, reference_marker_order=True), rodent_setup.kp_names,
               setup=rodent_setup, verbose=False)
    with pytest.raises(ValueError, match="reference_marker_order"):
        bad.ik_only(kp, off, post=post)
    stac = Stac(None, _cfg(rodent_cfg, n_frames_per_clip=2), rodent_setup.kp_names, setup=rodent_setup, verbose=False)
    stac.timings = {}
    plain = stac.ik_only(kp, off)
    keys = set(stac.timings)
    assert keys == {"batch_and_h2d_s", "q_phase_and_fk_kernels_s", "d2h_and_packing_s"} and np.asarray(plain.qvel).size == 0
    stac.timings = {}
    data = stac.ik_only(kp, off, post={"continuous": False, "n_frames_per_clip": 2, "infer_qvels": True})
    assert set(stac.timings) == keys | {"postprocess_s"}
    stac.timings = None
    np.testing.assert_array_equal(data.qpos, plain.qpos)
    np.testing.assert_array_equal(data.marker_sites, plain.marker_sites)
    np.testing.assert_array_equal(data.kp_data, plain.kp_data)
    pc.check_qvel(data.qvel, pc.host_qvel(plain.qpos, 2, stac._timestep, True), True, label="ik_only post")
