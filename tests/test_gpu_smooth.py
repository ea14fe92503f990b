"""Smoothing fitted poses on the GPU (stac.smooth): the kernel against the numpy restatement of the rule with tolerance 0, the
refusals of the entry point, and ``run_stac`` / ``Stac.smooth_result`` end to end.  Cases and restatement: tests/smooth_cases.py."""

import ctypes as C
import json

import numpy as np
import pytest
import torch

import host_scaffold as hs
import post_cases as pc
import smooth_cases as sc

pytestmark = pytest.mark.gpu

PATTERN = -12345.0
STAC_ERR_INVALID = -1


def _lib():
    return hs.loaded_library()


def _raw_smooth(lib, src, L, taps, cols, lb, ub, dst, stream=None):
    """The entry point itself, on a destination the caller filled."""
    N, nq = src.shape
    qc = np.ascontiguousarray(cols, dtype=np.int32)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    return lib.stac_post_smooth(p(src), N, nq, L, taps.shape[0] // 2, taps.ctypes.data_as(C.POINTER(C.c_float)),
                                qc.ctypes.data_as(C.POINTER(C.c_int32)), len(cols), p(lb), p(ub), p(dst),
                                C.c_void_p(stream) if stream else None)


@pytest.mark.parametrize("name", list(sc.LAYOUTS))
@pytest.mark.parametrize("H", sc.HALF_WINDOWS)
def test_kernel_equals_restatement(name, H):
    """Per layout and half-width every clip length at which the kernel takes another path (``smooth_cases.clip_lengths`` of the
    tile the host picks); the eight combinations of clips in {1, 3}, bounds / null bounds and the two kinds of table are dealt
    over the lengths.  Inputs: rotation chains with negated and rescaled frames, a zero quaternion, a zero block column, NaNs."""
    from stac_mjx_amd import post

    lib = _lib()
    nq, cols = sc.LAYOUTS[name]
    T = post.smooth_tile_frames(nq, H)
    assert T >= 1
    for i, L in enumerate(sc.clip_lengths(T, H)):
        k = i + sc.HALF_WINDOWS.index(H)
        clips, bounded, kind = (1, 3)[k & 1], bool(k & 2), ("savgol", "gaussian")[(k >> 2) & 1]
        label = f"{name} H={H} T={T} L={L} clips={clips} bounds={bounded} {kind}"
        taps = post.smooth_taps(kind, H)
        x = sc.make_input(L, clips, nq, cols, H)
        lb, ub = sc.make_bounds(nq, cols) if bounded else (None, None)
        want = sc.restate(x, L, taps, cols, lb, ub)
        src = torch.as_tensor(x).cuda()
        dlb, dub = (torch.as_tensor(lb).cuda(), torch.as_tensor(ub).cuda()) if bounded else (None, None)
        dst = torch.full((x.shape[0] * nq + 64,), PATTERN, dtype=torch.float32, device="cuda")  # (64 guard floats behind the output)
        rc = _raw_smooth(lib, src, L, taps, cols, dlb, dub, dst)
        assert rc == 0, lib.stac_last_error().decode()
        got = dst.cpu().numpy()
        sc.assert_same_bits(got[: x.size].reshape(x.shape), want, label=label)
        np.testing.assert_array_equal(got[x.size:], np.full(64, PATTERN, np.float32), err_msg=label)
        np.testing.assert_array_equal(src.cpu().numpy().view(np.uint32), x.view(np.uint32))  # the input is only read
        out = post.smooth(src, L, taps, cols, lb=lb, ub=ub)  # the Python wrapper: same kernel, its own output tensor
        assert out.is_cuda and out.shape == src.shape and out.data_ptr() != src.data_ptr()
        sc.assert_same_bits(out.cpu().numpy(), want, label="post.smooth " + label)


def test_kernel_many_tiles_and_unaligned_rows_on_a_stream():
    """15 000 rows of 74 (the scale of ``post_cases.STITCH_BIG``) as 1 500 clips of 10: more tiles than the 1 024 workgroups of a
    grid, so every workgroup strides; then as 3 clips of 5 000: 40 tiles per clip.  The buffers are 4-byte aligned only and the
    work is queued on a side stream."""
    from stac_mjx_amd import post

    lib = _lib()
    nq, cols = sc.LAYOUTS["rodent74"]
    lb, ub = sc.make_bounds(nq, cols)
    stream = torch.cuda.Stream()
    for L, clips, H, kind in ((10, 1500, 3, "savgol"), (5000, 3, 16, "gaussian")):
        assert clips * L == pc.STITCH_BIG[0] * pc.STITCH_BIG[1]
        T = post.smooth_tile_frames(nq, H)
        assert clips * -(-L // T) > 1024 or L > 2 * T
        taps = post.smooth_taps(kind, H)
        x = sc.make_input(L, clips, nq, cols, H, specials=False)
        x[7, 20] = np.nan
        want = sc.restate(x, L, taps, cols, lb, ub)
        sbuf = torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
        dbuf = torch.full((x.size + 65,), PATTERN, dtype=torch.float32, device="cuda")
        src, dst = sbuf[1:1 + x.size].view(x.shape), dbuf[1:]
        assert src.data_ptr() % 16 != 0 and dst.data_ptr() % 16 != 0
        with torch.cuda.stream(stream):
            src.copy_(torch.as_tensor(x).cuda())
            dlb, dub = torch.as_tensor(lb).cuda(), torch.as_tensor(ub).cuda()
            rc = _raw_smooth(lib, src, L, taps, cols, dlb, dub, dst, stream=stream.cuda_stream)
        assert rc == 0, lib.stac_last_error().decode()
        stream.synchronize()
        got = dbuf.cpu().numpy()
        sc.assert_same_bits(got[1:1 + x.size].reshape(x.shape), want, label=f"L={L} clips={clips}")
        np.testing.assert_array_equal(got[1 + x.size:], np.full(64, PATTERN, np.float32))
        assert got[0] == np.float32(PATTERN)


def test_entry_point_refusals_leave_out_untouched():
    from stac_mjx_amd import post

    lib = _lib()
    nq, cols = sc.LAYOUTS["tail_ball13"]
    x = sc.make_input(10, 4, nq, cols, 3)
    taps3, taps16 = post.smooth_taps("savgol", 3), post.smooth_taps("savgol", 16)
    src = torch.as_tensor(x).cuda()
    lb, ub = (torch.as_tensor(b).cuda() for b in sc.make_bounds(nq, cols))
    dst = torch.full_like(src, PATTERN)

    def refused(**kw):
        a = dict(src=src, L=10, taps=taps3, cols=cols, lb=lb, ub=ub, dst=dst)
        a.update(kw)
        rc = _raw_smooth(lib, a["src"], a["L"], a["taps"], a["cols"], a["lb"], a["ub"], a["dst"])
        msg = lib.stac_last_error().decode()
        assert rc == STAC_ERR_INVALID and lib.stac_last_error_code() == STAC_ERR_INVALID and msg, (kw.keys(), rc, msg)
        return msg

    refused(taps=np.zeros((1, 1), np.float32))                       # H = 0
    refused(taps=np.zeros((35, 35), np.float32), L=40)               # H = 17
    refused(taps=taps16)                                             # clip_len 10 < W = 33
    refused(L=6)                                                     # clip_len < W = 7
    refused(L=16)                                                    # 40 rows are not whole clips of 16
    assert "overlap" in refused(cols=[3, 6])
    assert "leaves" in refused(cols=[3, 10])
    wide = torch.zeros(40, 400, device="cuda")
    assert "64" in refused(src=wide, cols=list(range(0, 260, 4)), lb=None, ub=None, dst=torch.full_like(wide, PATTERN))
    assert "overlap" in refused(dst=src)                             # in place
    refused(lb=None)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dst.cpu().numpy(), np.full(x.shape, PATTERN, np.float32))
    np.testing.assert_array_equal(src.cpu().numpy().view(np.uint32), x.view(np.uint32))
    for bad in (dict(clip_len=6), dict(clip_len=16), dict(quat_cols=[3, 6]), dict(quat_cols=[10]), dict(lb=lb.cpu().numpy())):
        a = dict(clip_len=10, taps=taps3, quat_cols=cols)
        a.update(bad)
        with pytest.raises(ValueError):
            post.smooth(src, **a)
    with pytest.raises(ValueError):
        post.smooth(src, 10, taps3[:, :5], cols)
    assert post.smooth(src[:0], 10, taps3, cols).shape == (0, nq)


# ---- run_stac end to end ----------------------------------------------------------------------------------------------------------
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

    d = tmp_path_factory.mktemp("smooth_fit")
    fit_path, _ = run_stac(_cfg(rodent_cfg, skip_ik_only=True), rodent_mocap[200:236], rodent_setup.kp_names, base_path=d, setup=rodent_setup)
    return load_stac_data(fit_path)[1]


@pytest.mark.parametrize("continuous", [False, True])
def test_run_stac_smooth_end_to_end(tmp_path, one_fit, rodent_setup, rodent_cfg, rodent_mocap, continuous):
    """The config of the existing run_stac post tests (tests/test_gpu_post.py): one fit, 36 frames as 3 clips of 12."""
    from stac_mjx_amd import io, post
    from stac_mjx_amd.main import report_path, run_stac
    from stac_mjx_amd.stac import Stac

    kp = rodent_mocap[200:236]
    decides = dict(continuous=continuous, infer_qvels=True)
    runs = {}
    for mode in ("off", "savgol"):
        d = tmp_path / mode
        d.mkdir()
        io.save_data_to_h5(config=_cfg(rodent_cfg, **decides), file_path=d / "fit.h5", **one_fit.as_dict())
        cfg = _cfg(rodent_cfg, skip_fit_offsets=True, postprocess="gpu", smooth=mode, report="on", **decides)
        path = run_stac(cfg, kp, rodent_setup.kp_names, base_path=d, setup=rodent_setup)[1]
        runs[mode] = (path, io.load_stac_data(path)[1], cfg)
    off, (path, data, cfg) = runs["off"][1], runs["savgol"]
    assert np.asarray(off.qpos_raw).size == 0
    L = 36 if continuous else 12
    taps = post.smooth_taps("savgol", 3, order=2)
    # qpos_raw is the qpos of the same run without smoothing; qpos is its restatement
    sc.assert_same_bits(data.qpos_raw, off.qpos, label="qpos_raw")
    np.testing.assert_array_equal(data.kp_data, off.kp_data)
    want = sc.restate(data.qpos_raw, L, taps, [3], rodent_setup.lb.astype(np.float32), rodent_setup.ub.astype(np.float32))
    sc.assert_same_bits(data.qpos, want, label="qpos")
    assert np.any(data.qpos != data.qpos_raw)
    # the kinematics in the file are those of the file's qpos, under the file's offsets
    stac = Stac(None, cfg, rodent_setup.kp_names, setup=rodent_setup, verbose=False)
    stac.engine.set_site_pos(torch.as_tensor(np.array(data.offsets, dtype=np.float32)))
    fk = stac.engine.fk(torch.as_tensor(np.array(data.qpos)).cuda(), want=("xpos", "xquat", "site_xpos"))
    for name, key in (("xpos", "xpos"), ("xquat", "xquat"), ("marker_sites", "site_xpos")):
        sc.assert_same_bits(np.asarray(getattr(data, name)), fk[key].cpu().numpy(), label=name)
    # qvel is inferred from the smoothed qpos
    pc.assert_host_gyro_is_meaningful(data.qpos, 12)
    pc.check_qvel(data.qvel, pc.host_qvel(data.qpos, 12, stac._timestep, True), True, label=f"smooth continuous={continuous}")
    # the report states the smoothed pose's marker error, for the file's frames
    rep = json.loads(report_path(path).read_text())
    assert rep["n_frames"] == data.qpos.shape[0] == 36
    # smooth_result: the same options reproduce the file from its qpos_raw, other options do not
    again = stac.smooth_result(path, "savgol", half_window=3, order=2)
    for name in ("qpos", "qpos_raw", "xpos", "xquat", "marker_sites", "kp_data", "offsets"):
        sc.assert_same_bits(np.asarray(getattr(again, name), dtype=np.float32), np.asarray(getattr(data, name), dtype=np.float32), label="smooth_result " + name)
    np.testing.assert_array_equal(again.qvel.view(np.uint32), data.qvel.view(np.uint32))
    other = stac.smooth_result(path, "savgol", half_window=1, order=0)
    sc.assert_same_bits(other.qpos_raw, data.qpos_raw, label="smooth_result starts from qpos_raw")
    assert np.any(other.qpos != data.qpos) and np.any(other.marker_sites != data.marker_sites) and np.any(other.qvel != data.qvel)
    sc.assert_same_bits(other.qpos, sc.restate(data.qpos_raw, L, post.smooth_taps("savgol", 1, order=0), [3],
                                               rodent_setup.lb.astype(np.float32), rodent_setup.ub.astype(np.float32)), label="other")
    # a result without qpos_raw (the smooth: off file) is smoothed from its qpos: the same arrays again
    from_off = stac.smooth_result(runs["off"][0], "savgol", half_window=3, order=2)
    sc.assert_same_bits(from_off.qpos, data.qpos, label="smooth_result of the unsmoothed file")
    sc.assert_same_bits(from_off.marker_sites, data.marker_sites, label="smooth_result of the unsmoothed file, markers")
    if not continuous:  # the stored config decides the clips: 12 frames are shorter than a window of 33 (the 36 stitched ones are not)
        with pytest.raises(ValueError, match="33"):
            stac.smooth_result(path, "gaussian", half_window=16)
    else:
        assert stac.smooth_result(path, "gaussian", half_window=16).qpos.shape == data.qpos.shape


def test_ik_only_post_smooth_argument(rodent_setup, rodent_cfg, rodent_mocap):
    """Checked before any work; the phase clock gains no key; ``kp_data`` is untouched."""
    from stac_mjx_amd.stac import Stac

    kp, off = rodent_mocap[300:316], rodent_setup.tables.site_pos + 0.002
    post = {"continuous": False, "n_frames_per_clip": 8, "infer_qvels": True, "smooth": {"kind": "gaussian", "half_window": 2, "order": None, "sigma": None}}
    bad = Stac(None, _cfg(rodent_cfg, n_frames_per_clip=8, reference_marker_order=True), rodent_setup.kp_names, setup=rodent_setup, verbose=False)
    with pytest.raises(ValueError, match="reference_marker_order"):
        bad.ik_only(kp, off, post=post)
    stac = Stac(None, _cfg(rodent_cfg, n_frames_per_clip=8), rodent_setup.kp_names, setup=rodent_setup, verbose=False)
    for broken in ({"kind": "boxcar", "half_window": 2}, {"kind": "savgol", "half_window": 17}, {"kind": "gaussian", "half_window": 4}):
        with pytest.raises(ValueError):  # (the last: clips of 8 frames are shorter than the window of 9)
            stac.ik_only(kp, off, post=dict(post, smooth=broken))
    stac.timings = {}
    plain = stac.ik_only(kp, off, post=dict(post, smooth=None))
    keys = set(stac.timings)
    stac.timings = {}
    data = stac.ik_only(kp, off, post=post)
    assert set(stac.timings) == keys
    stac.timings = None
    assert np.asarray(plain.qpos_raw).size == 0
    sc.assert_same_bits(data.qpos_raw, plain.qpos, label="qpos_raw")
    np.testing.assert_array_equal(data.kp_data, plain.kp_data)
    from stac_mjx_amd import post as gpost

    want = sc.restate(plain.qpos, 8, gpost.smooth_taps("gaussian", 2), [3], rodent_setup.lb.astype(np.float32), rodent_setup.ub.astype(np.float32))
    sc.assert_same_bits(data.qpos, want, label="qpos")
