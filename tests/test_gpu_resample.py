"""Resampling fitted poses on the GPU (stac.resample): the kernel against the numpy restatement of the rule with tolerance 0, what
the rule promises on the kernel's output, the refusals of the entry point, and ``Stac.resample_result`` / ``run_stac`` end to end.
Cases and restatement: tests/resample_cases.py."""

import ctypes as C

import numpy as np
import pytest
import torch

import host_scaffold as hs
import resample_cases as rc

pytestmark = pytest.mark.gpu

PATTERN = -12345.0
STAC_ERR_INVALID = -1
ULP1 = float(np.spacing(np.float32(1.0)))


def _lib():
    return hs.loaded_library()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _raw(lib, src, L, U, D, taps_dev, cols, lb, ub, dst, out_rows, half=None, stream=None):
    """The entry point itself, on a destination the caller filled."""
    N, ncol = src.shape
    qc = np.ascontiguousarray(cols, dtype=np.int32)
    half = (taps_dev.shape[1] // 2 - 1) * U if half is None else half
    return lib.stac_post_resample(_p(src), N, ncol, L, U, D, half, _p(taps_dev), qc.ctypes.data_as(C.POINTER(C.c_int32)), len(cols), _p(lb),
                                  _p(ub), _p(dst), out_rows, C.c_void_p(stream) if stream else None)


def _cases():
    from stac_mjx_amd import post

    return rc.cases(post.resample_tile_rows, post.RESAMPLE_MAX_BAND)


def test_kernel_equals_restatement():
    """The case list: ratios and lobes, the clip lengths at which every tap is clamped or the outputs fill a tile, one more and two
    tiles and one, the column layouts around the band, the widest window, and a tile shorter than U.  Each case through the raw
    entry point (guard floats behind the output, the input only read) and through ``post.resample``."""
    from stac_mjx_amd import post

    lib = _lib()
    cases = _cases()
    assert len(cases) > 40
    for label, U, D, taps, L, clips, ncol, cols, bounded in cases:
        x = rc.make_input(L, clips, ncol, cols)
        lb, ub = rc.make_bounds(ncol, cols) if bounded else (None, None)
        want = rc.restate(x, L, U, D, taps, cols, lb, ub)
        src, taps_dev = torch.as_tensor(x).cuda(), torch.as_tensor(taps).cuda()
        dlb, dub = (torch.as_tensor(lb).cuda(), torch.as_tensor(ub).cuda()) if bounded else (None, None)
        dst = torch.full((want.size + 64,), PATTERN, dtype=torch.float32, device="cuda")  # (64 guard floats behind the output)
        rcode = _raw(lib, src, L, U, D, taps_dev, cols, dlb, dub, dst, want.shape[0])
        assert rcode == 0, (label, lib.stac_last_error().decode())
        got = dst.cpu().numpy()
        rc.assert_same_bits(got[: want.size].reshape(want.shape), want, label=label)
        np.testing.assert_array_equal(got[want.size:], np.full(64, PATTERN, np.float32), err_msg=label)
        np.testing.assert_array_equal(src.cpu().numpy().view(np.uint32), x.view(np.uint32))  # the input is only read
        out = post.resample(src, L, U, D, taps, cols, lb=lb, ub=ub)  # the Python wrapper: same kernel, its own output tensor
        assert out.is_cuda and out.shape == want.shape
        rc.assert_same_bits(out.cpu().numpy(), want, label="post.resample " + label)


def test_many_tiles_unaligned_rows_side_stream_and_determinism():
    """More tiles than the workgroups of a grid (1 500 clips of 12 rows up by 5 / 3: every workgroup strides) and long clips (3 of
    5 000 rows down by 6); buffers 4-byte aligned only, queued on a side stream; a second call gives the same bits."""
    from stac_mjx_amd import post

    lib = _lib()
    ncol, cols = 74, [3]
    lb, ub = rc.make_bounds(ncol, cols)
    stream = torch.cuda.Stream()
    for L, clips, U, D, lobes in ((12, 1500, 5, 3, 2), (5000, 3, 1, 6, 10)):
        taps = rc.taps32(U, D, lobes)
        Lo = rc.rows(L, U, D)
        T = post.resample_tile_rows(ncol, U, D, taps.shape[1])
        assert clips * -(-Lo // T) > 1024 or Lo > 2 * T
        x = rc.make_input(L, clips, ncol, cols, specials=False)
        x[7, 20] = np.nan
        want = rc.restate(x, L, U, D, taps, cols, lb, ub)
        sbuf = torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
        dbuf = torch.full((want.size + 65,), PATTERN, dtype=torch.float32, device="cuda")
        src, dst = sbuf[1:1 + x.size].view(x.shape), dbuf[1:]
        assert src.data_ptr() % 16 != 0 and dst.data_ptr() % 16 != 0
        with torch.cuda.stream(stream):
            src.copy_(torch.as_tensor(x).cuda())
            dlb, dub, taps_dev = torch.as_tensor(lb).cuda(), torch.as_tensor(ub).cuda(), torch.as_tensor(taps).cuda()
            rcode = _raw(lib, src, L, U, D, taps_dev, cols, dlb, dub, dst, want.shape[0], stream=stream.cuda_stream)
        assert rcode == 0, lib.stac_last_error().decode()
        stream.synchronize()
        got = dbuf.cpu().numpy()
        rc.assert_same_bits(got[1:1 + want.size].reshape(want.shape), want, label=f"L={L} clips={clips}")
        np.testing.assert_array_equal(got[1 + want.size:], np.full(64, PATTERN, np.float32))
        assert got[0] == np.float32(PATTERN)
        again = torch.full_like(dbuf, PATTERN)
        with torch.cuda.stream(stream):
            assert _raw(lib, src, L, U, D, taps_dev, cols, dlb, dub, again[1:], want.shape[0], stream=stream.cuda_stream) == 0
        stream.synchronize()
        np.testing.assert_array_equal(again.cpu().numpy().view(np.uint32), got.view(np.uint32))


def test_three_clips_of_constants_do_not_see_each_other():
    from stac_mjx_amd import post

    for U, D, lobes in ((5, 12, 10), (5, 3, 10)):
        taps = post.resample_taps(U, D, lobes)
        W = taps.shape[1]
        L = 9  # shorter than the window: every window of the middle clip reaches past both of its ends
        assert L < W // 2
        Lo = post.resample_rows(L, U, D)
        consts = (1.0, 100.0, -50.0)
        x = np.repeat(np.array(consts, np.float32), L)[:, None] * np.ones((1, 5), np.float32)
        out = post.resample(torch.as_tensor(x).cuda(), L, U, D, taps).cpu().numpy()
        rc.assert_same_bits(out, rc.restate(x, L, U, D, taps), label=f"{U}/{D}")
        for c, clip in zip(consts, out.reshape(3, Lo, 5)):
            assert np.abs(clip.astype(np.float64) - c).max() <= (W + 1) * 2.0**-23 * abs(c), (U, D, c)


def test_quaternions_signs_fallback_and_nan():
    from stac_mjx_amd import post

    U, D = 5, 12
    taps = post.resample_taps(U, D, 2)
    W = taps.shape[1]
    H = W // 2
    L = 40
    n, _ = rc.index(L, U, D)
    run = lambda a, cols: post.resample(torch.as_tensor(np.ascontiguousarray(a)).cuda(), L, U, D, taps, cols).cpu().numpy()  # noqa: E731
    # q, -q, q, ... comes out as the plain series does, times the sign of the centre row: bit for bit, a sign is exact
    q, flip, sign = rc.alternating_quats(L, n)
    plain, alt = run(q, [0]), run(flip, [0])
    rc.assert_same_bits(plain, rc.restate(q, L, U, D, taps, [0]), label="plain")
    rc.assert_same_bits(alt, plain * sign, label="alternating signs")
    assert np.abs(np.linalg.norm(alt.astype(np.float64), axis=1) - 1.0).max() <= 2.0 * ULP1
    # a zero block in the centre row decides no hemisphere (every dot product is 0 and counts as +) and the rows are summed as they
    # are; the fallback answers a sum without a direction: in a window of zeros the output is the centre block
    z = q.copy()
    z[int(n[5])] = 0.0
    out = run(z, [0])
    rc.assert_same_bits(out, rc.restate(z, L, U, D, taps, [0]), label="zero centre")
    assert abs(float(np.linalg.norm(out[5].astype(np.float64))) - 1.0) <= 2.0 * ULP1
    z[:] = 0.0
    z[L - 1] = q[L - 1]
    out = run(z, [0])
    rc.assert_same_bits(out, rc.restate(z, L, U, D, taps, [0]), label="zero window")
    np.testing.assert_array_equal(out[0], np.zeros(4, np.float32))
    # a NaN in one row of one scalar column reaches exactly the outputs whose window holds that row, and no other column
    x = rc.make_input(L, 1, 7, [3], specials=False)
    x[17, 1] = np.nan
    out = run(x, [3])
    hit = np.flatnonzero((n - H + 1 <= 17) & (17 <= n + H))
    assert 0 < hit.size < out.shape[0]
    np.testing.assert_array_equal(np.flatnonzero(np.isnan(out[:, 1])), hit)
    assert not np.isnan(np.delete(out, 1, axis=1)).any()


def test_bounds_cut_the_overshoot_of_a_step():
    from stac_mjx_amd import post

    U, D, L = 5, 12, 60
    taps = post.resample_taps(U, D)
    step = np.where(np.arange(L) < 30, -1.0, 1.0).astype(np.float32)[:, None] * np.ones((1, 3), np.float32)
    src = torch.as_tensor(step).cuda()
    one = np.ones(3, np.float32)
    cut = post.resample(src, L, U, D, taps, lb=-one, ub=one).cpu().numpy()
    assert cut.max() <= 1.0 and cut.min() >= -1.0
    wide = post.resample(src, L, U, D, taps, lb=-2 * one, ub=2 * one).cpu().numpy()
    assert (wide > 1.0).any() or (wide < -1.0).any()  # the negative lobes of the sinc overshoot
    rc.assert_same_bits(cut, np.clip(wide, -1.0, 1.0), label="the clamp alone differs")
    rc.assert_same_bits(wide, rc.restate(step, L, U, D, taps, [], -2 * one, 2 * one), label="wide")


def test_entry_point_refusals_leave_out_untouched():
    from stac_mjx_amd import post

    lib = _lib()
    ncol, cols, L, U, D = 13, [3, 9], 10, 5, 12
    taps = torch.as_tensor(post.resample_taps(U, D, 1)).cuda()
    x = rc.make_input(L, 4, ncol, cols)
    src = torch.as_tensor(x).cuda()
    lb, ub = (torch.as_tensor(b).cuda() for b in rc.make_bounds(ncol, cols))
    rows = 4 * rc.rows(L, U, D)
    dst = torch.full((rows, ncol), PATTERN, dtype=torch.float32, device="cuda")

    def refused(word, **kw):
        a = dict(src=src, L=L, U=U, D=D, taps=taps, cols=cols, lb=lb, ub=ub, dst=dst, rows=rows, half=None)
        a.update(kw)
        rcode = _raw(lib, a["src"], a["L"], a["U"], a["D"], a["taps"], a["cols"], a["lb"], a["ub"], a["dst"], a["rows"], half=a["half"])
        msg = lib.stac_last_error().decode()
        assert rcode == STAC_ERR_INVALID and lib.stac_last_error_code() == STAC_ERR_INVALID and word in msg, (kw.keys(), rcode, msg)

    refused("up is outside", U=33)
    refused("down is outside", D=65)
    refused("clip_len >= 1", L=0)
    refused("256", half=U * 128)                                       # W = 258
    refused("not whole clips", L=16)
    refused("out_rows", rows=rows - 1)
    refused("out_rows", rows=rows + 1)
    refused("overlap", cols=[3, 6])
    refused("leaves the row", cols=[3, 10])
    refused("at most 64", src=torch.zeros(40, 400, device="cuda"), cols=list(range(0, 260, 4)), lb=None, ub=None,
            dst=torch.full((rows, 400), PATTERN, device="cuda"))
    refused("lb and ub", lb=None)
    refused("x and out overlap", dst=src)                              # in place
    refused("4-byte aligned", dst=dst.view(-1).view(torch.uint8)[2:])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dst.cpu().numpy(), np.full((rows, ncol), PATTERN, np.float32))
    np.testing.assert_array_equal(src.cpu().numpy().view(np.uint32), x.view(np.uint32))
    t_np = taps.cpu().numpy()
    for bad in (dict(clip_len=0), dict(clip_len=16), dict(quat_cols=[3, 6]), dict(quat_cols=[10]), dict(lb=lb), dict(U=6), dict(D=65),
                dict(taps=t_np[:, :3]), dict(taps=np.zeros((5, 258), np.float32)), dict(taps=taps.cpu()), dict(lb=lb[:5], ub=ub[:5])):
        a = dict(clip_len=L, U=U, D=D, taps=t_np, quat_cols=cols)
        a.update(bad)
        with pytest.raises(ValueError):
            post.resample(src, **a)
    empty = post.resample(src[:0], L, U, D, t_np, cols)
    assert empty.shape == (0, ncol) and empty.is_cuda


# ---- Stac.resample_result and run_stac end to end ------------------------------------------------------------------------------------
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
def runs(tmp_path_factory, rodent_setup, rodent_cfg, rodent_mocap):
    """The 36-frame setup of tests/test_gpu_smooth.py (one fit, 3 clips of 12), with marks, once without and once with
    stac.resample from 120 to 50 Hz -> {mode: (ik_only path, config)}."""
    from stac_mjx_amd import io
    from stac_mjx_amd.main import run_stac

    d = tmp_path_factory.mktemp("resample_fit")
    kp = np.array(rodent_mocap[200:236], dtype=np.float32)
    fit_path, _ = run_stac(_cfg(rodent_cfg, skip_ik_only=True), kp, rodent_setup.kp_names, base_path=d, setup=rodent_setup)
    fit = io.load_stac_data(fit_path)[1]
    kp[5:9, 6:9] = np.nan  # a gap for fill_missing: the files carry kp_gap
    out = {}
    decides = dict(infer_qvels=True)
    for mode, keys in (("off", {}), ("kaiser", dict(resample="kaiser", mocap_hz=120, resample_hz=50, resample_lobes=2))):
        sub = d / mode
        sub.mkdir()
        io.save_data_to_h5(config=_cfg(rodent_cfg, **decides), file_path=sub / "fit.h5", **fit.as_dict())
        cfg = _cfg(rodent_cfg, skip_fit_offsets=True, postprocess="gpu", fill_missing="linear", report="on", **decides, **keys)
        paths = run_stac(cfg, kp, rodent_setup.kp_names, base_path=sub, setup=rodent_setup)
        assert len(paths) == 2
        out[mode] = (paths[1], cfg)
    return out


def test_run_stac_writes_a_second_file_and_leaves_the_first(runs):
    import json

    from stac_mjx_amd import io
    from stac_mjx_amd.main import report_path, resampled_path

    (off_path, _), (path, cfg) = runs["off"], runs["kaiser"]
    second = resampled_path(path, 50)
    assert second.exists() and second.parent == path.parent and not resampled_path(off_path, 50).exists()
    assert sorted(p.name for p in off_path.parent.iterdir()) == sorted(p.name for p in path.parent.iterdir() if ".50hz." not in p.name)
    a, b = io.load_stac_data(off_path)[1], io.load_stac_data(path)[1]
    for name, va in a.as_dict().items():  # every dataset of the first file is that of a run without the keys
        vb = b.as_dict()[name]
        if isinstance(va, np.ndarray):
            assert va.dtype == vb.dtype and va.shape == vb.shape, name
            np.testing.assert_array_equal(va.view(np.uint8) if va.dtype.kind == "f" else va, vb.view(np.uint8) if vb.dtype.kind == "f" else vb, err_msg=name)
        else:
            assert list(va) == list(vb), name
    stored, data = io.load_stac_result(second)
    Lo = rc.rows(12, 5, 12)
    assert stored.stac.n_frames_per_clip == Lo == 5 and data.qpos.shape == (3 * Lo, 74)
    assert (stored.stac.resample, stored.stac.mocap_hz, stored.stac.resample_hz, stored.stac.resample_lobes, stored.stac.resample_beta) == \
        ("kaiser", 120, 50, 2, 5.0)
    assert json.loads(report_path(second).read_text())["n_frames"] == 3 * Lo and json.loads(report_path(path).read_text())["n_frames"] == 36


def test_resample_result_on_a_stored_result(runs, rodent_setup):
    from stac_mjx_amd import io, post
    from stac_mjx_amd.main import resampled_path
    from stac_mjx_amd.stac import Stac

    path, cfg = runs["kaiser"]
    src = io.load_stac_data(path)[1]
    stac = Stac(None, cfg, rodent_setup.kp_names, setup=rodent_setup, verbose=False)
    before = stac.engine.get_site_pos().cpu().numpy().copy()
    U, D, L = 5, 12, 12
    Lo = rc.rows(L, U, D)
    for lobes in (2, 10):
        data = stac.resample_result(path, 120, 50, lobes=lobes)
        np.testing.assert_array_equal(stac.engine.get_site_pos().cpu().numpy(), before)  # the engine's offsets are as they were
        taps = rc.taps32(U, D, lobes)
        assert data.qpos.shape == (3 * Lo, 74) and data.kp_data.shape == (3 * Lo, 69) and data.qvel.shape == (3 * Lo, 73)
        assert data.xpos.shape[0] == data.xquat.shape[0] == data.marker_sites.shape[0] == 3 * Lo and np.asarray(data.qpos_raw).size == 0
        lb, ub = rodent_setup.lb.astype(np.float32), rodent_setup.ub.astype(np.float32)
        rc.assert_same_bits(data.qpos, rc.restate(np.asarray(src.qpos, np.float32), L, U, D, taps, [3], lb, ub), label="qpos")
        rc.assert_same_bits(data.kp_data, rc.restate(np.asarray(src.kp_data, np.float32), L, U, D, taps), label="kp_data")
        assert np.abs(np.linalg.norm(data.qpos[:, 3:7].astype(np.float64), axis=1) - 1.0).max() <= 2.0 * ULP1
        # the kinematics are those of the returned qpos, under the file's offsets
        stac.engine.set_site_pos(torch.as_tensor(np.array(src.offsets, dtype=np.float32)))
        q = torch.as_tensor(np.array(data.qpos)).cuda()
        fk = stac.engine.fk(q, want=("xpos", "xquat", "site_xpos"))
        stac.engine.set_site_pos(torch.as_tensor(before))
        for name, key in (("xpos", "xpos"), ("xquat", "xquat"), ("marker_sites", "site_xpos")):
            rc.assert_same_bits(np.asarray(getattr(data, name)), fk[key].cpu().numpy(), label=name)
        # qvel: the real step
        qvel = post.infer_qvel(q, Lo, 1.0 / 50, True).cpu().numpy()
        np.testing.assert_array_equal(data.qvel.view(np.uint32), qvel.view(np.uint32))
        assert np.any(qvel != post.infer_qvel(q, Lo, stac._timestep, True).cpu().numpy())
        # marks: the nearest input row of every output, clip by clip
        rows = (np.arange(3)[:, None] * L + post.resample_source_rows(L, U, D)[None, :]).reshape(-1)
        assert rows.tolist() == [c * L + r for c in range(3) for r in (0, 2, 5, 7, 10)]
        assert np.asarray(src.kp_gap).shape == (36, 23) and np.count_nonzero(src.kp_gap) == 4
        np.testing.assert_array_equal(data.kp_gap, np.asarray(src.kp_gap)[rows])
        assert np.count_nonzero(data.kp_gap) == 2  # rows 5 and 7 of the gap 5 .. 8
        assert np.asarray(data.kp_rejected).size == 0 and list(data.kp_names) == list(src.kp_names)
        np.testing.assert_array_equal(data.offsets, src.offsets)
    # the file run_stac wrote is resample_result of the first file with the config's keys, and a StacData is taken like its file
    stored = io.load_stac_data(resampled_path(path, 50))[1]
    again = stac.resample_result(src, 120, 50, lobes=2)
    for name in ("qpos", "kp_data", "xpos", "xquat", "marker_sites", "qvel", "kp_gap", "offsets"):
        np.testing.assert_array_equal(np.asarray(getattr(stored, name)), np.asarray(getattr(again, name)), err_msg=name)
    with pytest.raises(ValueError, match="5000 / 2997"):
        stac.resample_result(path, 29.97, 50)
