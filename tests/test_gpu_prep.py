"""fill_missing on the GPU (stac.fill_missing): the staged kernels of csrc/stac_prep.hip against the numpy float64 reference of
tests/prep_cases.py, tolerance 0, and ``run_stac`` end to end with the option.  Cases: tests/prep_cases.py."""

import ctypes as C

import numpy as np
import pytest
import torch

import host_scaffold as hs
import prep_cases as pc

pytestmark = pytest.mark.gpu

PATTERN, GAP_PATTERN, GUARD = -12345.0, -7, 64


def _lib():
    return hs.loaded_library()


def _raw(lib, kp, T, K, mode, out, gap, work, nbytes, stream=None):
    from stac_mjx_amd import prep

    return lib.stac_prep_fill(C.c_void_p(kp.data_ptr()), T, K, prep.MODES[mode], C.c_void_p(out.data_ptr()), C.c_void_p(gap.data_ptr()),
                              C.c_void_p(work.data_ptr()), nbytes, C.c_void_p(stream) if stream else None)


def _fill_prefilled(lib, kp_np, mode):
    """The entry point on outputs pre-filled with a pattern (an element it does not write shows), on a workspace of exactly
    the queried size filled with a pattern of its own (its contents must not matter)."""
    T, K = kp_np.shape[0], kp_np.shape[1] // 3
    kp = torch.as_tensor(np.array(kp_np)).cuda()  # (a copy: the shared cases are read-only)
    out = torch.full((T, 3 * K), PATTERN, dtype=torch.float32, device="cuda")
    gap = torch.full((T, K), GAP_PATTERN, dtype=torch.int32, device="cuda")
    nbytes = lib.stac_prep_fill_workspace(T, K)
    work = torch.full((nbytes // 8,), 0x7FF8_DEAD_BEEF_0123, dtype=torch.int64, device="cuda")
    rc = _raw(lib, kp, T, K, mode, out, gap, work, nbytes)
    assert rc == 0, lib.stac_last_error().decode()
    np.testing.assert_array_equal(kp.cpu().numpy().view(np.uint32), kp_np.view(np.uint32))  # the source is never written
    return out.cpu().numpy(), gap.cpu().numpy()


def _tile():
    from stac_mjx_amd import prep

    return prep.TILE_FRAMES


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("which", range(8))
def test_fill_equals_reference(which, mode):
    """T in {1, 2, 3, TILE-1, TILE, TILE+1, 2 TILE+1, 5 TILE+7} x K in {1, 2, 23, 70} x every pattern."""
    tile = _tile()
    T = pc.shapes_T(tile)[which]
    lib = _lib()
    for K in pc.KS:
        for name in pc.PATTERNS:
            kp, want_out, want_gap = pc.reference(name, T, K, tile, mode)
            out, gap = _fill_prefilled(lib, kp, mode)
            pc.check(out, gap, kp, want_out, want_gap, label=f"{name} T={T} K={K} {mode}")


def test_shapes_are_the_eight_of_the_issue():
    tile = _tile()
    assert pc.shapes_T(tile) == [1, 2, 3, tile - 1, tile, tile + 1, 2 * tile + 1, 5 * tile + 7]


@pytest.fixture(scope="module")
def long_series():
    """T = 70 000, K = 3: 30 % random holes, one run of 20 000 frames, a leading and a trailing run."""
    T, K = 70_000, 3
    rng = np.random.default_rng(11)
    x = pc.base_series(T, K, 12)
    x[rng.random((T, K)) < 0.3] = np.nan
    x[30_000:50_000, 1, :] = np.nan
    x[:700, 0, 2] = np.inf
    x[T - 900:, 2, 0] = -np.inf
    kp = np.ascontiguousarray(x.reshape(T, 3 * K))
    kp.setflags(write=False)
    return kp


@pytest.mark.parametrize("mode", pc.MODES)
def test_long_series_beyond_one_sweep_of_the_grid(long_series, mode):
    from stac_mjx_amd import prep

    T, K = long_series.shape[0], long_series.shape[1] // 3
    assert T > prep.MAX_BLOCKS * prep.TILE_FRAMES  # more tiles than workgroups: the grid strides
    want_out, want_gap = pc.reference_fill(long_series, mode)
    assert want_gap[:, 1].max() >= 20_000 and want_gap[0, 0] >= 700 and want_gap[T - 1, 2] >= 900
    out, gap = _fill_prefilled(_lib(), long_series, mode)
    pc.check(out, gap, long_series, want_out, want_gap, label=f"long {mode}")
    s = prep.summary(torch.as_tensor(gap).cuda())
    np.testing.assert_array_equal(s["missing"], np.count_nonzero(want_gap, axis=0))
    np.testing.assert_array_equal(s["longest"], want_gap.max(axis=0))
    assert s["empty"] == []


def test_raw_entry_point_guards_alignment_stream_and_aliasing():
    lib = _lib()
    tile = _tile()
    T, K, mode = 2 * tile + 1, 23, "linear"
    kp_np, want_out, want_gap = pc.reference("random_30_percent", T, K, tile, mode)
    n = kp_np.size
    sbuf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    src = sbuf[1:1 + n]
    assert src.data_ptr() % 4 == 0 and src.data_ptr() % 16 != 0
    obuf = torch.full((n + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    gbuf = torch.full((T * K + GUARD,), GAP_PATTERN, dtype=torch.int32, device="cuda")
    nbytes = lib.stac_prep_fill_workspace(T, K)
    wbuf = torch.full((nbytes // 8 + GUARD,), -3, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        src.copy_(torch.as_tensor(np.array(kp_np.reshape(-1))).cuda())
        rc = _raw(lib, src, T, K, mode, obuf, gbuf, wbuf, nbytes, stream=stream.cuda_stream)
    assert rc == 0, lib.stac_last_error().decode()
    stream.synchronize()
    out, gap = obuf.cpu().numpy(), gbuf.cpu().numpy()
    pc.check(out[:n].reshape(T, 3 * K), gap[:T * K].reshape(T, K), kp_np, want_out, want_gap, label="raw")
    np.testing.assert_array_equal(out[n:], np.full(GUARD, PATTERN, np.float32))       # the guard words behind out,
    np.testing.assert_array_equal(gap[T * K:], np.full(GUARD, GAP_PATTERN, np.int32))  # behind gap
    np.testing.assert_array_equal(wbuf[nbytes // 8:].cpu().numpy(), np.full(GUARD, -3, np.int64))  # and behind the workspace
    # aliased buffers are refused before anything is launched: the outputs keep what they hold
    before = obuf.clone()
    for bad in (dict(out=src), dict(out=sbuf), dict(gap=obuf), dict(work=obuf), dict(kp=obuf[4:])):
        args = dict(kp=src, out=obuf, gap=gbuf, work=wbuf)
        args.update(bad)
        rc = _raw(lib, args["kp"], T, K, mode, args["out"], args["gap"], args["work"], nbytes)
        assert rc == -1 and "overlap" in lib.stac_last_error().decode(), bad.keys()
    torch.cuda.synchronize()
    assert torch.equal(obuf, before)


def test_wrapper_makes_inputs_contiguous_float32():
    from stac_mjx_amd import prep

    tile = _tile()
    T, K = tile + 1, 23
    for mode in pc.MODES:
        kp_np, want_out, want_gap = pc.reference("random_30_percent", T, K, tile, mode)
        wide = torch.as_tensor(np.concatenate([kp_np, kp_np], axis=1)).cuda().double()[:, :3 * K]  # float64, not contiguous
        assert not wide.is_contiguous()
        out, gap = prep.fill_missing(wide, mode)
        assert out.is_cuda and out.dtype == torch.float32 and gap.dtype == torch.int32 and tuple(gap.shape) == (T, K)
        pc.check(out.cpu().numpy(), gap.cpu().numpy(), kp_np, want_out, want_gap, label=f"wrapper {mode}")
        assert torch.isnan(wide).any()  # the caller's tensor is not filled in place
    with pytest.raises(ValueError):
        prep.fill_missing(torch.zeros(4, 7, device="cuda"))  # 7 columns are not keypoints of three


# ---- run_stac end to end --------------------------------------------------------------------------------------------------------
def _cfg(rodent_cfg, **stac_over):
    from stac_mjx_amd.config import validate_config

    stac = dict(fit_offsets_path="fit.h5", ik_only_path="ik.h5", data_path="d.mat", continuous=False, n_fit_frames=12,
                skip_fit_offsets=False, skip_ik_only=False, infer_qvels=False, n_frames_per_clip=12,
                mujoco=dict(solver="newton", iterations=1, ls_iterations=4))
    stac.update(stac_over)
    cfg = validate_config({"model": dict(rodent_cfg), "stac": stac})
    cfg.model.N_ITER_Q = 30
    cfg.model.N_ITERS = 1
    return cfg


@pytest.fixture(scope="module")
def holed(rodent_mocap):
    """rodent_mocap[200:236] with the holes of the issue -> (holed series, reference out, reference gap)"""
    kp = np.array(rodent_mocap[200:236], dtype=np.float32)
    assert np.isfinite(kp).all() and kp.shape == (36, 69)
    kp[10:15, 3 * 3:3 * 3 + 3] = np.nan    # keypoint 3, frames 10-14: across the clip border at 12 (and n_fit_frames)
    kp[0:2, 0:3] = np.nan                  # keypoint 0, frames 0-1: a leading run
    kp[33:36, 3 * 22:3 * 22 + 3] = np.nan  # keypoint 22, frames 33-35: a trailing run
    kp[20, 3 * 7 + 1] = np.nan             # the y of keypoint 7 in frame 20
    out, gap = pc.reference_fill(kp, "linear")
    assert np.count_nonzero(gap) == 5 + 2 + 3 + 1
    for a in (kp, out, gap):
        a.setflags(write=False)
    return kp, out, gap


def _load_both(paths):
    from stac_mjx_amd.io import load_stac_data

    return [load_stac_data(p) for p in paths]


def test_run_stac_fill_missing_linear(tmp_path, rodent_setup, rodent_cfg, holed, capsys):
    from stac_mjx_amd.io import _DATASETS
    from stac_mjx_amd.main import run_stac

    kp, ref_out, ref_gap = holed
    names = rodent_setup.kp_names
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    capsys.readouterr()
    with_option = _load_both(run_stac(_cfg(rodent_cfg, fill_missing="linear"), kp, names, base_path=tmp_path / "a", setup=rodent_setup))
    log = capsys.readouterr().out
    lines = [ln for ln in log.splitlines() if ln.startswith("fill_missing (linear):")]
    assert len(lines) == 4, log  # one line per keypoint that had gaps: its count and its longest run
    for k, count, longest in ((0, 2, 2), (3, 5, 5), (7, 1, 1), (22, 3, 3)):
        (ln,) = [ln for ln in lines if f" {names[k]}: " in ln]
        assert f"{count} of 36 frames" in ln and f"longest run {longest}" in ln, ln
    assert "of the 12 fit frames are filled" in log
    # the same run with the option off on the series the numpy reference filled beforehand
    without = _load_both(run_stac(_cfg(rodent_cfg), np.array(ref_out), names, base_path=tmp_path / "b", setup=rodent_setup))
    for (cfg_a, a), (cfg_b, b), rows in zip(with_option, without, (12, 36)):
        for name in _DATASETS:  # every output is finite; everything but kp_gap is bit-equal: the fit saw the same numbers
            x, y = np.asarray(getattr(a, name)), np.asarray(getattr(b, name))
            assert np.isfinite(x).all(), name
            assert x.shape == y.shape and x.dtype == y.dtype, (name, x.shape, y.shape)
            np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y,
                                          err_msg=name)
        assert a.qpos.shape[0] == rows and (a.names_qpos, a.names_xpos, a.kp_names) == (b.names_qpos, b.names_xpos, b.kp_names)
        np.testing.assert_array_equal(a.kp_data.view(np.uint32), ref_out[:rows].view(np.uint32))
        assert a.kp_gap.dtype == np.int32
        np.testing.assert_array_equal(a.kp_gap, ref_gap[:rows])
        assert b.kp_gap.size == 0
        da, db = cfg_a.to_dict(), cfg_b.to_dict()  # the stored configs differ in the one key
        assert da["stac"].pop("fill_missing") == "linear" and "fill_missing" not in db["stac"] and da == db


def test_run_stac_fill_missing_continuous_postprocess_gpu(tmp_path, rodent_setup, rodent_cfg, holed):
    from stac_mjx_amd.io import load_stac_data
    from stac_mjx_amd.main import run_stac

    kp, ref_out, ref_gap = holed
    cfg = _cfg(rodent_cfg, fill_missing="linear", continuous=True, postprocess="gpu")
    fit_path, ik_path = run_stac(cfg, kp, rodent_setup.kp_names, base_path=tmp_path, setup=rodent_setup)
    d = load_stac_data(ik_path)[1]
    assert d.qpos.shape[0] == 36 and np.isfinite(d.qpos).all() and np.isfinite(d.kp_data).all() and np.isfinite(d.marker_sites).all()
    np.testing.assert_array_equal(d.kp_gap, ref_gap)  # the input's 36 rows, not cross-faded
    np.testing.assert_array_equal(load_stac_data(fit_path)[1].kp_gap, ref_gap[:12])


def test_run_stac_empty_track_raises_before_any_fit(tmp_path, rodent_setup, rodent_cfg, holed):
    from stac_mjx_amd.main import run_stac
    from stac_mjx_amd.stac import Stac

    kp = np.array(holed[0])
    kp[:, 3 * 5:3 * 5 + 3] = np.nan
    kp[:, 3 * 9 + 2] = np.inf
    names = rodent_setup.kp_names
    with pytest.raises(ValueError, match=names[5]) as e:
        run_stac(_cfg(rodent_cfg, fill_missing="hold"), kp, names, base_path=tmp_path, setup=rodent_setup)
    assert names[9] in str(e.value)  # every empty keypoint is named
    assert not list(tmp_path.iterdir())  # nothing was fitted or written
    stac = Stac(None, _cfg(rodent_cfg), names, setup=rodent_setup, verbose=False)
    filled, gap = stac.fill_missing(holed[0], "hold")  # the method on its own: numpy in, numpy out
    want_out, want_gap = pc.reference_fill(holed[0], "hold")
    pc.check(filled, gap, holed[0], want_out, want_gap, label="Stac.fill_missing hold")
    with pytest.raises(ValueError):
        stac.fill_missing(holed[0])  # the config says off: there is no mode to fill with
