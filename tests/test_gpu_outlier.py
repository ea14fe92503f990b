"""reject_outliers on the GPU (stac.reject_outliers): the kernel of csrc/stac_outlier.hip against the numpy float64 reference of
tests/outlier_cases.py, tolerance 0, and ``run_stac`` end to end with the option.  Cases: tests/outlier_cases.py."""

import ctypes as C

import numpy as np
import pytest
import torch

import host_scaffold as hs
import outlier_cases as oc
import prep_cases as pc

pytestmark = pytest.mark.gpu

PATTERN, FLAG_PATTERN, GUARD = -12345.0, 0xEE, 64


def _lib():
    return hs.loaded_library()


def _tile():
    from stac_mjx_amd import prep

    return prep.TILE_FRAMES


def _raw(lib, kp, T, K, h, thr, min_dev, out, flag, stream=None):
    """kp / out / flag: tensors or raw addresses"""
    addr = lambda a: C.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a) if a is not None else None  # noqa: E731
    return lib.stac_prep_reject(addr(kp), T, K, h, thr, min_dev, addr(out), addr(flag), C.c_void_p(stream) if stream else None)


def _reject_prefilled(lib, kp_np, h, min_dev):
    """The entry point on outputs pre-filled with a pattern: an element it does not write shows."""
    T, K = kp_np.shape[0], kp_np.shape[1] // 3
    kp = torch.as_tensor(np.array(kp_np)).cuda()  # (a copy: the shared cases are read-only)
    out = torch.full((T, 3 * K), PATTERN, dtype=torch.float32, device="cuda")
    flag = torch.full((T, K), FLAG_PATTERN, dtype=torch.uint8, device="cuda")
    rc = _raw(lib, kp, T, K, h, oc.THR, min_dev, out, flag)
    assert rc == 0, lib.stac_last_error().decode()
    np.testing.assert_array_equal(kp.cpu().numpy().view(np.uint32), kp_np.view(np.uint32))  # the source is never written
    return out.cpu().numpy(), flag.cpu().numpy()


@pytest.mark.parametrize("h", oc.HS)
def test_reject_equals_reference(h):
    """``mixed`` at every T x K of the issue, and every pattern on its own with and without the floor, for this half-width."""
    tile, lib = _tile(), _lib()
    cases = [c for c in oc.cases(tile) if c[1] == h]
    assert {c[2] for c in cases} == set(oc.shapes_T(h, tile)) and {c[0] for c in cases} == set(oc.PATTERNS) | {oc.MIXED}
    rejected = 0
    for name, _, T, K, min_dev in cases:
        kp, want_out, want_flag = oc.reference(name, h, T, K, tile, min_dev)
        out, flag = _reject_prefilled(lib, kp, h, min_dev)
        oc.check(out, flag, kp, want_out, want_flag, label=f"{name} h={h} T={T} K={K} min_dev={min_dev}")
        rejected += int(want_flag.sum())
    assert rejected > 100  # (the cases do reject)


@pytest.mark.parametrize("h", (5, 16))
def test_long_series_beyond_one_sweep_of_the_grid(h):
    """T = 70 000, K = 3: more tiles than workgroups, so the grid strides.  The series repeats a block of P = 1 000 frames (spikes,
    NaN runs, infinities).  A decision reads the frames t - h .. t + h only and h < P, so the reference of the long series is
    the reference of three blocks: its first block for the first, its middle block for every inner one, its last for the last.
    1 000 is no multiple of the tile, so the blocks meet the tile borders at 8 different phases."""
    from stac_mjx_amd import prep

    P, reps, K = 1000, 70, 3
    T = P * reps
    assert T > prep.MAX_BLOCKS * prep.TILE_FRAMES and h < P
    rng = np.random.default_rng(70_000 + h)
    block = np.stack([oc.smooth_track(P, rng) for _ in range(K)], axis=1)  # [P, K, 3]
    for k in range(K):
        oc._spike(block[:, k], np.flatnonzero(rng.random(P) < 0.04), rng)
    block[rng.random((P, K)) < 0.1] = np.nan
    block[100:100 + 2 * h + 3, 1] = np.nan
    block[500, 0, 2] = np.inf
    block[0, 2] += np.float32(0.2)      # on the seam between two blocks, and on the first and last frame of the series
    block[P - 1, 0] -= np.float32(0.2)
    three = np.ascontiguousarray(np.tile(block, (3, 1, 1)).reshape(3 * P, 3 * K))
    out3, flag3 = oc.reference_reject(three, h, oc.THR, 0.001)
    pick = lambda a: np.concatenate([a[:P]] + [a[P:2 * P]] * (reps - 2) + [a[2 * P:]], axis=0)  # noqa: E731
    kp = np.ascontiguousarray(np.tile(block, (reps, 1, 1)).reshape(T, 3 * K))
    want_out, want_flag = pick(out3), pick(flag3)
    assert 0.01 < want_flag.mean() < 0.2 and not np.array_equal(flag3[P:2 * P], flag3[2 * P:])  # (the ends of the series do differ)
    out, flag = _reject_prefilled(_lib(), kp, h, 0.001)
    oc.check(out, flag, kp, want_out, want_flag, label=f"long h={h}")
    # the wrapper on the same series: thr = n_sigma * 1.4826 computed in Python
    o2, f2 = prep.reject_outliers(torch.as_tensor(kp).cuda(), half_window=h, n_sigma=3.0, min_dev=0.001)
    oc.check(o2.cpu().numpy(), f2.cpu().numpy(), kp, want_out, want_flag, label=f"long wrapper h={h}")


def test_raw_entry_point_guards_alignment_stream_and_errors():
    lib, tile = _lib(), _tile()
    h, T, K, min_dev = 5, 2 * tile + 1, 23, 0.01
    kp_np, want_out, want_flag = oc.reference(oc.MIXED, h, T, K, tile, min_dev)
    n = kp_np.size
    sbuf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    src = sbuf[1:1 + n]
    assert src.data_ptr() % 4 == 0 and src.data_ptr() % 16 != 0
    obuf = torch.full((n + GUARD,), PATTERN, dtype=torch.float32, device="cuda")
    fbuf = torch.full((T * K + GUARD,), FLAG_PATTERN, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        src.copy_(torch.as_tensor(np.array(kp_np.reshape(-1))).cuda())
        rc = _raw(lib, src, T, K, h, oc.THR, min_dev, obuf, fbuf, stream=stream.cuda_stream)
    assert rc == 0, lib.stac_last_error().decode()
    stream.synchronize()
    out, flag = obuf.cpu().numpy(), fbuf.cpu().numpy()
    oc.check(out[:n].reshape(T, 3 * K), flag[:T * K].reshape(T, K), kp_np, want_out, want_flag, label="raw")
    np.testing.assert_array_equal(out[n:], np.full(GUARD, PATTERN, np.float32))         # the guard words behind out
    np.testing.assert_array_equal(flag[T * K:], np.full(GUARD, FLAG_PATTERN, np.uint8))  # and behind flag
    # every refusal happens before anything is launched: the outputs keep what they hold
    obuf.fill_(PATTERN)
    fbuf.fill_(FLAG_PATTERN)
    torch.cuda.synchronize()
    good = dict(kp=src, T=T, K=K, h=h, thr=oc.THR, min_dev=min_dev, out=obuf, flag=fbuf)
    bad = [dict(kp=None), dict(out=None), dict(flag=None), dict(T=0), dict(T=-1), dict(K=0), dict(K=-2), dict(h=0), dict(h=17), dict(h=-5),
           dict(thr=-1.0), dict(thr=float("nan")), dict(thr=float("inf")), dict(min_dev=-1e-12), dict(min_dev=float("nan")),
           dict(min_dev=float("-inf")), dict(kp=src.data_ptr() + 2), dict(out=obuf.data_ptr() + 1),
           dict(out=src), dict(out=sbuf), dict(kp=obuf[4:]), dict(flag=obuf), dict(flag=src), dict(out=fbuf), dict(kp=fbuf)]  # in place, overlaps
    for over in bad:
        a = {**good, **over}
        rc = _raw(lib, a["kp"], a["T"], a["K"], a["h"], a["thr"], a["min_dev"], a["out"], a["flag"])
        assert rc == -1 and lib.stac_last_error_code() == -1, (list(over), rc)
    torch.cuda.synchronize()
    assert bool((obuf == PATTERN).all()) and bool((fbuf == FLAG_PATTERN).all())


def test_wrapper_input_handling_and_empty_series():
    from stac_mjx_amd import prep

    tile = _tile()
    h, T, K, min_dev = 5, 2 * tile + 1, 23, 0.01
    kp_np, want_out, want_flag = oc.reference(oc.MIXED, h, T, K, tile, min_dev)
    wide = torch.as_tensor(np.concatenate([kp_np, kp_np], axis=1)).cuda()[:, :3 * K]  # not contiguous
    assert not wide.is_contiguous()
    before = wide.clone()
    out, flag = prep.reject_outliers(wide, half_window=h, n_sigma=3.0, min_dev=min_dev)
    assert out.is_cuda and out.dtype == torch.float32 and flag.dtype == torch.uint8 and tuple(flag.shape) == (T, K)
    oc.check(out.cpu().numpy(), flag.cpu().numpy(), kp_np, want_out, want_flag, label="wrapper")
    assert torch.equal(wide.contiguous().view(torch.int32), before.contiguous().view(torch.int32))  # the caller's tensor is not written
    out, flag = prep.reject_outliers(torch.zeros(0, 6, device="cuda"))  # T == 0: empty tensors without a call
    assert tuple(out.shape) == (0, 6) and tuple(flag.shape) == (0, 2) and flag.dtype == torch.uint8
    with pytest.raises(ValueError):
        prep.reject_outliers(torch.zeros(4, 7, device="cuda"))  # 7 columns are not keypoints of three
    with pytest.raises(ValueError):
        prep.reject_outliers(torch.zeros(4, 6, device="cuda"), half_window=17)


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


SPIKES = ((5, 3), (5, 10), (6, 17), (17, 0), (17, 15), (18, 8), (29, 22), (29, 7), (30, 12))  # (frame, keypoint): 8 cm, single frames


@pytest.fixture(scope="module")
def spiked(rodent_mocap):
    """rodent_mocap[200:236], clean and with the spikes -> (clean, spiked, reference out, reference flag, the reference's fill)"""
    clean = np.array(rodent_mocap[200:236], dtype=np.float32)
    assert np.isfinite(clean).all() and clean.shape == (36, 69)
    kp = clean.copy()
    for i, (t, k) in enumerate(SPIKES):
        kp[t, 3 * k + i % 3] += np.float32(0.08 if i % 2 else -0.08)
    out, flag = oc.reference_reject(kp, 5, oc.THR, 0.001)  # the defaults of the config keys
    assert all(flag[t, k] == 1 for t, k in SPIKES)  # (a condition on the inputs: every injected spike is one to the reference)
    filled, gap = pc.reference_fill(out, "linear")
    for a in (clean, kp, out, flag, filled, gap):
        a.setflags(write=False)
    return clean, kp, out, flag, filled, gap


def _load_both(paths):
    from stac_mjx_amd.io import load_stac_data

    return [load_stac_data(p)[1] for p in paths]


def test_run_stac_reject_outliers_hampel(tmp_path, rodent_setup, rodent_cfg, spiked, capsys):
    from stac_mjx_amd.io import _DATASETS
    from stac_mjx_amd.main import run_stac

    clean, kp, ref_out, ref_flag, ref_filled, ref_gap = spiked
    names = rodent_setup.kp_names

    def run(tag, data, **over):
        (tmp_path / tag).mkdir()
        return _load_both(run_stac(_cfg(rodent_cfg, **over), np.array(data), names, base_path=tmp_path / tag, setup=rodent_setup))

    base = run("clean", clean)
    capsys.readouterr()
    with_rejection = run("hampel", kp, fill_missing="linear", reject_outliers="hampel")
    log = capsys.readouterr().out
    without = run("absent", kp, fill_missing="linear")
    off = run("off", kp, fill_missing="linear", reject_outliers="off", outlier_window=3, outlier_nsigma=2.0, outlier_min_dev=0.0)

    # one log line per keypoint that had rejections (count and share), one about the fit frames
    lines = [ln for ln in log.splitlines() if ln.startswith("reject_outliers (hampel")]
    counts = ref_flag.sum(axis=0)
    assert len(lines) == np.count_nonzero(counts), log
    for k in np.flatnonzero(counts):
        (ln,) = [ln for ln in lines if f" {names[k]}: " in ln]
        assert f"{int(counts[k])} of 36 frames rejected" in ln and "%" in ln, ln
    assert "of the 12 fit frames were rejected as outliers" in log and "of the 12 fit frames are filled" in log

    for d, rows in zip(with_rejection, (12, 36)):
        assert d.kp_rejected.dtype == np.uint8
        np.testing.assert_array_equal(d.kp_rejected, ref_flag[:rows])     # the reference's flags, in both files
        assert (d.kp_gap[d.kp_rejected == 1] > 0).all()                   # the fill saw them as missing
        np.testing.assert_array_equal(d.kp_gap, ref_gap[:rows])
        np.testing.assert_array_equal(d.kp_data.view(np.uint32), ref_filled[:rows].view(np.uint32))  # bit for bit
        assert np.isfinite(d.qpos).all() and d.qpos.shape[0] == rows

    # over the spiked frames the poses are nearer to those of the clean series with rejection than without: two runs of this test
    frames = sorted({t for t, _ in SPIKES})
    q_clean, q_with, q_without = base[1].qpos[frames], with_rejection[1].qpos[frames], without[1].qpos[frames]
    err_with, err_without = np.abs(q_with - q_clean).mean(), np.abs(q_without - q_clean).mean()
    print(f"mean |qpos - clean| over the spiked frames: {err_with:.6f} with rejection, {err_without:.6f} without")
    assert err_with < err_without, (err_with, err_without)

    # with the key absent: no kp_rejected, and every dataset equals that of a run whose config names the feature's keys but leaves it off
    for a, b in zip(without, off):
        assert a.kp_rejected.size == 0 and b.kp_rejected.size == 0
        for name in _DATASETS + ("kp_gap",):
            x, y = np.asarray(getattr(a, name)), np.asarray(getattr(b, name))
            assert x.shape == y.shape and x.dtype == y.dtype, name
            np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y,
                                          err_msg=name)
        np.testing.assert_array_equal(a.kp_data.view(np.uint32), kp[:a.kp_data.shape[0]].view(np.uint32))  # spikes and all
    files = [p for p in (tmp_path / "absent").iterdir() if p.suffix in (".h5", ".npz")]
    assert len(files) == 2 and all("kp_rejected" not in _names(p) for p in files)


def _names(path):
    from stac_mjx_amd import io

    if path.suffix == ".npz":
        with np.load(path) as f:
            return set(f.files)
    with io.h5py.File(path, "r") as f:
        return set(f.keys())


def test_stac_method_on_its_own(rodent_setup, rodent_cfg, spiked):
    from stac_mjx_amd.stac import Stac

    _, kp, ref_out, ref_flag, _, _ = spiked
    stac = Stac(None, _cfg(rodent_cfg), rodent_setup.kp_names, setup=rodent_setup, verbose=False)
    out, flag = stac.reject_outliers(kp)  # numpy in, numpy out; the defaults are the config's
    oc.check(out, flag, kp, ref_out, ref_flag, label="Stac.reject_outliers")
    with pytest.raises(ValueError):
        stac.reject_outliers(kp[:, :66])
    with pytest.raises(ValueError):
        stac.reject_outliers(kp, half_window=0)
