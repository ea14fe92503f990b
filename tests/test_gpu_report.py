"""The fit report on the GPU (stac.report): the kernels of csrc/stac_report.hip against the numpy float64 reference of
tests/report_cases.py -- tolerance 0 for everything but ``sum`` -- and ``run_stac`` end to end with the option.  Cases:
tests/report_cases.py."""

import ctypes as C
import json

import numpy as np
import pytest
import torch

import host_scaffold as hs
import prep_cases as pc
import report_cases as rc

pytestmark = pytest.mark.gpu

GUARD = 64
# what every output holds before the call (an element the call does not write shows), per dtype
PATTERNS = {torch.float32: -12345.0, torch.float64: -12345.0, torch.int32: -7, torch.int64: -7}
WORK_PATTERN = 0x7FF8_DEAD_BEEF_0123


def _lib():
    return hs.loaded_library()


def _tile():
    from stac_mjx_amd import report

    return report.TILE_FRAMES


def _out_specs(N, K, Q):
    return (("sqerr", torch.float32, (N, K)), ("frame_sse", torch.float64, (N,)), ("frame_n", torch.int32, (N,)),
            ("count", torch.int64, (K,)), ("sum", torch.float64, (K,)), ("max", torch.float32, (K,)), ("argmax", torch.int64, (K,)),
            ("hist", torch.int64, (K, 1024)), ("quant", torch.float32, (K, Q)))


def _buffers(N, K, Q, guard=0):
    """Flat output buffers pre-filled with a pattern, `guard` more elements behind each; a workspace of exactly the queried size
    (plus guard words) filled with a pattern of its own."""
    out = {}
    for name, dtype, shape in _out_specs(N, K, Q):
        out[name] = torch.full((int(np.prod(shape)) + guard,), PATTERNS[dtype], dtype=dtype, device="cuda")
    nbytes = _lib().stac_report_workspace(N, K, Q)
    assert nbytes > 0 and nbytes % 8 == 0
    work = torch.full((nbytes // 8 + guard,), WORK_PATTERN, dtype=torch.int64, device="cuda")
    return out, work, nbytes


def _raw(lib, markers, kp, gap, N, K, permille, out, work, nbytes, stream=None):
    from stac_mjx_amd import report

    perm = (C.c_int32 * len(permille))(*permille)
    p = report.Params(markers=markers.data_ptr(), kp=kp.data_ptr(), gap=gap.data_ptr() if gap is not None else None, n_frames=N, n_kp=K,
                      n_quant=len(permille), permille=perm, workspace=work.data_ptr(), workspace_bytes=nbytes, stream=stream,
                      **{k: v.data_ptr() for k, v in out.items()})
    return lib.stac_report_errors(C.byref(p))


def _results(out, N, K, Q):
    return {name: out[name][:int(np.prod(shape))].reshape(shape).cpu().numpy() for name, _, shape in _out_specs(N, K, Q)}


def _dev(a):
    return None if a is None else torch.as_tensor(np.array(a)).cuda()  # (a copy: the shared cases are read-only)


def _run_prefilled(lib, m_np, kp_np, gap_np, permille, twice=False):
    N, K = m_np.shape[:2]
    Q = len(permille)
    m, kp, gap = _dev(m_np), _dev(kp_np), _dev(gap_np)
    out, work, nbytes = _buffers(N, K, Q)
    rc_ = _raw(lib, m, kp, gap, N, K, permille, out, work, nbytes)
    assert rc_ == 0, lib.stac_last_error().decode()
    got = _results(out, N, K, Q)
    # the inputs are never written
    np.testing.assert_array_equal(m.cpu().numpy().view(np.uint32), m_np.view(np.uint32))
    np.testing.assert_array_equal(kp.cpu().numpy().view(np.uint32), kp_np.view(np.uint32))
    if gap is not None:
        np.testing.assert_array_equal(gap.cpu().numpy(), gap_np)
    if twice:  # a second call, on the workspace the first one left: every output bit for bit, `sum` included
        out2, _, _ = _buffers(N, K, Q)
        assert _raw(lib, m, kp, gap, N, K, permille, out2, work, nbytes) == 0, lib.stac_last_error().decode()
        again = _results(out2, N, K, Q)
        for name in got:
            np.testing.assert_array_equal(rc._bits(again[name]), rc._bits(got[name]), err_msg=f"second call: {name}")
    return got


@pytest.mark.parametrize("which", range(8))
def test_report_equals_reference(which):
    """N in {1, 2, 3, T-1, T, T+1, 2T+1, 5T+7} x K in {1, 2, 23, 70} x every pattern; Q in {1, 3, 8} by (pattern, K)."""
    tile = _tile()
    N = rc.shapes_N(tile)[which]
    lib = _lib()
    seen = set()
    for name, n, K, Q in rc.all_cases(tile):
        if n != N:
            continue
        m, kp, gap, permille, want = rc.reference(name, N, K, tile, Q)
        got = _run_prefilled(lib, m, kp, gap, permille, twice=(name in ("random", "exponent_spread")))
        rc.check(got, want, label=f"{name} N={N} K={K} Q={Q}")
        seen.add(Q)
    assert seen == {1, 3, 8}


def test_shapes_and_quantile_sets_are_those_of_the_issue():
    tile = _tile()
    assert rc.shapes_N(tile) == [1, 2, 3, tile - 1, tile, tile + 1, 2 * tile + 1, 5 * tile + 7] and rc.KS == (1, 2, 23, 70)
    assert len(rc.all_cases(tile)) == 8 * 4 * len(rc.PATTERNS) and len(rc.PATTERNS) == 11
    for name in rc.PATTERNS:
        assert {rc.n_quant_of(name, K) for K in rc.KS} == {1, 3, 8}
    assert any(0 in p and 1000 in p for p in rc.PERMILLE.values())


def test_long_series_beyond_one_sweep_of_the_grid():
    from stac_mjx_amd import report

    N, K = 70_000, 3
    assert (N + report.TILE_FRAMES - 1) // report.TILE_FRAMES > report.MAX_BLOCKS  # more tiles than workgroups: the grid strides
    assert N > report.SEG_FRAMES  # and more than one segment per keypoint in the counting passes
    rng = np.random.default_rng(21)
    kp = (0.05 * rng.standard_normal((N, K, 3))).astype(np.float32)
    m = kp + (0.001 * rng.standard_normal((N, K, 3)) * rng.lognormal(0.0, 1.0, (N, K, 1))).astype(np.float32)
    gap = np.where(rng.random((N, K)) < 0.05, 4, 0).astype(np.int32)
    kp[30_000:50_000, 1, :] = np.nan
    m[69_990, 2] += np.float32(0.5)
    kp = np.ascontiguousarray(kp.reshape(N, 3 * K))
    permille = (0, 500, 900, 990, 1000)
    want = rc.reference_report(m, kp, gap, permille)
    assert want["argmax"][2] == 69_990 and want["count"][1] < 50_000 < want["count"][0]
    got = _run_prefilled(_lib(), m, kp, gap, permille, twice=True)
    rc.check(got, want, label="long")


def test_raw_entry_point_guards_alignment_stream_and_aliasing():
    lib = _lib()
    tile = _tile()
    N, K, Q = 2 * tile + 1, 23, 3
    m_np, kp_np, gap_np, permille, want = rc.reference("random", N, K, tile, Q)
    n = m_np.size
    mbuf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    kbuf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    m, kp = mbuf[1:1 + n], kbuf[3:3 + n]  # inputs that are 4-byte aligned and no more
    assert m.data_ptr() % 4 == 0 and m.data_ptr() % 16 != 0 and kp.data_ptr() % 8 != 0
    gap = _dev(gap_np)
    out, work, nbytes = _buffers(N, K, Q, guard=GUARD)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        m.copy_(_dev(m_np.reshape(-1)))
        kp.copy_(_dev(kp_np.reshape(-1)))
        rc_ = _raw(lib, m, kp, gap, N, K, permille, out, work, nbytes, stream=stream.cuda_stream)
    assert rc_ == 0, lib.stac_last_error().decode()
    stream.synchronize()
    rc.check(_results(out, N, K, Q), want, label="raw")
    for name, dtype, shape in _out_specs(N, K, Q):  # the guard words behind every output
        tail = out[name][int(np.prod(shape)):].cpu().numpy()
        np.testing.assert_array_equal(tail, np.full(GUARD, PATTERNS[dtype], tail.dtype), err_msg=name)
    np.testing.assert_array_equal(work[nbytes // 8:].cpu().numpy(), np.full(GUARD, WORK_PATTERN, np.int64))  # and behind the workspace
    # aliased buffers are refused before anything is launched: the outputs keep what they hold
    before = {k: v.clone() for k, v in out.items()}
    for bad in (dict(sqerr=m), dict(markers=kp), dict(hist=work), dict(quant=out["max"]), dict(frame_sse=out["sum"]), dict(gap=out["frame_n"]),
                dict(count=out["hist"][8:]), dict(workspace=out["hist"])):
        args = dict(out)
        ins = dict(markers=m, kp=kp, gap=gap, workspace=work)
        for k, v in bad.items():
            (ins if k in ins else args)[k] = v
        rc_ = _raw(lib, ins["markers"], ins["kp"], ins["gap"], N, K, permille, args, ins["workspace"], nbytes)
        assert rc_ == -1 and "overlap" in lib.stac_last_error().decode(), (bad.keys(), lib.stac_last_error().decode())
    torch.cuda.synchronize()
    for k, v in out.items():
        assert torch.equal(v, before[k]), k


def test_wrapper_makes_inputs_contiguous_float32():
    from stac_mjx_amd import report

    tile = _tile()
    N, K, Q = tile + 1, 23, 3
    m_np, kp_np, gap_np, permille, want = rc.reference("random", N, K, tile, Q)
    wide = torch.as_tensor(np.concatenate([kp_np, kp_np], axis=1)).cuda().double()[:, :3 * K]  # float64, not contiguous
    m64 = _dev(m_np).double().permute(1, 0, 2).contiguous().permute(1, 0, 2)
    assert not wide.is_contiguous() and not m64.is_contiguous()
    keep = wide.clone()
    res = report.fit_errors(m64, wide, _dev(gap_np).long(), permille)
    assert all(v.is_cuda for v in res.values()) and res["sqerr"].dtype == torch.float32 and res["frame_sse"].dtype == torch.float64
    rc.check({k: v.cpu().numpy() for k, v in res.items()}, want, label="wrapper")
    assert torch.equal(wide, keep)
    # without gap and with the default quantiles
    want = rc.reference_report(m_np, kp_np, None, report.DEFAULT_PERMILLE)
    res = report.fit_errors(_dev(m_np), _dev(kp_np))
    rc.check({k: v.cpu().numpy() for k, v in res.items()}, want, label="wrapper, no gap")
    # N == 0: empty or neutral tensors, no call
    res = report.fit_errors(torch.zeros(0, K, 3, device="cuda"), torch.zeros(0, 3 * K, device="cuda"))
    assert res["sqerr"].shape == (0, K) and res["frame_sse"].numel() == 0 and not res["count"].any() and not res["hist"].any()
    assert (res["argmax"] == -1).all() and torch.isnan(res["max"]).all() and torch.isnan(res["quant"]).all() and not res["sum"].any()
    for bad in ((torch.zeros(4, 7, device="cuda"), torch.zeros(4, 21, device="cuda"), None),       # markers are not [N, K, 3]
                (torch.zeros(4, 7, 3, device="cuda"), torch.zeros(4, 20, device="cuda"), None),    # kp does not match
                (torch.zeros(4, 7, 3, device="cuda"), torch.zeros(5, 21, device="cuda"), None),
                (torch.zeros(4, 7, 3, device="cuda"), torch.zeros(4, 21, device="cuda"), torch.zeros(4, 6, device="cuda")),
                (torch.zeros(4, 7, 3, device="cuda"), torch.zeros(4, 21), None)):                  # a host tensor
        with pytest.raises(ValueError):
            report.fit_errors(*bad)


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
    """rodent_mocap[200:236] with the holes of tests/test_gpu_prep.py -> (holed series, gap of the reference fill)"""
    kp = np.array(rodent_mocap[200:236], dtype=np.float32)
    assert np.isfinite(kp).all() and kp.shape == (36, 69)
    kp[10:15, 3 * 3:3 * 3 + 3] = np.nan
    kp[0:2, 0:3] = np.nan
    kp[33:36, 3 * 22:3 * 22 + 3] = np.nan
    kp[20, 3 * 7 + 1] = np.nan
    gap = pc.reference_fill(kp, "linear")[1]
    kp.setflags(write=False)
    return kp, gap


def _dataset_names(path):
    from stac_mjx_amd import io

    if path.suffix == ".npz":
        with np.load(path) as f:
            return set(f.files)
    with io.h5py.File(path, "r") as f:
        return set(f.keys())


def _same_summary(got, want, counts):
    """Exact fields equal; rms within the bound of `sum`: |sum - fsum| <= n 2^-52 fsum, so the roots differ by at most half that,
    relatively (plus the rounding of the division and the root: 2^-52)."""
    assert set(got) == set(want) and got["n_frames"] == want["n_frames"] and got["permille"] == want["permille"]
    assert got["kp_names"] == want["kp_names"] and got["worst_frames"] == want["worst_frames"]
    for (name, g), (name_w, w) in zip(list(got["keypoints"].items()) + [("overall", got["overall"])],
                                      list(want["keypoints"].items()) + [("overall", want["overall"])]):
        assert name == name_w and set(g) == set(w)
        for field in g:
            if field == "rms":
                n = counts[name]
                print(f"report rms {name}: got {g[field]!r} reference {w[field]!r} n {n}")
                assert abs(g[field] - w[field]) <= (n + 2) * 2.0 ** -52 * w[field], (name, g[field], w[field])
            else:
                assert g[field] == w[field], (name, field, g[field], w[field])


def test_run_stac_report_on(tmp_path, rodent_setup, rodent_cfg, holed, capsys):
    from stac_mjx_amd import report
    from stac_mjx_amd.io import load_stac_data
    from stac_mjx_amd.main import report_path, run_stac
    from stac_mjx_amd.stac import Stac

    kp, ref_gap = holed
    names = rodent_setup.kp_names
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    capsys.readouterr()
    cfg_on = _cfg(rodent_cfg, fill_missing="linear", report="on")
    paths_on = run_stac(cfg_on, kp, names, base_path=tmp_path / "a", setup=rodent_setup)
    log = capsys.readouterr().out
    paths_off = run_stac(_cfg(rodent_cfg, fill_missing="linear"), kp, names, base_path=tmp_path / "b", setup=rodent_setup)
    assert sum(ln.startswith("report: wrote ") for ln in log.splitlines()) == 2
    assert sum(ln.startswith(f"report: {names[3]}: ") for ln in log.splitlines()) == 2  # one table line per keypoint and phase
    holes = {names[0]: (2, 2), names[3]: (2, 5), names[7]: (0, 1), names[22]: (0, 3)}  # gaps in the 12 fit frames, in the 36
    for phase, (p_on, p_off, rows) in enumerate(zip(paths_on, paths_off, (12, 36))):
        side = report_path(p_on)
        assert side.exists() and side.name == p_on.name + ".report.json" and not report_path(p_off).exists()
        doc = json.loads(side.read_text())
        _, d = load_stac_data(p_on)
        assert d.qpos.shape[0] == rows
        want_raw = rc.reference_report(d.marker_sites, d.kp_data, d.kp_gap, report.DEFAULT_PERMILLE)
        want = json.loads(json.dumps(report.summarize(want_raw, d.kp_names, worst=10)))
        counts = {n: int(c) for n, c in zip(d.kp_names, want_raw["count"])}
        counts["overall"] = int(want_raw["count"].sum())
        _same_summary(doc, want, counts)
        for name in names:  # the n of the holed keypoints are smaller by exactly their gap counts
            assert doc["keypoints"][name]["n"] == rows - holes.get(name, (0, 0))[phase], name
        np.testing.assert_array_equal(d.kp_gap, ref_gap[:rows])
        # the result files hold exactly the datasets they hold without the option, bit for bit
        assert _dataset_names(p_on) == _dataset_names(p_off)
        _, e = load_stac_data(p_off)
        for field in ("qpos", "xpos", "xquat", "marker_sites", "offsets", "kp_data", "kp_gap", "qvel"):
            x, y = np.asarray(getattr(d, field)), np.asarray(getattr(e, field))
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), field
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == sorted(p.name for p in paths_off)  # no sidecar without the option
    stac = Stac(None, cfg_on, names, setup=rodent_setup, verbose=False)
    assert stac.fit_report(paths_on[1]) == json.loads(report_path(paths_on[1]).read_text())
    assert stac.fit_report(load_stac_data(paths_on[1])[1], permille=(0, 1000), worst=2)["permille"] == [0, 1000]


def test_reference_marker_order_is_refused_before_any_work(tmp_path, rodent_setup, rodent_cfg, holed):
    from stac_mjx_amd.main import run_stac

    kp = np.nan_to_num(np.array(holed[0]))
    names = rodent_setup.kp_names
    with pytest.raises(ValueError, match="reference_marker_order"):
        run_stac(_cfg(rodent_cfg, report="on", reference_marker_order=True), kp, names, base_path=tmp_path, setup=rodent_setup)
    assert not list(tmp_path.iterdir())  # nothing was fitted or written
