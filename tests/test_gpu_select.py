"""Choosing calibration frames on the GPU (stac.fit_frames: diverse): the three kernels of csrc/select/stac_select.hip against the CPU
build of the rule of csrc/select/stac_select.hpp (tests/select_cases.py), tolerance 0 on ``sel``, ``n_selected`` and the bits of
``radius2``; and ``run_stac`` end to end with the option.  Cases: tests/select_cases.py."""

import ctypes as C
import json
import re

import numpy as np
import pytest
import torch

import host_scaffold as hs
import select_cases as sc

pytestmark = pytest.mark.gpu

SEL_PATTERN, R2_PATTERN, N_PATTERN, WORK_PATTERN, GUARD = -12345, -7.5, -99, 0xFF, 64


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return sc.cpu_rule(tmp_path_factory)[0]


@pytest.fixture(scope="module")
def lib():
    from stac_mjx_amd.build import build_extension
    from stac_mjx_amd.engine import load_select_library

    build_extension()
    return load_select_library()


@pytest.fixture(scope="module")
def side_stream():
    return torch.cuda.Stream()


class _Buffers:
    """Inputs, pre-filled outputs with ``GUARD`` elements around each, and a workspace of 0xFF bytes, on the device"""

    def __init__(self, lib, kp_np, cand_np, n):
        self.T, self.K, self.n = kp_np.shape[0], kp_np.shape[1] // 3, n
        self.kp = torch.as_tensor(np.array(kp_np.reshape(-1))).cuda()
        self.cand = None if cand_np is None else torch.as_tensor(np.array(cand_np, dtype=np.uint8)).cuda()
        self.nbytes = lib.stac_select_workspace(self.T, self.K)
        assert self.nbytes >= 8, lib.stac_select_last_error().decode()
        self.fill()

    def fill(self):
        self.whole = {}
        for name, count, dtype, pattern in (("sel", self.n, torch.int64, SEL_PATTERN), ("radius2", self.n, torch.float32, R2_PATTERN),
                                            ("n_selected", 1, torch.int64, N_PATTERN), ("work", (self.nbytes + 7) // 8 * 8, torch.uint8, WORK_PATTERN)):
            whole = torch.full((GUARD + count + GUARD,), pattern, dtype=dtype, device="cuda")
            self.whole[name] = (whole, count, pattern)
            setattr(self, name, whole[GUARD:GUARD + count])
        assert self.work.data_ptr() % 8 == 0

    def call(self, lib, stream=None, **over):
        a = dict(kp=self.kp, T=self.T, K=self.K, cand=self.cand, n=self.n, sel=self.sel, radius2=self.radius2, n_selected=self.n_selected,
                 work=self.work, nbytes=self.nbytes)
        a.update(over)
        addr = lambda v: C.c_void_p(v.data_ptr() if isinstance(v, torch.Tensor) else v) if v is not None else None  # noqa: E731
        return lib.stac_select_diverse(addr(a["kp"]), a["T"], a["K"], addr(a["cand"]), a["n"], addr(a["sel"]), addr(a["radius2"]),
                                       addr(a["n_selected"]), addr(a["work"]), a["nbytes"], C.c_void_p(stream) if stream else None)

    def results(self):
        """-> (sel, radius2, n_selected) as numpy arrays / an int, without their guards; asserts that every guard word holds its pattern"""
        for name, (whole, count, pattern) in self.whole.items():
            assert bool((whole[:GUARD] == pattern).all()) and bool((whole[GUARD + count:] == pattern).all()), f"guard words around {name}"
        return self.sel.cpu().numpy(), self.radius2.cpu().numpy(), int(self.n_selected.item())

    def untouched(self):
        return all(bool((whole == pattern).all()) for whole, _, pattern in self.whole.values())


def _check(lib, rule, label, kp, cand, n, stream):
    """One case on ``stream``: outputs pre-filled with a pattern and the workspace poisoned to 0xFF, tolerance 0 against the CPU rule;
    a second call into freshly poisoned outputs (on the workspace the first one left) equals the first bit for bit."""
    want_sel, want_r2, want_n = rule(kp, cand, n)
    b = _Buffers(lib, kp, cand, n)
    torch.cuda.synchronize()
    got = []
    for _ in range(2):
        with torch.cuda.stream(stream):
            rc = b.call(lib, stream=stream.cuda_stream)
        assert rc == 0, lib.stac_select_last_error().decode()
        stream.synchronize()
        sel, r2, n_sel = b.results()
        assert n_sel == want_n, (label, n_sel, want_n)
        np.testing.assert_array_equal(sel, want_sel, err_msg=label)  # (every element written: the tails are -1, never the pattern)
        np.testing.assert_array_equal(r2.view(np.uint32), want_r2.view(np.uint32), err_msg=label)
        got.append((sel, r2, n_sel))
        work = b.work
        b.fill()
        b.work.copy_(work)  # (what the first call left, not the pattern)
        torch.cuda.synchronize()
    return got[0]


@pytest.mark.parametrize("T", sc.TS)
@pytest.mark.parametrize("K", sc.KS)
def test_select_equals_the_rule(lib, rule, side_stream, K, T):
    for label, kp, cand, n in sc.shape_cases(K, T):
        _check(lib, rule, label, kp, cand, n, side_stream)


def test_select_on_the_edges(lib, rule, side_stream):
    got = {}
    for label, kp, cand, n in sc.edge_cases():
        got[label] = _check(lib, rule, label, kp, cand, n, side_stream)
    assert got["all_equal"][2] == 1 and (got["all_equal"][0][1:] == -1).all() and np.isnan(got["all_equal"][1][1:]).all()
    assert got["ties_across_block_borders"][0][1] == 255 and got["no_candidate"][2] == 0


def test_more_partials_than_a_wavefront_and_a_ragged_tail(lib, rule):
    """T = 16 643, K = 23: 66 workgroups of the update pass; a duplicate of the farthest frame in the ragged tail; default stream"""
    kp = sc.series(sc.T_PARTIALS, sc.K_PARTIALS, 31)
    kp[sc.T_PARTIALS - 2] = kp[9000] = 2.5 * kp[9000]
    cand = np.ones(sc.T_PARTIALS, np.uint8)
    cand[:300] = 0
    cand[-1] = 0
    sel, _, n_sel = _check(lib, rule, "partials", kp, cand, 30, torch.cuda.current_stream())
    assert n_sel == 30 and sel[0] == 300 and 9000 in sel and sc.T_PARTIALS - 2 not in sel


def test_the_capped_grid_strides(lib, rule):
    """1024 x 256 + 5 frames, K = 3: the last five frames are a second trip of the first workgroup; one of them is the farthest"""
    kp = sc.series(sc.T_STRIDED, sc.K_STRIDED, 32)
    kp[sc.T_STRIDED - 3] *= 4.0
    sel, _, n_sel = _check(lib, rule, "strided grid", kp, None, 30, torch.cuda.current_stream())
    assert n_sel == 30 and sel[1] == sc.T_STRIDED - 3


def test_bad_arguments_are_refused_before_any_launch(lib):
    kp = sc.series(100, 3, 33)
    b = _Buffers(lib, kp, np.ones(100, np.uint8), 10)
    torch.cuda.synchronize()
    for over, code in ((dict(T=0), hs.STAC_ERR_INVALID), (dict(K=1), hs.STAC_ERR_INVALID), (dict(K=65), hs.STAC_ERR_CAPACITY), (dict(n=0), hs.STAC_ERR_INVALID),
                       (dict(n=101), hs.STAC_ERR_INVALID), (dict(kp=None), hs.STAC_ERR_INVALID), (dict(sel=None), hs.STAC_ERR_INVALID),
                       (dict(nbytes=b.nbytes - 1), hs.STAC_ERR_INVALID), (dict(work=b.work[4:]), hs.STAC_ERR_INVALID),
                       (dict(radius2=b.sel), hs.STAC_ERR_INVALID), (dict(cand=b.kp), hs.STAC_ERR_INVALID), (dict(n_selected=b.work), hs.STAC_ERR_INVALID)):
        rc = b.call(lib, **over)
        assert rc == code and lib.stac_select_last_error_code() == code and lib.stac_select_last_error().decode(), over
    torch.cuda.synchronize()
    assert b.untouched()
    assert b.call(lib) == 0 and lib.stac_select_last_error_code() == 0 and lib.stac_select_last_error() == b""
    torch.cuda.synchronize()


def test_wrapper(rule):
    from stac_mjx_amd import select

    kp = sc.series(300, 23, 34)
    kp[7] = np.nan
    cand = np.ones(300, bool)
    cand[:3] = False
    want = rule(kp, cand, 20)
    for c in (cand, torch.as_tensor(cand).cuda(), cand.astype(np.int32)):
        sel, r2, n_sel = select.select_diverse(torch.as_tensor(kp).cuda(), 20, c)
        assert sel.is_cuda and sel.dtype == torch.int64 and r2.dtype == torch.float32 and n_sel == want[2]
        np.testing.assert_array_equal(sel.cpu().numpy(), want[0])
        np.testing.assert_array_equal(r2.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    sel, _, n_sel = select.select_diverse(torch.as_tensor(kp).cuda().double(), 5)  # (made float32 first)
    assert sel.cpu().numpy().tolist() == rule(kp, None, 5)[0].tolist()
    for bad in (lambda: select.select_diverse(torch.zeros(10, 3).cuda(), 2), lambda: select.select_diverse(torch.zeros(10, 9).cuda(), 11),
                lambda: select.select_diverse(torch.zeros(10, 9).cuda(), 0), lambda: select.select_diverse(torch.zeros(10, 8).cuda(), 2),
                lambda: select.select_diverse(torch.zeros(10, 9).cuda(), 2, np.ones(9)), lambda: select.select_diverse(torch.zeros(0, 9).cuda(), 1)):
        with pytest.raises(ValueError):
            bad()


# ---- run_stac end to end --------------------------------------------------------------------------------------------------------
def _cfg(rodent_cfg, **stac_over):
    from stac_mjx_amd.config import validate_config

    stac = dict(fit_offsets_path="fit.h5", ik_only_path="ik.h5", data_path="d.mat", continuous=False, n_fit_frames=30,
                skip_fit_offsets=False, skip_ik_only=True, infer_qvels=False, n_frames_per_clip=250,
                mujoco=dict(solver="newton", iterations=1, ls_iterations=4))
    stac.update(stac_over)
    cfg = validate_config({"model": dict(rodent_cfg), "stac": stac})
    cfg.model.N_ITER_Q = 30
    cfg.model.N_ITERS = 1
    return cfg


def _datasets(path):
    from stac_mjx_amd import io

    if path.suffix == ".npz":
        with np.load(path) as f:
            return {k: np.asarray(f[k]) for k in f.files}
    with io.h5py.File(path, "r") as f:
        return {k: np.asarray(f[k][()]) for k in f.keys()}


def test_run_stac_fit_frames(tmp_path, rodent_setup, rodent_cfg, rodent_mocap, rule, capsys):
    from stac_mjx_amd import prep
    from stac_mjx_amd.io import load_stac_data
    from stac_mjx_amd.main import frames_path, run_stac

    rest, _ = sc.resting(np.asarray(rodent_mocap, dtype=np.float32))
    names = rodent_setup.kp_names
    plain_sel, plain_r2, _ = rule(rest, None, 30)

    def run(tag, kp, **over):
        (tmp_path / tag).mkdir()
        fit, ik = run_stac(_cfg(rodent_cfg, **over), np.array(kp), names, base_path=tmp_path / tag, setup=rodent_setup)
        assert ik is None
        return fit

    # the plain recording: the sidecar's indices are the CPU rule's, the rows of the fit file are those frames of the series
    capsys.readouterr()
    fit = run("diverse", rest, fit_frames="diverse")
    log = capsys.readouterr().out
    side = json.loads(frames_path(fit).read_text())
    assert side["mode"] == "diverse" and side["indices"] == sorted(plain_sel.tolist()) and side["order"] == plain_sel.tolist()
    assert side["radius2"][0] is None
    np.testing.assert_array_equal(np.array(side["radius2"][1:], np.float32).view(np.uint32), plain_r2[1:].view(np.uint32))
    data = load_stac_data(fit)[1]
    np.testing.assert_array_equal(data.kp_data.view(np.uint32), rest[side["indices"]].view(np.uint32))
    assert data.qpos.shape[0] == 30 and np.isfinite(data.qpos).all() and data.kp_gap.size == 0
    assert "select_frames (diverse): 30 of 1000 frames, covering radius" in log and "picks per tenth of the recording:" in log
    assert int(np.count_nonzero(np.array(side["indices"]) >= 880)) >= 24

    # with a hole in a frame that the plain run picks and fill_missing on: the frame is filled, carries a mark and is passed over
    holed = rest.copy()
    hole = int(plain_sel[2])
    holed[hole, 15:18] = np.nan
    filled, gap = prep.fill_missing(torch.as_tensor(holed).cuda(), "linear")
    filled, gap = filled.cpu().numpy(), gap.cpu().numpy()
    cand = (gap == 0).all(axis=1)
    assert not cand[hole] and cand.sum() == 999
    want_sel, _, want_n = rule(filled, cand, 30)
    assert want_n == 30 and hole not in want_sel
    fit = run("holed", holed, fit_frames="diverse", fill_missing="linear")
    side = json.loads(frames_path(fit).read_text())
    assert side["order"] == want_sel.tolist() and side["indices"] == sorted(want_sel.tolist())
    data = load_stac_data(fit)[1]
    np.testing.assert_array_equal(data.kp_data.view(np.uint32), filled[side["indices"]].view(np.uint32))
    assert data.kp_gap.shape == (30, 23) and not data.kp_gap.any()  # the marks of the fit file are those of the selected rows

    # strided: the host's choice, same files
    fit = run("strided", rest, fit_frames="strided")
    side = json.loads(frames_path(fit).read_text())
    assert side["mode"] == "strided" and side["indices"] == side["order"] == [(i * 1000) // 30 for i in range(30)] and side["radius2"] == []
    np.testing.assert_array_equal(load_stac_data(fit)[1].kp_data.view(np.uint32), rest[side["indices"]].view(np.uint32))

    # first: dataset for dataset the bytes of a run without the key (the config text aside, which names the key), and no sidecar
    first, absent = run("first", rest, fit_frames="first"), run("absent", rest)
    assert not frames_path(first).exists() and not frames_path(absent).exists()
    da, do = _datasets(absent), _datasets(first)
    assert set(da) == set(do)
    for name in da:
        if name != "config":
            assert da[name].dtype == do[name].dtype and da[name].tobytes() == do[name].tobytes(), name
    key = re.compile(r"(?m)^\W*fit_frames\W")  # (a key of its own: n_fit_frames is in both)
    assert not key.search(da["config"].tobytes().decode()) and key.search(do["config"].tobytes().decode())
    np.testing.assert_array_equal(_datasets(absent)["kp_data"].view(np.uint32), rest[:30].view(np.uint32))

    # a selection that cannot be had names both numbers
    with pytest.raises(ValueError, match="n_fit_frames = 200, but the selection stopped after 160 frames"):
        run("short", rest, fit_frames="diverse", n_fit_frames=200)
    with pytest.raises(ValueError, match="n_fit_frames = 1001 exceeds the 1000 frames"):
        run("long", rest, fit_frames="diverse", n_fit_frames=1001)


def test_stac_method_on_its_own(rodent_setup, rodent_cfg, rodent_mocap, rule):
    from stac_mjx_amd.stac import Stac

    rest, _ = sc.resting(np.asarray(rodent_mocap, dtype=np.float32))
    stac = Stac(None, _cfg(rodent_cfg), rodent_setup.kp_names, setup=rodent_setup, verbose=False)
    exclude = np.zeros(1000, bool)
    exclude[:5] = True
    want = rule(rest, ~exclude, 30)
    rows, info = stac.select_frames(rest, 30, "diverse", exclude=exclude)
    assert rows.dtype == np.int64 and rows.tolist() == sorted(want[0].tolist()) and info["order"].tolist() == want[0].tolist()
    assert info["n_selected"] == 30 and info["mode"] == "diverse"
    np.testing.assert_array_equal(info["radius2"].view(np.uint32), want[1].view(np.uint32))
    rows, info = stac.select_frames(rest, 200, "diverse")  # stops early: the caller sees how many there are
    assert info["n_selected"] == 160 == rows.size and info["radius2"].size == 160
