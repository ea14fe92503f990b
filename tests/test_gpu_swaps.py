"""repair_swaps on the GPU (stac.repair_swaps): pairwise_swap_kernel of csrc/stac_pairwise.hip against the numpy reference of
tests/swaps_cases.py, tolerance 0, and ``run_stac`` end to end with the option.  Cases: tests/swaps_cases.py."""

import ctypes as C

import numpy as np
import pytest
import torch

import host_scaffold as hs
import swaps_cases as sc

pytestmark = pytest.mark.gpu

PATTERN, FLAG_PATTERN, N_PATTERN, STAT_PATTERN, WORK_PATTERN, GUARD = -12345.0, 0xEE, -7, -7.5, 0xFF, 64
STAC_ERR_INVALID, STAC_ERR_CAPACITY = -1, -3


def _lib():
    return hs.loaded_library()


class _Buffers:
    """Inputs, pre-filled outputs with ``GUARD`` elements around each, and a workspace of 0xFF bytes, on the device"""

    def __init__(self, lib, kp_np, cand, offset=0, flag_cols=None):
        """``flag_cols``: the columns of ``flag`` where they are not the candidates (``stac_prep_pairwise``: one per keypoint)"""
        self.T, self.K, self.cand = kp_np.shape[0], kp_np.shape[1] // 3, list(cand)
        self.S, self.P = len(self.cand) if flag_cols is None else flag_cols, self.K * (self.K - 1) // 2
        n = kp_np.size
        self.src = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
        self.kp = self.src[offset:offset + n]  # (offset 1: aligned to 4 bytes only)
        self.kp.copy_(torch.as_tensor(np.array(kp_np.reshape(-1))).cuda())
        self.nbytes = lib.stac_prep_swaps_workspace(self.T, self.K)
        assert self.nbytes >= 8, lib.stac_last_error().decode()
        self.fill()

    def fill(self):
        """Every output and the workspace anew, ``GUARD`` elements in front of and behind each, all holding a pattern"""
        T, K, P, S = self.T, self.K, self.P, self.S
        self.whole = {}
        for name, n, dtype, pattern in (("out", T * 3 * K, torch.float32, PATTERN), ("flag", T * S, torch.uint8, FLAG_PATTERN),
                                        ("pair_n", P, torch.int64, N_PATTERN), ("pair_med", P, torch.float64, STAT_PATTERN),
                                        ("pair_mad", P, torch.float64, STAT_PATTERN), ("work", (self.nbytes + 7) // 8 * 8, torch.uint8, WORK_PATTERN)):
            room = max(n, T) if name == "flag" else n  # (S = 0: room for T bytes, which stay what they are)
            whole = torch.full((GUARD + room + GUARD,), pattern, dtype=dtype, device="cuda")
            self.whole[name] = (whole, n, pattern)
            setattr(self, name, whole[GUARD:GUARD + room] if room else whole[GUARD:GUARD + 1])  # (P = 0: room for one element, a guard word)
        assert self.work.data_ptr() % 8 == 0 and self.pair_n.data_ptr() % 8 == 0

    def call(self, lib, stream=None, entry="stac_prep_swaps", **over):
        """``over``: thr, min_dev, min_bad (votes for ``stac_prep_pairwise``), and whatever differs from the buffers of this object"""
        a = dict(kp=self.kp, T=self.T, K=self.K, cand=self.cand, out=self.out, flag=self.flag, pair_n=self.pair_n,
                 pair_med=self.pair_med, pair_mad=self.pair_mad, work=self.work, nbytes=self.nbytes)
        a.update(over)
        addr = lambda v: C.c_void_p(v.data_ptr() if isinstance(v, torch.Tensor) else v) if v is not None else None  # noqa: E731
        tail = (addr(a["out"]), addr(a["flag"]), addr(a["pair_n"]), addr(a["pair_med"]), addr(a["pair_mad"]), addr(a["work"]), a["nbytes"],
                C.c_void_p(stream) if stream else None)
        if entry == "stac_prep_pairwise":
            return lib.stac_prep_pairwise(addr(a["kp"]), a["T"], a["K"], a["thr"], a["min_dev"], a["votes"], *tail)
        cand = a["cand"]
        n_cand = a.get("n_cand", len(cand) if cand is not None else 0)
        table = (C.c_int32 * max(2 * len(cand), 1))(*[v for ab in cand for v in ab]) if cand is not None else None  # host memory
        return lib.stac_prep_swaps(addr(a["kp"]), a["T"], a["K"], table, n_cand, a["thr"], a["min_dev"], a["min_bad"], *tail)

    def results(self):
        """-> (the five outputs as numpy arrays, without their guards); asserts that every guard word holds its pattern"""
        T, K, P, S = self.T, self.K, self.P, self.S
        got = []
        for name, shape in (("out", (T, 3 * K)), ("flag", (T, S)), ("pair_n", (P,)), ("pair_med", (P,)), ("pair_mad", (P,)), ("work", None)):
            whole, n, pattern = self.whole[name]
            assert bool((whole[:GUARD] == pattern).all()) and bool((whole[GUARD + n:] == pattern).all()), f"guard words around {name}"
            if shape is not None:  # (the workspace stays on the device: 124 MB at K = 64)
                got.append(whole[GUARD:GUARD + n].cpu().numpy().reshape(shape))
        return got

    def untouched(self):
        return all(bool((whole == pattern).all()) for whole, _, pattern in self.whole.values())


@pytest.fixture(scope="module")
def side_stream():
    return torch.cuda.Stream()


@pytest.mark.parametrize("T", sc.TS)
@pytest.mark.parametrize("K", sc.KS)
def test_swaps_equal_reference(K, T, side_stream):
    """Every case of this shape, on a stream that is not the default one: outputs pre-filled and the workspace poisoned to 0xFF,
    tolerance 0 on the bits of the five outputs; the statistics are those of ``stac_prep_pairwise`` on the same input, bit for bit;
    and a second call (on the workspace the first one left) equals the first bit for bit."""
    lib = _lib()
    cases = sc.cases(ks=(K,), ts=(T,))
    assert len(cases) >= 9
    for name, _, _ in cases:
        kp, cand, thr, min_dev, min_bad, want = sc.reference(name, T, K)
        b = _Buffers(lib, kp, cand)
        torch.cuda.synchronize()
        par = dict(thr=thr, min_dev=min_dev, min_bad=min_bad)
        with torch.cuda.stream(side_stream):
            rc = b.call(lib, stream=side_stream.cuda_stream, **par)
        assert rc == 0, lib.stac_last_error().decode()
        side_stream.synchronize()
        first = b.results()
        sc.check(first, kp, cand, want, label=f"{name} T={T} K={K}")
        np.testing.assert_array_equal(b.kp.cpu().numpy().view(np.uint32), kp.reshape(-1).view(np.uint32))  # the source is never written
        work = b.work
        b.fill()
        b.work.copy_(work)  # (what the first call left, not the pattern)
        torch.cuda.synchronize()
        with torch.cuda.stream(side_stream):
            rc = b.call(lib, stream=side_stream.cuda_stream, **par)
        assert rc == 0, lib.stac_last_error().decode()
        side_stream.synchronize()
        for x, y in zip(first, b.results()):
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=f"{name} T={T} K={K} second call")
        # the statistics of stac_prep_pairwise on the same input (flag there is [T][K])
        p = _Buffers(lib, kp, [], flag_cols=K)
        assert p.call(lib, entry="stac_prep_pairwise", thr=thr, min_dev=min_dev, votes=2) == 0, lib.stac_last_error().decode()
        torch.cuda.synchronize()
        for x, y in zip(first[2:], p.results()[2:]):
            np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64), err_msg=f"{name} T={T} K={K} statistics of stac_prep_pairwise")


def test_long_series_beyond_one_sweep_of_the_grid():
    """T = 270 000, K = 5: more tiles than the 4096 workgroups of the decision launch.  Swaps of two candidates, displaced and
    missing keypoints, the last frame of the last tile swapped; through the wrapper."""
    from stac_mjx_amd import prep

    T, K = 270_000, 5
    assert T > 4096 * 64
    rng = np.random.default_rng(270_000)
    x = sc.pc.skeleton(T, K, rng)
    cand = [(3, 0), (1, 4)]
    hit = rng.random((T, 2)) < 0.05
    hit[T - 1] = (True, False)
    hit[T - 2] = (False, True)
    sc.exchange_frames(x, cand, hit)
    sc.pc._noise(x, rng, missing=0.02)
    kp = np.ascontiguousarray(x.reshape(T, 3 * K))
    want = sc.reference_swaps_all_frames(kp, cand, sc.THR, sc.MIN_DEV, sc.MIN_BAD)
    assert 0.02 < want[1].mean() < 0.1 and want[1][T - 1, 0] == 1 and want[1][T - 2, 1] == 1
    out, flag, stats = prep.repair_swaps(torch.as_tensor(kp).cuda(), cand)
    got = [out.cpu().numpy(), flag.cpu().numpy(), stats["pair_n"].cpu().numpy(), stats["pair_med"].cpu().numpy(), stats["pair_mad"].cpu().numpy()]
    sc.check(got, kp, cand, want, label="long wrapper")


def test_raw_entry_point_alignment_and_refusals():
    lib = _lib()
    name, T, K = "swaps_missing", 129, 23
    kp, cand, thr, min_dev, min_bad, want = sc.reference(name, T, K)
    par = dict(thr=thr, min_dev=min_dev, min_bad=min_bad)
    b = _Buffers(lib, kp, cand, offset=1)
    assert b.kp.data_ptr() % 4 == 0 and b.kp.data_ptr() % 16 != 0  # inputs aligned to 4 bytes only
    assert b.call(lib, **par) == 0, lib.stac_last_error().decode()
    torch.cuda.synchronize()
    sc.check(b.results(), kp, cand, want, label="raw, default stream")  # (and the guard words around every output)
    # every refusal happens before anything is launched: outputs and workspace keep what they hold
    b.fill()
    torch.cuda.synchronize()
    big = torch.zeros(8 * 3 * 65, dtype=torch.float32, device="cuda")
    assert b.call(lib, **par, T=8, K=65, kp=big) == STAC_ERR_CAPACITY and lib.stac_last_error_code() == STAC_ERR_CAPACITY
    assert lib.stac_prep_swaps_workspace(8, 65) == STAC_ERR_CAPACITY
    bad = [dict(kp=None), dict(out=None), dict(flag=None), dict(pair_n=None), dict(pair_med=None), dict(pair_mad=None), dict(work=None),
           dict(cand=None, n_cand=1), dict(T=0), dict(T=-1), dict(K=0), dict(K=-2), dict(n_cand=-1),
           dict(cand=[(0, 23)]), dict(cand=[(-1, 2)]), dict(cand=[(4, 4)]), dict(cand=[(0, 1), (1, 2)]), dict(cand=[(0, 1), (2, 3), (3, 0)]),
           dict(thr=-1.0), dict(thr=float("nan")), dict(thr=float("inf")), dict(min_dev=-1e-12), dict(min_dev=float("nan")),
           dict(min_dev=float("inf")), dict(min_bad=0), dict(min_bad=-1), dict(nbytes=b.nbytes - 1), dict(nbytes=0),
           dict(kp=b.kp.data_ptr() + 2), dict(out=b.out.data_ptr() + 1), dict(pair_med=b.pair_med.data_ptr() + 4),
           dict(work=b.work.data_ptr() + 4), dict(out=b.kp), dict(out=b.src), dict(flag=b.out), dict(pair_mad=b.pair_med),
           dict(work=b.out), dict(pair_n=b.work)]  # nulls, sizes, candidates, parameters, alignment, in place and overlaps
    for over in bad:
        assert b.call(lib, **{**par, **over}) == STAC_ERR_INVALID and lib.stac_last_error_code() == STAC_ERR_INVALID, list(over)
    torch.cuda.synchronize()
    assert b.untouched()


def test_wrapper_input_handling_and_empty_series():
    from stac_mjx_amd import prep

    name, T, K = "swaps", 129, 23
    kp_np, cand, thr, min_dev, min_bad, want = sc.reference(name, T, K)
    wide = torch.as_tensor(np.concatenate([kp_np, kp_np], axis=1)).cuda()[:, :3 * K]  # not contiguous
    assert not wide.is_contiguous()
    before = wide.clone()
    out, flag, stats = prep.repair_swaps(wide, cand, n_sigma=thr / sc.pc.MAD_TO_SIGMA, min_dev=min_dev, min_bad=min_bad)
    assert thr / sc.pc.MAD_TO_SIGMA * sc.pc.MAD_TO_SIGMA == thr
    assert out.is_cuda and out.dtype == torch.float32 and flag.dtype == torch.uint8 and tuple(flag.shape) == (T, len(cand))
    got = [out.cpu().numpy(), flag.cpu().numpy(), stats["pair_n"].cpu().numpy(), stats["pair_med"].cpu().numpy(), stats["pair_mad"].cpu().numpy()]
    sc.check(got, kp_np, cand, want, label="wrapper")
    assert torch.equal(wide.contiguous().view(torch.int32), before.contiguous().view(torch.int32))  # the caller's tensor is not written
    out, flag, stats = prep.repair_swaps(wide, [])  # no candidate: everything passes, the statistics are computed
    assert torch.equal(out.view(torch.int32), before.contiguous().view(torch.int32)) and tuple(flag.shape) == (T, 0)
    np.testing.assert_array_equal(stats["pair_med"].cpu().numpy().view(np.uint64), want[3].view(np.uint64))
    one = torch.as_tensor(np.array(sc.pc.reference("missing", 65, 1)[0])).cuda()  # K = 1: no pairs, no candidate can be
    out, flag, stats = prep.repair_swaps(one, [])
    assert torch.equal(out.view(torch.int32), one.view(torch.int32)) and tuple(flag.shape) == (65, 0) and stats["pair_n"].numel() == 0
    out, flag, stats = prep.repair_swaps(torch.zeros(0, 6, device="cuda"), [(0, 1)])  # T == 0: empty tensors without a call
    assert tuple(out.shape) == (0, 6) and tuple(flag.shape) == (0, 1) and flag.dtype == torch.uint8
    with pytest.raises(ValueError):
        prep.repair_swaps(torch.zeros(4, 7, device="cuda"), [(0, 1)])  # 7 columns are not keypoints of three
    with pytest.raises(ValueError):
        prep.repair_swaps(torch.zeros(4, 6, device="cuda"), [(0, 1)], min_bad=0)
    with pytest.raises(ValueError):
        prep.repair_swaps(torch.zeros(4, 6, device="cuda"), [(0, 2)])
    with pytest.raises(RuntimeError, match="65"):
        prep.repair_swaps(torch.zeros(4, 3 * 65, device="cuda"), [(0, 1)])  # above the capacity: refused, nothing launched


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


ROWS = 96                        # frames of the short series (the run of tests/test_gpu_pairwise.py)
RUNS = ((20, 44), (50, 74))      # the first left / right pair is exchanged in the frames 20 .. 43, the second in 50 .. 73


@pytest.fixture(scope="module")
def swapped(rodent_mocap, rodent_setup):
    """rodent_mocap[200:296] untouched, and with the first two left / right pairs swapped for 24 frames each -> (clean, kp, cand,
    hit [ROWS, S]); on the CPU first: the reference finds no swap in the untouched frames and exactly the injected ones"""
    from stac_mjx_amd.config import lr_pairs

    cand = lr_pairs(list(rodent_setup.kp_names))
    clean = np.array(rodent_mocap[200:200 + ROWS], dtype=np.float32)
    assert np.isfinite(clean).all() and clean.shape == (ROWS, 69) and len(cand) == 9
    assert sc.reference_swaps_all_frames(clean, cand, sc.THR, sc.MIN_DEV, sc.MIN_BAD)[1].sum() == 0
    hit = np.zeros((ROWS, len(cand)), bool)
    for s, (lo, hi) in enumerate(RUNS):
        hit[lo:hi, s] = True
    kp = clean.copy()
    sc.exchange_frames(kp.reshape(ROWS, 23, 3), cand, hit)
    out, flag = sc.reference_swaps_all_frames(kp, cand, sc.THR, sc.MIN_DEV, sc.MIN_BAD)[:2]
    np.testing.assert_array_equal(flag, hit.astype(np.uint8))
    np.testing.assert_array_equal(out.view(np.uint32), clean.view(np.uint32))
    for a in (clean, kp, hit):
        a.setflags(write=False)
    return clean, kp, cand, hit


def _datasets(path):
    from stac_mjx_amd import io

    if path.suffix == ".npz":
        with np.load(path) as f:
            return {k: np.asarray(f[k]) for k in f.files}
    with io.h5py.File(path, "r") as f:
        return {k: np.asarray(f[k][()]) for k in f.keys()}


def test_run_stac_repair_swaps(tmp_path, rodent_setup, rodent_cfg, swapped, capsys):
    from stac_mjx_amd.main import run_stac

    clean, kp, cand, hit = swapped
    names = list(rodent_setup.kp_names)

    def run(tag, series, **over):
        (tmp_path / tag).mkdir()
        return run_stac(_cfg(rodent_cfg, **over), np.array(series), names, base_path=tmp_path / tag, setup=rodent_setup)

    untouched = run("untouched", clean)  # the untouched series, the feature off
    capsys.readouterr()
    repaired = run("repaired", kp, repair_swaps="lr")
    log = capsys.readouterr().out

    marks = np.zeros((ROWS, 23), np.uint8)
    for s, (a, b) in enumerate(cand):
        marks[hit[:, s], a] = marks[hit[:, s], b] = 1
    assert marks.sum() == 96
    for pu, pr, rows in zip(untouched, repaired, (12, ROWS)):
        du, dr = _datasets(pu), _datasets(pr)
        assert set(dr) == set(du) | {"kp_swapped"} and "kp_swapped" not in du
        for name in du:  # kp_data, qpos and every other dataset: those of the untouched run, bit for bit
            if name != "config":
                assert du[name].dtype == dr[name].dtype and du[name].tobytes() == dr[name].tobytes(), name
        np.testing.assert_array_equal(dr["kp_data"].view(np.uint32), clean[:rows].view(np.uint32))
        assert dr["kp_swapped"].dtype == np.uint8
        np.testing.assert_array_equal(dr["kp_swapped"], marks[:rows])  # exactly the swapped (frame, keypoint)s
        assert "repair_swaps" not in du["config"].tobytes().decode() and "repair_swaps: lr" in dr["config"].tobytes().decode()
    # one log line per candidate that had swaps, one about the fit frames (none of the 12 is swapped)
    lines = [ln for ln in log.splitlines() if ln.startswith("repair_swaps (")]
    assert len(lines) == 2, log
    for s in (0, 1):
        a, b = cand[s]
        (ln,) = [ln for ln in lines if f" {names[a]} / {names[b]}: " in ln]
        assert f"24 of {ROWS} frames exchanged" in ln, ln
    assert "repair_swaps: 0 (frame, pair)s of the 12 fit frames were exchanged back" in log


def test_stac_method_on_its_own(rodent_setup, rodent_cfg, swapped):
    from stac_mjx_amd.stac import Stac

    clean, kp, cand, hit = swapped
    names = list(rodent_setup.kp_names)
    stac = Stac(None, _cfg(rodent_cfg), rodent_setup.kp_names, setup=rodent_setup, verbose=False)
    out, flag = stac.repair_swaps(kp)  # numpy in, numpy out; the candidates are the left / right pairs of the names
    assert out.dtype == np.float32 and flag.dtype == np.uint8 and flag.shape == (ROWS, 9)
    np.testing.assert_array_equal(flag, hit.astype(np.uint8))
    np.testing.assert_array_equal(out.view(np.uint32), clean.view(np.uint32))
    out, flag = stac.repair_swaps(kp, [[names[cand[1][1]], names[cand[1][0]]]])  # one pair by name, R first
    np.testing.assert_array_equal(flag[:, 0], hit[:, 1].astype(np.uint8))
    out, flag = stac.repair_swaps(kp, [cand[0]])  # by index
    np.testing.assert_array_equal(flag[:, 0], hit[:, 0].astype(np.uint8))
    with pytest.raises(ValueError):
        stac.repair_swaps(kp[:, :66])
    with pytest.raises(ValueError):
        stac.repair_swaps(kp, min_bad=0)
    with pytest.raises(ValueError):
        stac.repair_swaps(kp, [["KneeL", "Elbow"]])
