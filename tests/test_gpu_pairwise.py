"""reject_pairwise on the GPU (stac.reject_pairwise): the kernels of csrc/stac_pairwise.hip against the numpy reference of
tests/pairwise_cases.py, tolerance 0, and ``run_stac`` end to end with the option.  Cases: tests/pairwise_cases.py."""

import ctypes as C

import numpy as np
import pytest
import torch

import host_scaffold as hs
import outlier_cases as oc
import pairwise_cases as pc
import prep_cases as prc

pytestmark = pytest.mark.gpu

PATTERN, FLAG_PATTERN, N_PATTERN, STAT_PATTERN, WORK_PATTERN, GUARD = -12345.0, 0xEE, -7, -7.5, 0x5A, 64
STAC_ERR_INVALID, STAC_ERR_CAPACITY = -1, -3


def _lib():
    return hs.loaded_library()


class _Buffers:
    """Inputs, pre-filled outputs with ``GUARD`` elements around each, and a pre-filled workspace, on the device"""

    def __init__(self, lib, kp_np, offset=0):
        self.T, self.K = kp_np.shape[0], kp_np.shape[1] // 3
        self.P = self.K * (self.K - 1) // 2
        n = kp_np.size
        self.src = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
        self.kp = self.src[offset:offset + n]  # (offset 1: aligned to 4 bytes only)
        self.kp.copy_(torch.as_tensor(np.array(kp_np.reshape(-1))).cuda())
        self.nbytes = lib.stac_prep_pairwise_workspace(self.T, self.K)
        assert self.nbytes >= 8, lib.stac_last_error().decode()
        self.fill()

    def fill(self):
        """Every output and the workspace anew, ``GUARD`` elements in front of and behind each, all holding a pattern"""
        T, K, P = self.T, self.K, self.P
        self.whole = {}
        for name, n, dtype, pattern in (("out", T * 3 * K, torch.float32, PATTERN), ("flag", T * K, torch.uint8, FLAG_PATTERN),
                                        ("pair_n", P, torch.int64, N_PATTERN), ("pair_med", P, torch.float64, STAT_PATTERN),
                                        ("pair_mad", P, torch.float64, STAT_PATTERN), ("work", (self.nbytes + 7) // 8 * 8, torch.uint8, WORK_PATTERN)):
            whole = torch.full((GUARD + n + GUARD,), pattern, dtype=dtype, device="cuda")
            self.whole[name] = (whole, n, pattern)
            setattr(self, name, whole[GUARD:GUARD + n] if n else whole[GUARD:GUARD + 1])  # (P = 0: room for one element, a guard word)
        assert self.work.data_ptr() % 8 == 0 and self.pair_n.data_ptr() % 8 == 0

    def call(self, lib, stream=None, **over):
        """``over``: thr, min_dev, votes, and whatever differs from the buffers of this object"""
        a = dict(kp=self.kp, T=self.T, K=self.K, out=self.out, flag=self.flag, pair_n=self.pair_n,
                 pair_med=self.pair_med, pair_mad=self.pair_mad, work=self.work, nbytes=self.nbytes)
        a.update(over)
        addr = lambda v: C.c_void_p(v.data_ptr() if isinstance(v, torch.Tensor) else v) if v is not None else None  # noqa: E731
        return lib.stac_prep_pairwise(addr(a["kp"]), a["T"], a["K"], a["thr"], a["min_dev"], a["votes"], addr(a["out"]), addr(a["flag"]),
                                      addr(a["pair_n"]), addr(a["pair_med"]), addr(a["pair_mad"]), addr(a["work"]), a["nbytes"],
                                      C.c_void_p(stream) if stream else None)

    def results(self):
        """-> (the five outputs as numpy arrays, without their guards); asserts that every guard word holds its pattern"""
        T, K, P = self.T, self.K, self.P
        got = []
        for name, shape in (("out", (T, 3 * K)), ("flag", (T, K)), ("pair_n", (P,)), ("pair_med", (P,)), ("pair_mad", (P,)), ("work", None)):
            whole, n, pattern = self.whole[name]
            assert bool((whole[:GUARD] == pattern).all()) and bool((whole[GUARD + n:] == pattern).all()), f"guard words around {name}"
            if shape is not None:  # (the workspace stays on the device: 124 MB at K = 64)
                got.append(whole[GUARD:GUARD + n].cpu().numpy().reshape(shape))
        return got

    def untouched(self):
        return all(bool((whole == pattern).all()) for whole, _, pattern in self.whole.values())


@pytest.mark.parametrize("K", pc.KS)
def test_pairwise_equals_reference(K):
    """Every pattern that fits at every T of the grid for this K: outputs and workspace pre-filled, tolerance 0 on the bits of the
    five outputs, and a second call (on the workspace the first one left) equals the first bit for bit."""
    lib = _lib()
    cases = pc.cases(ks=(K,))
    assert {T for _, T, _ in cases} == set(pc.TS)
    rejected = 0
    for name, T, _ in cases:
        kp, thr, min_dev, votes, want = pc.reference(name, T, K)
        b = _Buffers(lib, kp)
        assert b.call(lib, thr=thr, min_dev=min_dev, votes=votes) == 0, lib.stac_last_error().decode()
        first = b.results()
        pc.check(first, kp, want, label=f"{name} T={T} K={K}")
        np.testing.assert_array_equal(b.kp.cpu().numpy().view(np.uint32), kp.reshape(-1).view(np.uint32))  # the source is never written
        work = b.work
        b.fill()
        b.work.copy_(work)  # (what the first call left, not the pattern)
        assert b.call(lib, thr=thr, min_dev=min_dev, votes=votes) == 0, lib.stac_last_error().decode()
        for x, y in zip(first, b.results()):
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=f"{name} T={T} K={K} second call")
        rejected += int(want[1].sum())
    assert K < 3 or rejected > 50  # (the cases do reject)


def test_long_series_beyond_one_sweep_of_the_grids():
    """T = 70 000, K = 4: more tiles than workgroups in the first and in the decision pass, and several segments per pair in the
    counting passes.  Noise with displaced and missing keypoints; through the wrapper as well."""
    from stac_mjx_amd import prep

    T, K = 70_000, 4
    assert T > 64 * 1024 and T > 4096 * 16 and T > 8 * 8192
    rng = np.random.default_rng(70_000)
    x = pc.skeleton(T, K, rng)
    pc._noise(x, rng)
    x[T - 1, 2, 0] += np.float32(pc.BIG)  # the last frame of the last tile
    x[0, 1, 1] -= np.float32(pc.BIG)
    kp = np.ascontiguousarray(x.reshape(T, 3 * K))
    want = pc.reference_pairwise_all_pairs(kp, pc.THR, pc.MIN_DEV, 2)
    assert 0.005 < want[1].mean() < 0.2 and want[1][T - 1, 2] == 1 and want[1][0, 1] == 1
    lib = _lib()
    b = _Buffers(lib, kp)
    assert b.call(lib, thr=pc.THR, min_dev=pc.MIN_DEV, votes=2) == 0, lib.stac_last_error().decode()
    pc.check(b.results(), kp, want, label="long")
    out, flag, stats = prep.reject_pairwise(torch.as_tensor(kp).cuda(), n_sigma=6.0, min_dev=pc.MIN_DEV, votes=2)
    got = [out.cpu().numpy(), flag.cpu().numpy(), stats["pair_n"].cpu().numpy(), stats["pair_med"].cpu().numpy(), stats["pair_mad"].cpu().numpy()]
    pc.check(got, kp, want, label="long wrapper")


def test_raw_entry_point_guards_alignment_stream_and_refusals():
    lib = _lib()
    name, T, K = "noise_votes_2", 129, 23
    kp, thr, min_dev, votes, want = pc.reference(name, T, K)
    b = _Buffers(lib, kp, offset=1)
    assert b.kp.data_ptr() % 4 == 0 and b.kp.data_ptr() % 16 != 0  # inputs aligned to 4 bytes only
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rc = b.call(lib, stream=stream.cuda_stream, thr=thr, min_dev=min_dev, votes=votes)
    assert rc == 0, lib.stac_last_error().decode()
    stream.synchronize()
    pc.check(b.results(), kp, want, label="raw, side stream")  # (and the guard words around every output)
    # every refusal happens before anything is launched: outputs and workspace keep what they hold
    b.fill()
    torch.cuda.synchronize()
    big = torch.zeros(8 * 3 * 65, dtype=torch.float32, device="cuda")
    assert b.call(lib, thr=thr, min_dev=min_dev, votes=votes, T=8, K=65, kp=big) == STAC_ERR_CAPACITY and lib.stac_last_error_code() == STAC_ERR_CAPACITY
    assert lib.stac_prep_pairwise_workspace(8, 65) == STAC_ERR_CAPACITY
    bad = [dict(kp=None), dict(out=None), dict(flag=None), dict(pair_n=None), dict(pair_med=None), dict(pair_mad=None), dict(work=None),
           dict(T=0), dict(T=-1), dict(K=0), dict(K=-2), dict(thr=-1.0), dict(thr=float("nan")), dict(thr=float("inf")),
           dict(min_dev=-1e-12), dict(min_dev=float("nan")), dict(votes=0), dict(votes=-1), dict(nbytes=b.nbytes - 1), dict(nbytes=0),
           dict(kp=b.kp.data_ptr() + 2), dict(out=b.out.data_ptr() + 1), dict(pair_med=b.pair_med.data_ptr() + 4),
           dict(work=b.work.data_ptr() + 4), dict(out=b.kp), dict(out=b.src), dict(flag=b.out), dict(pair_mad=b.pair_med),
           dict(work=b.out), dict(pair_n=b.work)]  # nulls, sizes, parameters, alignment, in place and overlaps
    for over in bad:
        assert b.call(lib, **{**dict(thr=thr, min_dev=min_dev, votes=votes), **over}) == STAC_ERR_INVALID and lib.stac_last_error_code() == STAC_ERR_INVALID, list(over)
    torch.cuda.synchronize()
    assert b.untouched()


def test_wrapper_input_handling_and_empty_series():
    from stac_mjx_amd import prep

    name, T, K = "noise_votes_1", 129, 23
    kp_np, thr, min_dev, votes, want = pc.reference(name, T, K)
    wide = torch.as_tensor(np.concatenate([kp_np, kp_np], axis=1)).cuda()[:, :3 * K]  # not contiguous
    assert not wide.is_contiguous()
    before = wide.clone()
    out, flag, stats = prep.reject_pairwise(wide, n_sigma=thr / pc.MAD_TO_SIGMA, min_dev=min_dev, votes=votes)
    assert thr / pc.MAD_TO_SIGMA * pc.MAD_TO_SIGMA == thr
    assert out.is_cuda and out.dtype == torch.float32 and flag.dtype == torch.uint8 and tuple(flag.shape) == (T, K)
    got = [out.cpu().numpy(), flag.cpu().numpy(), stats["pair_n"].cpu().numpy(), stats["pair_med"].cpu().numpy(), stats["pair_mad"].cpu().numpy()]
    pc.check(got, kp_np, want, label="wrapper")
    assert torch.equal(wide.contiguous().view(torch.int32), before.contiguous().view(torch.int32))  # the caller's tensor is not written
    one = torch.as_tensor(np.array(pc.reference("missing", 65, 1)[0])).cuda()  # K = 1: no pairs, everything passes
    out, flag, stats = prep.reject_pairwise(one)
    assert torch.equal(out.view(torch.int32), one.view(torch.int32)) and int(flag.sum()) == 0 and stats["pair_n"].numel() == 0
    out, flag, stats = prep.reject_pairwise(torch.zeros(0, 6, device="cuda"))  # T == 0: empty tensors without a call
    assert tuple(out.shape) == (0, 6) and tuple(flag.shape) == (0, 2) and flag.dtype == torch.uint8 and stats["pair_n"].numel() == 1
    with pytest.raises(ValueError):
        prep.reject_pairwise(torch.zeros(4, 7, device="cuda"))  # 7 columns are not keypoints of three
    with pytest.raises(ValueError):
        prep.reject_pairwise(torch.zeros(4, 6, device="cuda"), votes=0)
    with pytest.raises(RuntimeError, match="65"):
        prep.reject_pairwise(torch.zeros(4, 3 * 65, device="cuda"))  # above the capacity: refused, nothing launched


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


ROWS = 96      # frames of the short series
SWAP = (4, 44)  # the injected swap: frames 4 .. 43, 40 in a row
SPIKES = ((60, 3), (75, 17))  # (frame, keypoint): single-frame spikes of 8 cm in one coordinate, Hampel's share


@pytest.fixture(scope="module")
def swapped(rodent_mocap, rodent_setup):
    """rodent_mocap[200:296] with KneeL / KneeR swapped for 40 frames and two single-frame spikes -> (kp, the pairwise reference's
    out and flag, the Hampel reference's flag on that out, the fill's reference)"""
    names = list(rodent_setup.kp_names)
    l, r = names.index("KneeL"), names.index("KneeR")
    kp = np.array(rodent_mocap[200:200 + ROWS], dtype=np.float32)
    assert np.isfinite(kp).all() and kp.shape == (ROWS, 69)
    x = kp.reshape(ROWS, 23, 3)
    x[SWAP[0]:SWAP[1], [l, r]] = x[SWAP[0]:SWAP[1], [r, l]]
    for i, (t, k) in enumerate(SPIKES):
        x[t, k, i % 3] += np.float32(0.08)
    out, flag = pc.reference_pairwise(kp, pc.THR, pc.MIN_DEV, 2)[:2]
    assert flag[SWAP[0]:SWAP[1], [l, r]].mean() > 0.5  # (a condition on the inputs: the swap is one to the reference)
    out2, hampel = oc.reference_reject(out, 5, oc.THR, 0.001)
    assert hampel.sum() > 0 and not (hampel & flag).any()
    filled, gap = prc.reference_fill(out2, "linear")
    for a in (kp, out, flag, hampel, filled, gap):
        a.setflags(write=False)
    return kp, out, flag, hampel, filled, gap


def _load_both(paths):
    from stac_mjx_amd.io import load_stac_data

    return [load_stac_data(p)[1] for p in paths]


def test_run_stac_reject_pairwise(tmp_path, rodent_setup, rodent_cfg, swapped, capsys):
    from stac_mjx_amd.main import run_stac

    kp, ref_out, ref_flag, ref_hampel, ref_filled, ref_gap = swapped
    names = rodent_setup.kp_names

    def run(tag, **over):
        (tmp_path / tag).mkdir()
        paths = run_stac(_cfg(rodent_cfg, **over), np.array(kp), names, base_path=tmp_path / tag, setup=rodent_setup)
        return paths, _load_both(paths)

    capsys.readouterr()
    _, both = run("both", fill_missing="linear", reject_pairwise="mad", reject_outliers="hampel")
    log = capsys.readouterr().out
    _, alone = run("alone", fill_missing="linear", reject_pairwise="mad")
    absent_paths, absent = run("absent", fill_missing="linear")
    off_paths, _ = run("off", fill_missing="linear", reject_pairwise="off", pairwise_nsigma=3.0, pairwise_min_dev=0.0, pairwise_votes=1)

    # one log line per keypoint that had rejections (count and share), one about the fit frames
    lines = [ln for ln in log.splitlines() if ln.startswith("reject_pairwise (mad")]
    counts = ref_flag.sum(axis=0)
    assert len(lines) == np.count_nonzero(counts), log
    for k in np.flatnonzero(counts):
        (ln,) = [ln for ln in lines if f" {names[k]}: " in ln]
        assert f"{int(counts[k])} of {ROWS} frames rejected" in ln and "%" in ln, ln
    assert "of the 12 fit frames were rejected by their pairwise distances" in log and "of the 12 fit frames were rejected as outliers" in log

    for d, rows in zip(both, (12, ROWS)):
        assert d.kp_rejected_pairwise.dtype == np.uint8 and d.kp_rejected.dtype == np.uint8
        np.testing.assert_array_equal(d.kp_rejected_pairwise, ref_flag[:rows])          # the reference's flags, in both files
        np.testing.assert_array_equal(d.kp_rejected, (ref_flag | ref_hampel)[:rows])    # the OR with Hampel's
        np.testing.assert_array_equal(d.kp_gap, ref_gap[:rows])
        assert (d.kp_gap[d.kp_rejected == 1] > 0).all()                                 # the fill saw them as missing
        np.testing.assert_array_equal(d.kp_data.view(np.uint32), ref_filled[:rows].view(np.uint32))  # bit for bit
        assert np.isfinite(d.qpos).all() and d.qpos.shape[0] == rows
    for d, rows in zip(alone, (12, ROWS)):  # without Hampel: kp_rejected is this detector's share
        np.testing.assert_array_equal(d.kp_rejected_pairwise, ref_flag[:rows])
        np.testing.assert_array_equal(d.kp_rejected, ref_flag[:rows])

    # with the key absent: no new dataset, and the files are byte for byte those of a run whose config names the feature's keys
    # but leaves it off, except for the config text they carry (compared dataset by dataset below)
    for a in absent:
        assert a.kp_rejected_pairwise.size == 0 and a.kp_rejected.size == 0
    for pa, po in zip(absent_paths, off_paths):
        da, do = _datasets(pa), _datasets(po)
        assert set(da) == set(do) and "kp_rejected_pairwise" not in da and "kp_rejected" not in da
        for name in da:
            if name != "config":
                assert da[name].dtype == do[name].dtype and da[name].tobytes() == do[name].tobytes(), name
        assert "pairwise" not in da["config"].tobytes().decode() and "reject_pairwise: 'off'" in do["config"].tobytes().decode().replace('"', "'")


def _datasets(path):
    from stac_mjx_amd import io

    if path.suffix == ".npz":
        with np.load(path) as f:
            return {k: np.asarray(f[k]) for k in f.files}
    with io.h5py.File(path, "r") as f:
        return {k: np.asarray(f[k][()]) for k in f.keys()}


def test_stac_method_on_its_own(rodent_setup, rodent_cfg, swapped):
    from stac_mjx_amd.stac import Stac

    kp, ref_out, ref_flag, _, _, _ = swapped
    stac = Stac(None, _cfg(rodent_cfg), rodent_setup.kp_names, setup=rodent_setup, verbose=False)
    out, flag = stac.reject_pairwise(kp)  # numpy in, numpy out; the defaults are the config's
    assert out.dtype == np.float32 and flag.dtype == np.uint8
    np.testing.assert_array_equal(flag, ref_flag)
    np.testing.assert_array_equal(out.view(np.uint32), ref_out.view(np.uint32))
    with pytest.raises(ValueError):
        stac.reject_pairwise(kp[:, :66])
    with pytest.raises(ValueError):
        stac.reject_pairwise(kp, votes=0)
