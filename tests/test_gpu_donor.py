"""fill_donors on the GPU (stac.fill_donors): donor_fill_kernel of csrc/stac_donor.hip, behind the two scan launches it shares with
fill_missing, against the numpy float64 reference of tests/donor_cases.py, tolerance 0 on ``out`` (as bits), ``gap`` and ``src``, and
``run_stac`` end to end with the option.  Cases: tests/donor_cases.py."""

import ctypes as C

import numpy as np
import pytest
import torch

import host_scaffold as hs
import donor_cases as dc
import pairwise_cases as pw
import prep_cases as pc

pytestmark = pytest.mark.gpu

PATTERN, GAP_PATTERN, SRC_PATTERN, WORK_PATTERN, GUARD = -12345.0, -7, 0xEE, 0xFF, 64
STAC_ERR_INVALID, STAC_ERR_CAPACITY = -1, -3


def _lib():
    return hs.loaded_library()


class _Buffers:
    """Inputs, pre-filled outputs with ``GUARD`` elements around each, and a workspace of 0xFF bytes, on the device"""

    def __init__(self, lib, kp_np, don_np, offset=0):
        self.T, self.K, self.D = kp_np.shape[0], kp_np.shape[1] // 3, don_np.shape[1]
        n = kp_np.size
        self.source = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
        self.kp = self.source[offset:offset + n]  # (offset 1: aligned to 4 bytes only)
        self.kp.copy_(torch.as_tensor(np.array(kp_np.reshape(-1))).cuda())
        self.don = torch.as_tensor(np.array(don_np, dtype=np.int32).reshape(-1)).cuda()
        self.nbytes = lib.stac_prep_donor_workspace(self.T, self.K)
        assert self.nbytes >= 32, lib.stac_last_error().decode()
        self.fill()

    def fill(self):
        """Every output and the workspace anew, ``GUARD`` elements in front of and behind each, all holding a pattern"""
        T, K = self.T, self.K
        self.whole = {}
        for name, n, dtype, pattern in (("out", T * 3 * K, torch.float32, PATTERN), ("gap", T * K, torch.int32, GAP_PATTERN),
                                        ("src", T * K, torch.uint8, SRC_PATTERN), ("work", (self.nbytes + 7) // 8 * 8, torch.uint8, WORK_PATTERN)):
            whole = torch.full((GUARD + n + GUARD,), pattern, dtype=dtype, device="cuda")
            self.whole[name] = (whole, n, pattern)
            setattr(self, name, whole[GUARD:GUARD + n])
        assert self.work.data_ptr() % 8 == 0

    def call(self, lib, stream=None, **over):
        a = dict(kp=self.kp, T=self.T, K=self.K, don=self.don, D=self.D, out=self.out, gap=self.gap, src=self.src, work=self.work,
                 nbytes=self.nbytes)
        a.update(over)
        addr = lambda v: C.c_void_p(v.data_ptr() if isinstance(v, torch.Tensor) else v) if v is not None else None  # noqa: E731
        return lib.stac_prep_donor(addr(a["kp"]), a["T"], a["K"], addr(a["don"]), a["D"], addr(a["out"]), addr(a["gap"]), addr(a["src"]),
                                   addr(a["work"]), a["nbytes"], C.c_void_p(stream) if stream else None)

    def results(self):
        """-> (out, gap, src) as numpy arrays, without their guards; asserts that every guard word holds its pattern"""
        T, K = self.T, self.K
        got = []
        for name, shape in (("out", (T, 3 * K)), ("gap", (T, K)), ("src", (T, K)), ("work", None)):
            whole, n, pattern = self.whole[name]
            assert bool((whole[:GUARD] == pattern).all()) and bool((whole[GUARD + n:] == pattern).all()), f"guard words around {name}"
            if shape is not None:
                got.append(whole[GUARD:GUARD + n].cpu().numpy().reshape(shape))
        return got

    def untouched(self):
        return all(bool((whole == pattern).all()) for whole, _, pattern in self.whole.values())


@pytest.fixture(scope="module")
def side_stream():
    return torch.cuda.Stream()


@pytest.mark.parametrize("T", dc.TS)
@pytest.mark.parametrize("K", dc.KS)
def test_donor_fill_equals_reference(K, T, side_stream):
    """Every case of this shape, on a stream that is not the default one: outputs pre-filled with a pattern (every element is
    written: none of it survives) and the workspace poisoned to 0xFF, tolerance 0 on the bits of the three outputs; ``gap`` is that of
    ``prep.fill_missing`` on the same input; a second call (on the workspace the first one left) equals the first bit for bit."""
    from stac_mjx_amd import prep

    lib = _lib()
    cases = [c for c in dc.CASES if c[1] == T and c[2] == K]
    assert cases
    for case in cases:
        kp, don, want_out, want_gap, want_src = dc.reference(*case)
        b = _Buffers(lib, kp, don)
        torch.cuda.synchronize()
        with torch.cuda.stream(side_stream):
            rc = b.call(lib, stream=side_stream.cuda_stream)
        assert rc == 0, lib.stac_last_error().decode()
        side_stream.synchronize()
        first = b.results()
        dc.check(*first, kp, want_out, want_gap, want_src, label=str(case))
        assert not (first[1] == GAP_PATTERN).any() and not (first[0] == PATTERN).any()  # every element of out and gap was written
        assert set(np.unique(first[2])) <= set(range(b.D + 1)) | {255}                  # ... and of src (0xEE is none of its values)
        np.testing.assert_array_equal(b.kp.cpu().numpy().view(np.uint32), kp.reshape(-1).view(np.uint32))  # the source is never written
        work = b.work
        b.fill()
        b.work.copy_(work)  # (what the first call left, not the pattern)
        torch.cuda.synchronize()
        with torch.cuda.stream(side_stream):
            rc = b.call(lib, stream=side_stream.cuda_stream)
        assert rc == 0, lib.stac_last_error().decode()
        side_stream.synchronize()
        for x, y in zip(first, b.results()):
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=f"{case} second call")
        gap = prep.fill_missing(torch.as_tensor(np.array(kp)).cuda(), "linear")[1].cpu().numpy()
        np.testing.assert_array_equal(first[1], gap, err_msg=f"{case} gap of fill_missing")


def test_long_series_beyond_one_sweep_of_the_grid():
    """T = 66 000, K = 4: more tiles than the 1 024 workgroups of a launch.  Sparse holes, a run over many tiles, a trailing run that
    ends the series; through the wrapper."""
    from stac_mjx_amd import prep

    T, K, D = 66_000, 4, 2
    assert T > prep.MAX_BLOCKS * prep.TILE_FRAMES
    rng = np.random.default_rng(66_000)
    x = dc.base_series(T, K, 66)
    for t, k in zip(*np.nonzero(rng.random((T, K)) < 0.002)):
        x[t:t + int(rng.geometric(0.25)), k] = np.nan
    x[30_000:30_700, 1] = np.nan
    x[T - 3:, 2] = np.nan
    kp, don = np.ascontiguousarray(x.reshape(T, 3 * K)), dc.default_table(K, D)
    want = dc.reference_donor(kp, don)
    assert (want[2][30_000:30_700, 1] > 0).all() and (want[1][T - 3:, 2] == 3).all() and 0.005 < np.count_nonzero(want[1]) / want[1].size < 0.05
    out, gap, src = prep.fill_donors(torch.as_tensor(kp).cuda(), don)
    dc.check(out.cpu().numpy(), gap.cpu().numpy(), src.cpu().numpy(), kp, *want, label="long wrapper")


def test_raw_entry_point_alignment_and_refusals():
    lib = _lib()
    case = ("random_holes", 129, 23, 4)
    kp, don, want_out, want_gap, want_src = dc.reference(*case)
    b = _Buffers(lib, kp, don, offset=1)
    assert b.kp.data_ptr() % 4 == 0 and b.kp.data_ptr() % 16 != 0  # inputs aligned to 4 bytes only
    assert b.call(lib) == 0, lib.stac_last_error().decode()
    torch.cuda.synchronize()
    dc.check(*b.results(), kp, want_out, want_gap, want_src, label="raw, default stream")  # (and the guard words around every output)
    # every refusal happens before anything is launched: outputs and workspace keep what they hold
    b.fill()
    torch.cuda.synchronize()
    big = torch.zeros(8 * 3 * 65, dtype=torch.float32, device="cuda")
    big_don = torch.zeros(65 * 4 * 3, dtype=torch.int32, device="cuda")
    assert b.call(lib, T=8, K=65, kp=big, don=big_don) == STAC_ERR_CAPACITY and lib.stac_last_error_code() == STAC_ERR_CAPACITY
    assert lib.stac_prep_donor_workspace(8, 65) == STAC_ERR_CAPACITY
    bad = [dict(kp=None), dict(don=None), dict(out=None), dict(gap=None), dict(src=None), dict(work=None),
           dict(T=0), dict(T=-1), dict(K=0), dict(K=-2), dict(D=0), dict(D=9), dict(D=-1), dict(nbytes=b.nbytes - 1), dict(nbytes=0),
           dict(kp=b.kp.data_ptr() + 2), dict(out=b.out.data_ptr() + 1), dict(gap=b.gap.data_ptr() + 2), dict(don=b.don.data_ptr() + 2),
           dict(work=b.work.data_ptr() + 4), dict(out=b.kp), dict(out=b.source), dict(gap=b.out), dict(src=b.gap), dict(src=b.kp),
           dict(don=b.out), dict(work=b.out), dict(gap=b.work)]  # nulls, sizes, n_triples, alignment, in place and overlaps
    for over in bad:
        assert b.call(lib, **over) == STAC_ERR_INVALID and lib.stac_last_error_code() == STAC_ERR_INVALID, list(over)
    torch.cuda.synchronize()
    assert b.untouched()


def test_wrapper_input_handling_and_empty_series():
    from stac_mjx_amd import prep

    case = ("donor_missing", 129, 23, 4)
    kp_np, don, want_out, want_gap, want_src = dc.reference(*case)
    wide = torch.as_tensor(np.concatenate([kp_np, kp_np], axis=1)).cuda()[:, :kp_np.shape[1]]  # not contiguous
    assert not wide.is_contiguous()
    before = wide.clone()
    for table in (don, torch.as_tensor(np.array(don)), torch.as_tensor(np.array(don)).cuda().to(torch.int64)):  # an array, host and device tensors
        out, gap, src = prep.fill_donors(wide, table)
        assert out.is_cuda and out.dtype == torch.float32 and gap.dtype == torch.int32 and src.dtype == torch.uint8
        dc.check(out.cpu().numpy(), gap.cpu().numpy(), src.cpu().numpy(), kp_np, want_out, want_gap, want_src, label="wrapper")
    assert torch.equal(wide.contiguous().view(torch.int32), before.contiguous().view(torch.int32))  # the caller's tensor is not written
    out, gap, src = prep.fill_donors(torch.zeros(0, 12, device="cuda"), dc.default_table(4, 2))  # T == 0: empty tensors without a call
    assert tuple(out.shape) == (0, 12) and tuple(gap.shape) == (0, 4) and tuple(src.shape) == (0, 4) and src.dtype == torch.uint8
    with pytest.raises(ValueError):
        prep.fill_donors(torch.zeros(4, 13, device="cuda"), dc.default_table(4, 2))  # 13 columns are not keypoints of three
    for table in (dc.default_table(5, 2), dc.default_table(4, 2)[:, :, :2], dc.default_table(4, 2).astype(np.float32), dc.default_table(4, 8)[:, :0],
                  np.concatenate([dc.default_table(4, 8), dc.default_table(4, 1)], axis=1)):  # K, the row, the type, no row, nine rows
        with pytest.raises(ValueError):
            prep.fill_donors(torch.zeros(4, 12, device="cuda"), table)
    with pytest.raises(RuntimeError, match="65"):
        prep.fill_donors(torch.zeros(4, 3 * 65, device="cuda"), dc.default_table(65, 1))  # above the capacity: refused, nothing launched


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


ROWS = 96  # frames of the short series


@pytest.fixture(scope="module")
def holed(rodent_mocap):
    """rodent_mocap[200:296] with holes: a run of 40 frames, one across the border of the fit frames, a leading run, and a frame in
    which every keypoint is missing (nothing to carry it: left to fill_missing) -> (kp, the table of the run, what the donors make of
    it, what the linear fill makes of that)"""
    from stac_mjx_amd.prep import donor_table

    x = np.array(rodent_mocap[200:200 + ROWS], dtype=np.float32).reshape(ROWS, 23, 3)
    x[30:70, 5] = np.nan
    x[8:16, 11] = np.nan
    x[:3, 20] = np.nan
    x[80, :] = np.nan
    kp = np.ascontiguousarray(x.reshape(ROWS, 69))
    _, _, pair_n, _, pair_mad = pw.reference_pairwise(kp, pw.THR, pw.MIN_DEV, 2**31 - 1)
    don = donor_table({"pair_n": pair_n, "pair_mad": pair_mad}, 23, 4)
    d_out, d_gap, d_src = dc.reference_donor(kp, don)
    assert (d_src[80] == 255).all() and (d_src[30:70, 5] >= 1).all() and (d_src[30:70, 5] <= 4).all() and (d_src[:3, 20] < 255).all()
    final = pc.reference_fill(d_out, "linear")[0]
    assert np.isfinite(final).all()
    for a in (kp, don, d_out, d_gap, d_src, final):
        a.setflags(write=False)
    return kp, don, d_out, d_gap, d_src, final


def _datasets(path):
    from stac_mjx_amd import io

    if path.suffix == ".npz":
        with np.load(path) as f:
            return {k: np.asarray(f[k]) for k in f.files}
    with io.h5py.File(path, "r") as f:
        return {k: np.asarray(f[k][()]) for k in f.keys()}


def test_run_stac_fill_donors(tmp_path, rodent_setup, rodent_cfg, holed, capsys):
    from stac_mjx_amd.main import run_stac

    kp, don, d_out, d_gap, d_src, final = holed
    names = list(rodent_setup.kp_names)

    def run(tag, **over):
        (tmp_path / tag).mkdir()
        return run_stac(_cfg(rodent_cfg, **over), np.array(kp), names, base_path=tmp_path / tag, setup=rodent_setup)

    off = run("off", fill_missing="linear", fill_donors="off")
    log_off = capsys.readouterr().out
    auto = run("auto", fill_missing="linear", fill_donors="auto")
    log = capsys.readouterr().out
    today, today_gap = pc.reference_fill(kp, "linear")
    for p_off, p_auto, rows in zip(off, auto, (12, ROWS)):
        d_off, d_auto = _datasets(p_off), _datasets(p_auto)
        assert set(d_auto) == set(d_off) and "kp_gap" in d_auto  # no new dataset
        # reference donor fill, then reference linear fill, bit for bit; kp_gap is the gap of the series as it came
        np.testing.assert_array_equal(d_auto["kp_data"].view(np.uint32), final[:rows].view(np.uint32))
        np.testing.assert_array_equal(d_auto["kp_gap"], d_gap[:rows])
        np.testing.assert_array_equal(d_auto["kp_gap"], today_gap[:rows])
        # the key off: today's path
        np.testing.assert_array_equal(d_off["kp_data"].view(np.uint32), today[:rows].view(np.uint32))
        np.testing.assert_array_equal(d_off["kp_gap"], today_gap[:rows])
        assert "fill_donors: auto" in d_auto["config"].tobytes().decode()
    assert not np.array_equal(final.view(np.uint32), today.view(np.uint32))
    assert not [ln for ln in log_off.splitlines() if ln.startswith("fill_donors")]  # with the key off no line of the log is the stage's
    n_fit = 12 * 23
    want = ", ".join(f"triple {d + 1}: {100.0 * np.count_nonzero(d_src[:12] == d + 1) / n_fit:.3f} %" for d in range(4))
    left = 100.0 * np.count_nonzero(d_src[:12] == 255) / n_fit
    assert f"fill_donors: of the keypoints of the 12 fit frames, filled by {want}; left to fill_missing: {left:.3f} %" in log, log
    assert f"fill_donors: {names[5]}: 40 of {ROWS} frames filled from donors" in log  # (its frame 80 is left: 40 of its 41 missing ones)


def test_stac_method_on_its_own(rodent_setup, rodent_cfg, holed):
    from stac_mjx_amd.stac import Stac

    kp, don, d_out, d_gap, d_src, final = holed
    stac = Stac(None, _cfg(rodent_cfg), rodent_setup.kp_names, setup=rodent_setup, verbose=False)
    out, gap, src = stac.fill_donors(kp)  # numpy in, numpy out; the table from the pairwise statistics of this series
    dc.check(out, gap, src, kp, d_out, d_gap, d_src, label="Stac.fill_donors, automatic table")
    out, gap, src = stac.fill_donors(kp, don[:, :1])  # a table of the caller's
    dc.check(out, gap, src, kp, *dc.reference_donor(kp, don[:, :1]), label="Stac.fill_donors, one triple")
    out, gap, src = stac.fill_donors(kp, n_triples=2)
    dc.check(out, gap, src, kp, *dc.reference_donor(kp, don[:, :2]), label="Stac.fill_donors, two triples")
    with pytest.raises(ValueError):
        stac.fill_donors(kp[:, :66])
    with pytest.raises(ValueError):
        stac.fill_donors(kp, n_triples=0)
