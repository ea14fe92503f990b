"""The offset phase on observed keypoints only (stac.offset_mask), host side: the rule of csrc/mmask/stac_mmask.hpp, built for the
CPU, against the numpy float64 judge of tests/mmask_cases.py and, with every entry observed, against the oracle bit for bit; what a
masked value may hold; keypoints that are never observed; shards; every refusal of the entry points and of the pre-flight that needs
no device; the binding table against csrc/mmask/stac_mmask.h; the candidate rule of stac.fit_frames_min_observed; and the value
claim of DESIGN.md "Offsets from observed keypoints", pinned with the oracle."""

import json
import types

import numpy as np
import pytest

import host_scaffold as hs
import mmask_cases as mc


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return mc.cpu_rule(tmp_path_factory)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the rule against the float64 judge ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", mc.KS)
def test_rule_holds_the_judges_bounds(rule, K):
    partial, finish, _ = rule
    for T in mc.TS:
        for kind in mc.MASKS:
            label, kp, xpos, xquat, bodyid, valid, m0, dreg, lam = mc.case(T, K, kind)
            p = partial(kp, xpos, xquat, bodyid, valid)
            J = mc.judge_partial(p, kp, xpos, xquat, bodyid, valid, label)
            for lam_i in (lam, 0.0):
                off, err, n = finish(p, m0, dreg, lam_i)
                mc.judge_finish(off, err, n, J, m0, dreg, lam_i, f"{label}_lam{lam_i}")


def test_masked_values_reach_no_output(rule):
    """NaN, infinities and 1e30 in the masked entries: the same bits as zeros there, and as the clean series"""
    partial, finish, _ = rule
    for T, K in ((65, 23), (130, 1)):
        _, kp, xpos, xquat, bodyid, valid, m0, dreg, lam = mc.case(T, K, "random30")  # (its masked entries hold the fillers)
        assert not np.isfinite(kp).all()
        clean = np.where(np.repeat(valid, 3, axis=1), kp, 0.0).astype(np.float32)
        p, p0 = partial(kp, xpos, xquat, bodyid, valid), partial(clean, xpos, xquat, bodyid, valid)
        assert np.array_equal(_bits(p), _bits(p0)) and np.isfinite(p).all()
        for filler in (np.nan, 1e30):
            other = np.where(np.repeat(valid, 3, axis=1), kp, np.float32(filler)).astype(np.float32)
            assert np.array_equal(_bits(partial(other, xpos, xquat, bodyid, valid)), _bits(p0))
        a, b = finish(p, m0, dreg, lam), finish(p0, m0, dreg, lam)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and _bits(a[1]) == _bits(b[1]) and np.array_equal(a[2], b[2])


def test_nan_in_an_observed_value_propagates(rule):
    """As today: a NaN that the mask calls an observation poisons its keypoint's sums and z2, and nothing else"""
    partial, finish, _ = rule
    _, kp, xpos, xquat, bodyid, valid, m0, dreg, lam = mc.case(65, 23, "random30")
    t, k = (int(i) for i in np.argwhere(valid)[7])
    kp = kp.copy()
    kp[t, 3 * k + 1] = np.nan
    p = partial(kp, xpos, xquat, bodyid, valid)
    s = p[:69].reshape(23, 3)
    assert np.isnan(s[k]).all() and np.isfinite(np.delete(s, k, axis=0)).all() and np.isnan(p[4 * 23]) and np.isfinite(p[69:92]).all()
    off, err, n = finish(p, m0, dreg, lam)
    assert np.isnan(off[k]).all() and np.isfinite(np.delete(off, k, axis=0)).all() and np.isnan(err)


def test_body_outside_the_model_counts_as_never_observed(rule):
    partial, _, _ = rule
    _, kp, xpos, xquat, bodyid, valid, *_ = mc.case(64, 23, "all_valid")
    for bad in (-1, mc.NBODY, 2**31 - 1):
        b = bodyid.copy()
        b[4] = bad
        p = partial(kp, xpos, xquat, b, valid)
        v = valid.copy()
        v[:, 4] = False
        assert np.array_equal(_bits(p), _bits(partial(kp, xpos, xquat, bodyid, v))) and p[69 + 4] == 0
        mc.judge_partial(p, kp, xpos, xquat, b, valid, f"body {bad}")


def test_keypoint_never_observed(rule):
    """It keeps m0 where it is not regularised and gets lam d m0 / (lam d) where it is; its n is 0"""
    partial, finish, _ = rule
    _, kp, xpos, xquat, bodyid, valid, m0, _, _ = mc.case(130, 23, "one_kp_never")
    k = 23 // 2
    dreg = np.zeros((23, 3), np.float32)
    dreg[k] = [0.0, 1.0, 2.5]
    lam = np.float32(0.3)
    p = partial(kp, xpos, xquat, bodyid, valid)
    off, err, n = finish(p, m0, dreg, lam)
    assert n[k] == 0 and (np.delete(n, k) == 130).all()
    assert _bits(off[k, 0]) == _bits(m0[k, 0])
    for i in (1, 2):
        want = (np.float32(0.0) + lam * dreg[k, i] * m0[k, i]) / (np.float32(0.0) + lam * dreg[k, i])
        assert _bits(off[k, i]) == _bits(want)
    assert np.isfinite(err)
    off0, _, _ = finish(p, m0, dreg, 0.0)  # lam = 0: nothing determines any of its coordinates
    assert np.array_equal(_bits(off0[k]), _bits(m0[k]))
    # nobody observed at all, no frames at all
    pz = partial(kp, xpos, xquat, bodyid, np.zeros_like(valid))
    assert not pz[:-1].any() and pz[-1] == 130
    offz, errz, nz = finish(pz, m0, np.zeros_like(dreg), lam)
    assert np.array_equal(_bits(offz), _bits(m0)) and errz == 0 and not nz.any()
    pe = partial(kp[:0], xpos[:0], xquat[:0], bodyid, valid[:0])
    assert not pe.any() and not np.signbit(pe).any()


def test_two_shards_add_up(rule):
    partial, finish, _ = rule
    label, kp, xpos, xquat, bodyid, valid, m0, dreg, lam = mc.case(1000, 23, "random30")
    cut = 377
    pa = partial(kp[:cut], xpos[:cut], xquat[:cut], bodyid, valid[:cut])
    pb = partial(kp[cut:], xpos[cut:], xquat[cut:], bodyid, valid[cut:])
    J = mc.judge_partial(pa + pb, kp, xpos, xquat, bodyid, valid, label)  # (one more rounding per word: inside the serial bound)
    off, err, n = finish(pa + pb, m0, dreg, lam)
    mc.judge_finish(off, err, n, J, m0, dreg, lam, label)
    assert np.array_equal((pa + pb)[69:92], partial(kp, xpos, xquat, bodyid, valid)[69:92])


# ---- every entry observed: the oracle's bits -------------------------------------------------------------------------------------
def _against_oracle(rule, orc, kp, q, m0, dreg, lam, label):
    partial, finish, _ = rule
    K = orc.K
    xpos, xquat = mc.oracle_bodies(orc, q)
    valid = np.ones((kp.shape[0], K), bool)
    p = partial(kp, xpos, xquat, orc.t.site_bodyid, valid)
    ref = orc.m_partial(kp, q)
    assert np.array_equal(_bits(p[: 3 * K]), _bits(ref[: 3 * K])), (label, "s")
    assert _bits(p[4 * K]) == _bits(ref[3 * K]) and _bits(p[4 * K + 1]) == _bits(ref[3 * K + 1]), (label, "z2, T")
    assert (p[3 * K: 4 * K] == kp.shape[0]).all(), label
    off, err, n = finish(p, m0, dreg, lam)
    ref_off, ref_err = orc.m_finish(ref, m0, dreg, lam)
    assert np.array_equal(_bits(off), _bits(ref_off)), (label, "offsets")
    J = mc.judge_partial(p, kp, xpos, xquat, orc.t.site_bodyid, valid, label)
    _, e64, be = mc.judge_finish(off, err, n, J, m0, dreg, lam, label)
    assert abs(ref_err - e64) <= be, (label, "the oracle's err", ref_err, e64, be)  # (both inside the bound of the same float64 value)
    return off, err, ref_err


def test_all_valid_equals_the_oracle_on_the_rodent(rule, rodent_setup, rodent_cfg, rodent_mocap, demo_viz):
    from oracle import Oracle

    fs = rodent_setup
    orc = Oracle(fs.tables)
    kp = rodent_mocap[:120].astype(np.float32)
    rng = np.random.default_rng(3)
    q = np.tile(fs.tables.qpos0, (120, 1)).astype(np.float32)
    q[:, :3] = kp[:, :3] + rng.normal(0, 0.01, (120, 3))
    q[:, 3:7] = rng.normal(0, 1, (120, 4))
    q[:, 7:] += rng.normal(0, 0.2, (120, q.shape[1] - 7)).astype(np.float32)
    m0 = fs.tables.site_pos.astype(np.float32)
    for lam in (float(rodent_cfg["M_REG_COEF"]), 0.0):
        _against_oracle(rule, orc, kp, q, m0, fs.is_regularized, lam, f"rodent lam {lam}")


def test_all_valid_equals_the_oracle_on_the_known_answers(rule, toy_tables):
    from oracle import Oracle

    for label, q, gt, m0, dreg, lam in mc.known_answer_cases():
        orc = Oracle(toy_tables)
        orc.set_site_pos(gt)
        kp = np.stack([orc.fk(row)["site_xpos"].reshape(-1) for row in q])
        off, err, ref_err = _against_oracle(rule, orc, kp, q, m0, dreg, lam, label)
        if label in ("identity", "varied", "sweep", "reg_zero"):  # (the answers the reference's tests know)
            np.testing.assert_allclose(off, gt, atol=1e-5)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _mmask_lib():
    from stac_mjx_amd.build import build_extension
    from stac_mjx_amd.engine import load_mmask_library

    build_extension()
    return load_mmask_library()


def _refused(lib, rc, code):
    msg = lib.stac_mmask_last_error().decode()
    assert rc == code and lib.stac_mmask_last_error_code() == code and msg, (rc, code, msg)
    return msg


def test_workspace_function_and_its_refusals(rule):
    lib = _mmask_lib()
    for T, K in ((0, 1), (1, 1), (63, 23), (64, 64), (1000, 23), (2**24, 4096)):
        got = lib.stac_mmask_workspace(T, K)
        assert got == rule[2].mmask_bytes(T, K) and got % 8 == 0 and got >= max(4 * T * (3 * K + 1), 8)
        assert lib.stac_mmask_last_error_code() == 0
    for T, K, code in ((-1, 3, hs.STAC_ERR_INVALID), (2**24 + 1, 3, hs.STAC_ERR_INVALID), (10, 0, hs.STAC_ERR_INVALID),
                       (10, -2, hs.STAC_ERR_INVALID), (10, 4097, hs.STAC_ERR_CAPACITY)):
        _refused(lib, lib.stac_mmask_workspace(T, K), code)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every refusal comes before the device is touched: made-up addresses do on a machine without a GPU"""
    lib = _mmask_lib()
    T, K, nbody = 100, 3, 5
    need = lib.stac_mmask_workspace(T, K)
    base, step = 1 << 20, 1 << 16
    good = dict(kp=base, xpos=base + step, xquat=base + 2 * step, nbody=nbody, bodyid=base + 3 * step, valid=base + 4 * step, T=T, K=K,
                work=base + 5 * step, nbytes=need, partial=base + 6 * step)

    def call(**over):
        a = dict(good)
        a.update(over)
        return lib.stac_mmask_partial(a["kp"], a["xpos"], a["xquat"], a["nbody"], a["bodyid"], a["valid"], a["T"], a["K"], a["work"], a["nbytes"],
                                      a["partial"], None)

    inv, cap = hs.STAC_ERR_INVALID, hs.STAC_ERR_CAPACITY
    for over, code, word in (
            (dict(T=-1), inv, "n_frames"), (dict(T=2**24 + 1), inv, "2^24"), (dict(K=0), inv, "n_kp"), (dict(K=4097), cap, "n_kp"),
            (dict(nbody=0), inv, "nbody"), (dict(nbody=65537), inv, "nbody"), (dict(nbytes=need - 1), inv, "workspace_bytes"),
            (dict(kp=None), inv, "null kp"), (dict(xpos=None), inv, "null xpos"), (dict(xquat=None), inv, "null xquat"),
            (dict(bodyid=None), inv, "null site_bodyid"), (dict(valid=None), inv, "null valid"), (dict(work=None), inv, "null workspace"),
            (dict(partial=None), inv, "null partial"), (dict(kp=base + 2), inv, "kp must be 4-byte aligned"),
            (dict(xpos=good["xpos"] + 1), inv, "xpos must be 4-byte"), (dict(xquat=good["xquat"] + 3), inv, "xquat must be 4-byte"),
            (dict(bodyid=good["bodyid"] + 2), inv, "site_bodyid must be 4-byte"), (dict(work=good["work"] + 2), inv, "workspace must be 4-byte"),
            (dict(partial=good["partial"] + 1), inv, "partial must be 4-byte"),
            (dict(xpos=base + 12 * T * K - 4), inv, "kp and xpos overlap"), (dict(partial=good["work"] + need - 4), inv, "workspace and partial overlap"),
            (dict(valid=good["partial"] + 4), inv, "valid and partial overlap"), (dict(work=good["kp"]), inv, "kp and workspace overlap"),
            (dict(partial=good["bodyid"] + 8), inv, "site_bodyid and partial overlap"), (dict(valid=good["xquat"] + 16 * T * nbody - 1), inv, "xquat and valid overlap")):
        assert word in _refused(lib, call(**over), code), over

    K3 = 12 * K
    fgood = dict(partial=base, K=K, m0=base + step, dreg=base + 2 * step, off=base + 3 * step, err=base + 4 * step, n=base + 5 * step)

    def fcall(**over):
        a = dict(fgood)
        a.update(over)
        return lib.stac_mmask_finish(a["partial"], a["K"], a["m0"], a["dreg"], 1.0, a["off"], a["err"], a["n"], None)

    for over, code, word in (
            (dict(K=0), inv, "n_kp"), (dict(K=4097), cap, "n_kp"), (dict(partial=None), inv, "null partial"), (dict(m0=None), inv, "null m0"),
            (dict(dreg=None), inv, "null dreg"), (dict(off=None), inv, "null offsets_out"), (dict(partial=base + 2), inv, "partial must be 4-byte"),
            (dict(off=fgood["off"] + 1), inv, "offsets_out must be 4-byte"), (dict(err=fgood["err"] + 2), inv, "err_out must be 4-byte"),
            (dict(n=fgood["n"] + 2), inv, "n_out must be 4-byte"), (dict(off=fgood["m0"]), inv, "m0 and offsets_out overlap"),
            (dict(off=base + 4 * (4 * K + 2) - 4), inv, "partial and offsets_out overlap"), (dict(err=fgood["off"] + K3 - 4), inv, "offsets_out and err_out overlap"),
            (dict(n=fgood["dreg"] + 4), inv, "dreg and n_out overlap")):
        assert word in _refused(lib, fcall(**over), code), over


def test_option_refusals(rodent_cfg):
    from stac_mjx_amd.config import ConfigError, offset_mask_options
    from stac_mjx_amd.main import _Preflight

    assert offset_mask_options({}) == ("off", 1.0) and offset_mask_options({"offset_mask": False, "fit_frames_min_observed": None}) == ("off", 1.0)
    assert offset_mask_options({"offset_mask": "observed", "fit_frames_min_observed": 0.5}) == ("observed", 0.5)
    assert offset_mask_options({"offset_mask": "observed", "fit_frames_min_observed": 1}) == ("observed", 1.0)
    for bad in ("on", "Observed", True, 1, ["observed"]):
        with pytest.raises(ConfigError, match="stac.offset_mask must be off or observed"):
            hs.stage_cfg(rodent_cfg, offset_mask=bad, fill_missing="linear")
    for bad in (0, 0.0, -0.5, 1.0001, 2, "0.5", True, float("nan"), float("inf")):
        with pytest.raises(ConfigError, match=r"stac.fit_frames_min_observed must be a number in \(0, 1\]"):
            hs.stage_cfg(rodent_cfg, offset_mask="observed", fill_missing="linear", fit_frames_min_observed=bad)
    for mask in ({}, {"offset_mask": "off"}):
        with pytest.raises(ConfigError, match="honoured only with stac.offset_mask = observed"):
            hs.stage_cfg(rodent_cfg, fit_frames_min_observed=0.9, fill_missing="linear", **mask)
    hs.stage_cfg(rodent_cfg, fit_frames_min_observed=1.0)  # (1.0 is today's rule: no mask needed)
    # the pre-flight: the mask reads kp_gap, the mark of fill_missing
    for fill in ({}, {"fill_missing": "off"}):
        with pytest.raises(ValueError, match="stac.offset_mask = observed reads .* kp_gap.*set stac.fill_missing"):
            _Preflight(hs.stage_cfg(rodent_cfg, offset_mask="observed", **fill), 100, "fit.h5").check_config()
    for fill in ("linear", "hold"):
        pre = _Preflight(hs.stage_cfg(rodent_cfg, offset_mask="observed", fill_missing=fill, fit_frames_min_observed=0.75), 100, "fit.h5")
        pre.check_config()
        assert (pre.offset_mask, pre.min_observed) == ("observed", 0.75)
    pre = _Preflight(hs.stage_cfg(rodent_cfg), 100, "fit.h5")
    pre.check_config()
    assert (pre.offset_mask, pre.min_observed) == ("off", 1.0)


def test_wrapper_refusals():
    """Engine-free: fit_offsets checks ``valid`` before any device work"""
    from stac_mjx_amd.stac import Stac

    stub = types.SimpleNamespace(cfg=types.SimpleNamespace(model=None, stac={}), engine=None, _kp_names=["a", "b"])
    kp = np.zeros((4, 6), np.float32)
    for bad in (np.ones((4, 2), np.uint8), np.ones((4, 3), bool), np.ones((3, 2), bool), np.ones(8, bool)):
        with pytest.raises(ValueError, match="valid must be a bool array"):
            Stac.fit_offsets(stub, kp, valid=bad)


# ---- stac.fit_frames_min_observed ---------------------------------------------------------------------------------------------------
def test_min_observed_candidate_rule(rodent_cfg, tmp_path):
    from stac_mjx_amd.main import _select_fit_frames, _Series, _write_frames, fit_frame_exclude, min_observed_count
    from stac_mjx_amd.stac import Stac

    assert [min_observed_count(q, 10) for q in (1.0, 0.7, 0.71, 0.05, 0.1, 0.3)] == [10, 7, 8, 1, 1, 3]
    assert [min_observed_count(q, 23) for q in (1.0, 0.8, 0.5, 1 / 23)] == [23, 19, 12, 1]
    T, K = 12, 10
    gap = np.zeros((T, K), np.int32)
    for t in range(T):
        gap[t, : min(t, K)] = 5  # frame t has t filled keypoints (from 10 on: all of them)
    swapped = np.zeros((T, K), np.uint8)
    swapped[1, [2, 3]] = 1
    cand = lambda q, sw=swapped: np.flatnonzero(~fit_frame_exclude(gap, sw, q)).tolist()  # noqa: E731
    assert cand(1.0) == [0] and cand(0.7) == [0, 2, 3] and cand(0.71) == [0, 2] and cand(0.05) == [0, 2, 3, 4, 5, 6, 7, 8, 9]
    assert cand(0.7, None) == [0, 1, 2, 3] and cand(1.0, None) == [0]
    # through the selection of run_stac: strided needs no device
    kp = np.random.default_rng(2).normal(0, 0.05, (T, 69)).astype(np.float32)
    gap23 = np.zeros((T, 23), np.int32)
    gap23[3:, 0] = 4       # one keypoint filled in frames 3 ..: today's rule leaves frames 0 .. 2
    gap23[8:, 1:12] = 4    # 12 of 23 filled in frames 8 ..
    series = _Series(kp, {"kp_gap": gap23})
    stub = types.SimpleNamespace(_kp_names=[f"k{i}" for i in range(23)], _log=lambda *a: None)
    stub.select_frames = types.MethodType(Stac.select_frames, stub)
    over = dict(fit_frames="strided", offset_mask="observed", fill_missing="linear")
    rows, info = _select_fit_frames(stub, hs.stage_cfg(rodent_cfg, n_fit_frames=8, fit_frames_min_observed=0.9, **over), series, "strided", 0.9)
    assert rows.tolist() == list(range(8)) and info["min_observed"] == 0.9
    rows, info = _select_fit_frames(stub, hs.stage_cfg(rodent_cfg, n_fit_frames=3, **over), series, "strided", 1.0)
    assert rows.tolist() == [0, 1, 2]
    with pytest.raises(ValueError, match=r"only 8 of the 12 frames have at least 21 of their 23 keypoints observed \(stac.fit_frames_min_observed = 0.9\)"):
        _select_fit_frames(stub, hs.stage_cfg(rodent_cfg, n_fit_frames=9, fit_frames_min_observed=0.9, **over), series, "strided", 0.9)
    with pytest.raises(ValueError, match="only 3 of the 12 frames carry no mark"):  # (mask off: today's rule and text)
        _select_fit_frames(stub, hs.stage_cfg(rodent_cfg, n_fit_frames=4, fit_frames="strided"), series, "strided")
    path = _write_frames(tmp_path / "fit.npz", rows, info)
    assert json.loads(path.read_text())["min_observed"] == 1.0


def test_run_fit_hands_the_rows_of_the_mask_to_fit_offsets(rodent_cfg):
    """``valid = kp_gap == 0`` sliced with the fit rows, the first ones or the selected ones; without the option no ``valid`` at all"""
    from stac_mjx_amd.main import _run_fit, _Series
    from stac_mjx_amd.stac import Stac

    class Stop(Exception):
        pass

    T, K = 20, 23
    kp = np.random.default_rng(4).normal(0, 0.05, (T, 3 * K)).astype(np.float32)
    gap = np.zeros((T, K), np.int32)
    gap[2:6, 3] = 4
    gap[9:, 7] = 11
    gap[0, 1:8] = 1  # (7 of 23 filled: frame 0 is no candidate at q = 0.9, which wants 21)
    series = _Series(kp, {"kp_gap": gap})
    seen = {}

    def fit_offsets(kps, **kw):
        seen.update(kps=kps, kw=kw)
        raise Stop

    stub = types.SimpleNamespace(_kp_names=[f"k{i}" for i in range(K)], _log=lambda *a: None, fit_offsets=fit_offsets)
    stub.select_frames = types.MethodType(Stac.select_frames, stub)
    over = dict(offset_mask="observed", fill_missing="linear", n_fit_frames=6)
    with pytest.raises(Stop):
        _run_fit(stub, hs.stage_cfg(rodent_cfg, **over), series, "fit.h5", (False, None, None), "first", "observed", 1.0)
    assert np.array_equal(seen["kps"], kp[:6]) and seen["kw"]["valid"].dtype == np.bool_ and np.array_equal(seen["kw"]["valid"], gap[:6] == 0)
    with pytest.raises(Stop):
        _run_fit(stub, hs.stage_cfg(rodent_cfg, fit_frames="strided", fit_frames_min_observed=0.9, **over), series, "fit.h5", (False, None, None),
                 "strided", "observed", 0.9)
    rows = np.array([(i * 19) // 6 for i in range(6)]) + 1  # even steps through the 19 candidates 1 .. 19
    assert np.array_equal(seen["kps"], kp[rows]) and np.array_equal(seen["kw"]["valid"], gap[rows] == 0)
    with pytest.raises(Stop):
        _run_fit(stub, hs.stage_cfg(rodent_cfg, n_fit_frames=6, fill_missing="linear"), series, "fit.h5", (False, None, None))
    assert seen["kw"] == {} and np.array_equal(seen["kps"], kp[:6])


def test_offsets_sidecar(tmp_path):
    from stac_mjx_amd.main import _write_offset_counts, offset_counts_path

    path = _write_offset_counts(tmp_path / "fit.npz", ["a", "b", "c"], {"n": np.array([5, 0, 7], np.int32), "n_sampled": 7})
    assert path == offset_counts_path(tmp_path / "fit.npz") and path.name == "fit.npz.offsets.json"
    assert json.loads(path.read_text()) == {"kp_names": ["a", "b", "c"], "n": [5, 0, 7], "n_sampled": 7, "never_observed": ["b"]}


# ---- binding ----------------------------------------------------------------------------------------------------------------------
def test_mmask_prototypes_equal_the_header(monkeypatch):
    """abi.MMASK_PROTOTYPES against csrc/mmask/stac_mmask.h with the comparison that test_host.py makes for the main table; the library
    carries them; and the main table, the main header and the build's globs know nothing of the companion."""
    import re

    from stac_mjx_amd import abi, build

    header = hs.CSRC / "mmask" / "stac_mmask.h"
    monkeypatch.setattr(hs, "HEADER", header)
    protos, n_statements = hs.header_prototypes()
    declared = set(re.findall(r"\b(stac_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header.read_text(), flags=re.S)))
    assert n_statements == len(protos) == 5 and set(protos) == declared and tuple(abi.MMASK_PROTOTYPES) == tuple(protos)
    for name, (ret, args) in protos.items():
        restype, argtypes = abi.MMASK_PROTOTYPES[name]
        assert hs.ctypes_class(restype) == ret, name
        assert [hs.ctypes_class(t) for t in argtypes] == [c for c, _ in args], name
    lib = _mmask_lib()
    for name, (restype, argtypes) in abi.MMASK_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name
    assert not set(abi.MMASK_PROTOTYPES) & (set(abi.PROTOTYPES) | set(abi.SELECT_PROTOTYPES)) and len(abi.PROTOTYPES) == 39
    assert build.MMASK_LIB.parent == hs.CSRC / "mmask" and not any(p.parent == build.MMASK_DIR for p in build.SOURCES + build.HEADERS)
    assert set(build.MMASK_SOURCES) == set(build.MMASK_DIR.glob("*.hip")) and header in build.MMASK_HEADERS
    assert build.MMASK_DIR / "stac_mmask.hpp" in build.MMASK_HEADERS
    text = (build.MMASK_DIR / "stac_mmask.hpp").read_text()
    assert "kMmaskMaxFrames = 1ll << 24;" in text and "kMmaskMaxKp = 4096;" in text
    assert not build.mmask_is_stale() and build.MMASK_STAMP.read_text().strip() == build.mmask_digest()


# ---- the value claim --------------------------------------------------------------------------------------------------------------
N_ITERS_VALUE = 6  # (the golden config's N_ITERS: the two fits take about half a minute on the CPU oracle)


def test_mask_lowers_the_held_out_error_on_long_gaps(rule, rodent_setup, rodent_cfg, rodent_mocap):
    """Six keypoints (seed 0) lose a run of 100 of the fit rows 0 .. 299 each and are filled linearly.  Offsets fitted by the float32
    oracle as one chain over the 300 rows, N_ITERS = 6, M_REG_COEF of the golden config, all 300 rows in the offset phase, which is
    the CPU rule with the mask and the oracle's m_opt without; scored on rows 400 .. 990 step 10, fitted as independent frames, by the
    mean marker-to-keypoint distance of the six keypoints.  With the mask the error must be lower (the design measured 2.20 against
    2.56 mm with a float64 closed form; this test: DESIGN.md "Offsets from observed keypoints")."""
    from oracle import Oracle

    partial, finish, _ = rule
    fs, cfgm = rodent_setup, rodent_cfg
    kp = rodent_mocap.astype(np.float32)
    filled, valid, which = mc.cut_holes(kp[:300], 6, 100, 0)
    fill_mm = float(np.linalg.norm((filled - kp[:300]).reshape(300, -1, 3)[~valid], axis=-1).mean() * 1e3)
    held = np.ascontiguousarray(kp[400:1000:10])
    lam = float(cfgm["M_REG_COEF"])
    err = {}
    for mode in ("unmasked", "masked"):
        orc = Oracle(fs.tables, tol=float(cfgm["FTOL"]), maxiter=int(cfgm["N_ITER_Q"]))
        offsets = fs.tables.site_pos.astype(np.float32).copy()
        q = fs.tables.qpos0
        if fs.do_root_opt:
            q, _ = orc.root_optimization(filled, q, fs.lb, fs.ub, fs.trunk_kps, fs.root_kp_idx, fs.root_dims)
        for _ in range(N_ITERS_VALUE):
            out = orc.pose_optimization(filled, q, fs.lb, fs.ub, fs.part_masks)
            q = out["carry_qpos"]
            if mode == "masked":
                offsets, _, n = finish(partial(filled, out["xpos"], out["xquat"], fs.tables.site_bodyid, valid), offsets, fs.is_regularized, lam)
                assert (n[which] == 200).all() and (np.delete(n, which) == 300).all()
            else:
                offsets, _ = orc.m_opt(filled, out["qpos"], offsets, fs.is_regularized, lam)
            orc.set_site_pos(offsets)
        fit = orc.ik_clips(held.reshape(held.shape[0], 1, -1), fs.lb, fs.ub, fs.part_masks, fs.trunk_kps, fs.root_kp_idx, fs.root_dims)
        d = np.linalg.norm(fit["marker_sites"].reshape(held.shape[0], -1, 3) - held.reshape(held.shape[0], -1, 3), axis=-1)
        err[mode] = float(d[:, which].mean() * 1e3)
    print(f"holes in keypoints {which.tolist()}, fill error {fill_mm:.3f} mm; held-out error on them, mm: unmasked {err['unmasked']:.4f}, "
          f"masked {err['masked']:.4f} (N_ITERS = {N_ITERS_VALUE})")
    assert err["masked"] < err["unmasked"], err
