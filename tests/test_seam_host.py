"""Warm-started clips (stac.seam_passes) and pose steps (stac.seam_report), host side: the rule of csrc/seam/stac_seam.hpp, built for
the CPU, against the numpy float32 judge of tests/seam_cases.py at tolerance 0; values that are not finite; every refusal of the entry
point, which needs no device; the binding table against csrc/seam/stac_seam.h; the options and the pre-flight; the neighbour rule of
the rank exchange; and the value of the passes, pinned with the oracle (DESIGN.md "Warm-started clips and pose steps")."""

import types

import numpy as np
import pytest

import host_scaffold as hs
import seam_cases as sc


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return sc.cpu_rule(tmp_path_factory)


# ---- the rule against the judge ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", sc.NQS)
def test_rule_equals_the_judge(rule, nq):
    steps, _ = rule
    cases = sc.cases(nq)
    assert {c[0].split("_")[0] for c in cases} == {f"N{N}" for N in sc.NS}
    for label, q, L, cols, n_lin in cases:
        sc.same(steps(q, L, cols, n_lin), sc.judge(q, L, cols, n_lin), label)


def test_the_cases_cover_what_they_claim():
    """Every layout that fits, every clip length that divides, ties for the largest step and a negative r"""
    assert [len(sc.layouts(nq)) for nq in sc.NQS] == [1, 4, 6, 6]
    labels = [c[0] for nq in sc.NQS for c in sc.cases(nq)]
    assert len(labels) == len(set(labels))
    for L in (1, 5, 13, 65, 130):
        assert any(f"_L{L}_" in lab for lab in labels), L
    _, q, L, cols, n_lin = next(c for c in sc.cases(74) if c[0] == "N64_nq74_L1_quat0_lin0")
    d = np.abs(np.diff(q, axis=0))
    assert ((d == d.max(axis=1, keepdims=True)).sum(axis=1) > 1).any()  # (quantised: two columns tie)
    _, q, L, cols, n_lin = next(c for c in sc.cases(74) if c[0] == "N65_nq74_L5_quat2_lin3")
    assert cols == (62, 3) and (1 - np.abs((q[:-1, 62:66] * q[1:, 62:66]).sum(axis=1)) < 0).any()
    _, q, L, cols, n_lin = next(c for c in sc.cases(74) if c[0] == "N65_nq74_L5_quat1_lin3")  # (one block, scaled: the largest r is negative)
    assert (sc.judge(q, L, cols, n_lin)["step_rot"][1:] < 0).any()


def test_row_zero_and_a_single_row(rule):
    steps, _ = rule
    for nq, cols, n_lin in ((1, (), 0), (74, (3,), 3)):
        out = steps(sc.series(1, nq, cols, 5, False), 1, cols, n_lin)
        assert out["step_col"].tolist() == [-1]
        for k in ("step_joint", "step_rot", "step_lin2", "col_max_in", "col_max_seam"):
            assert not sc.bits(out[k]).any(), k  # (+0 everywhere)
    # without a scalar column: +0 and -1 in every row
    q = sc.series(10, 7, (3,), 6, False)
    out = steps(q, 5, (3,), 3)
    assert not sc.bits(out["step_joint"]).any() and (out["step_col"] == -1).all() and (out["step_lin2"][1:] > 0).all()
    # clip_len 1: every step is a seam; one clip: none is
    q = sc.series(20, 9, (), 7, False)
    assert not steps(q, 1)["col_max_in"].any() and steps(q, 1)["col_max_seam"].all()
    assert steps(q, 20)["col_max_in"].all() and not steps(q, 20)["col_max_seam"].any()


@pytest.mark.parametrize("value,where", sc.POISONS)
def test_values_that_are_not_finite(rule, value, where):
    """A NaN or an infinity in row t: the quiet NaN (and -1) in the outputs of rows t and t + 1 that the column enters, the other
    outputs of those rows and every other row as without it; the column maxima skip it"""
    steps, _ = rule
    for N, nq in ((65, 74), (130, 230)):
        label, q, L, cols, n_lin = sc.poisoned(N, nq, value, where)
        got = steps(q, L, cols, n_lin)
        sc.same(got, sc.judge(q, L, cols, n_lin), label)
        clean = q.copy()
        hit = ~np.isfinite(q)
        assert hit.sum() == 2
        clean[hit] = 0.25
        ref = steps(clean, L, cols, n_lin)
        touched = {"scalar": "step_joint", "block": "step_rot", "lin": "step_lin2"}[where]
        rows = sorted({t + k for t in np.flatnonzero(hit.any(axis=1)) for k in (0, 1)})
        for k in ("step_joint", "step_rot", "step_lin2"):
            if k == touched:
                assert (sc.bits(got[k][rows]) == 0x7FC00000).all(), (label, k)
                keep = np.ones(N, bool)
                keep[rows] = False
                assert np.array_equal(sc.bits(got[k][keep]), sc.bits(ref[k][keep])), (label, k)
            else:
                assert np.array_equal(sc.bits(got[k]), sc.bits(ref[k])), (label, k)
        assert (got["step_col"][rows] == -1).all() if where == "scalar" else np.array_equal(got["step_col"], ref["step_col"])
        for k in ("col_max_in", "col_max_seam"):
            assert np.isfinite(got[k]).all() and (got[k] >= 0).all() and not np.signbit(got[k]).any(), (label, k)
            j = int(np.flatnonzero(hit.any(axis=0))[0])
            j = cols[0] if where == "block" else j  # (a block's measure lives in its first column)
            assert np.array_equal(np.delete(sc.bits(got[k]), j), np.delete(sc.bits(ref[k]), j)), (label, k)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _seam_lib():
    from stac_mjx_amd.build import build_extension
    from stac_mjx_amd.engine import load_seam_library

    build_extension()
    return load_seam_library()


def _refused(lib, rc, code):
    msg = lib.stac_seam_last_error().decode()
    assert rc == code and lib.stac_seam_last_error_code() == code and msg, (rc, code, msg)
    return msg


def test_entry_point_refuses_bad_arguments_before_any_launch(rule):
    """Every refusal comes before the device is touched: made-up addresses do on a machine without a GPU"""
    import ctypes as C

    lib = _seam_lib()
    N, nq = 100, 74
    base, step = 1 << 20, 1 << 16
    good = dict(qpos=base, N=N, nq=nq, L=10, cols=(3, 40), n_lin=3, sj=base + step, sc=base + 2 * step, sr=base + 3 * step, sl=base + 4 * step,
                cin=base + 5 * step, cseam=base + 6 * step)

    def call(**over):
        a = dict(good)
        a.update(over)
        cols = None if a["cols"] is None else (C.c_int32 * max(len(a["cols"]), 1))(*a["cols"])
        n_quat = a.get("n_quat", 0 if a["cols"] is None else len(a["cols"]))
        return lib.stac_seam_steps(a["qpos"], a["N"], a["nq"], a["L"], cols, n_quat, a["n_lin"], a["sj"], a["sc"], a["sr"], a["sl"], a["cin"],
                                   a["cseam"], None)

    inv, cap = hs.STAC_ERR_INVALID, hs.STAC_ERR_CAPACITY
    for over, code, word in (
            (dict(N=0), inv, "n_rows"), (dict(N=-5), inv, "n_rows"), (dict(N=2**32 + 1, L=1), inv, "n_rows"), (dict(nq=0), inv, "nq >= 1"),
            (dict(nq=-1), inv, "nq >= 1"), (dict(nq=4097), cap, "nq = 4097"), (dict(L=0), inv, "clip_len >= 1"), (dict(L=-10), inv, "clip_len >= 1"),
            (dict(L=7), inv, "not whole clips"), (dict(L=200), inv, "not whole clips"), (dict(cols=(3,) * 65), inv, "n_quat = 65"),
            (dict(n_quat=-1), inv, "n_quat = -1"), (dict(cols=None, n_quat=1), inv, "null quat_cols"),
            (dict(cols=(3, 6)), inv, "overlap"), (dict(cols=(40, 3, 43)), inv, "overlap"), (dict(cols=(3, 3)), inv, "overlap"),
            (dict(cols=(2,)), inv, "outside the columns"), (dict(cols=(71,)), inv, "outside the columns"), (dict(cols=(-1,)), inv, "outside the columns"),
            (dict(cols=(0,)), inv, "outside the columns"), (dict(n_lin=1), inv, "n_lin = 1"), (dict(n_lin=-3), inv, "n_lin = -3"),
            (dict(n_lin=6), inv, "n_lin = 6"), (dict(nq=2, cols=(), n_lin=3), inv, "n_lin = 3"),
            (dict(qpos=None), inv, "null qpos"), (dict(sj=None), inv, "null step_joint"), (dict(sc=None), inv, "null step_col"),
            (dict(sr=None), inv, "null step_rot"), (dict(sl=None), inv, "null step_lin2"), (dict(cin=None), inv, "null col_max_in"),
            (dict(cseam=None), inv, "null col_max_seam"), (dict(qpos=base + 2), inv, "qpos must be 4-byte"),
            (dict(sj=good["sj"] + 1), inv, "step_joint must be 4-byte"), (dict(sc=good["sc"] + 2), inv, "step_col must be 4-byte"),
            (dict(sr=good["sr"] + 3), inv, "step_rot must be 4-byte"), (dict(sl=good["sl"] + 1), inv, "step_lin2 must be 4-byte"),
            (dict(cin=good["cin"] + 2), inv, "col_max_in must be 4-byte"), (dict(cseam=good["cseam"] + 2), inv, "col_max_seam must be 4-byte"),
            (dict(sj=base + 4 * N * nq - 4), inv, "qpos and step_joint overlap"), (dict(sc=good["sj"]), inv, "step_joint and step_col overlap"),
            (dict(sr=good["sc"] + 4 * N - 4), inv, "step_col and step_rot overlap"), (dict(sl=good["sr"] + 4), inv, "step_rot and step_lin2 overlap"),
            (dict(cin=good["sl"] + 8), inv, "step_lin2 and col_max_in overlap"), (dict(cseam=good["cin"] + 4 * nq - 4), inv, "col_max_in and col_max_seam overlap"),
            (dict(cseam=base + 16), inv, "qpos and col_max_seam overlap")):
        assert word in _refused(lib, call(**over), code), over
    # the layout check is the header's, whichever side asks
    _, cpu = rule
    arr = lambda *c: np.array(c, np.int32).ctypes.data  # noqa: E731
    assert cpu.seam_layout(74, arr(3, 40), 2, 3) == 0 and cpu.seam_layout(74, arr(3, 70), 2, 3) == 0 and cpu.seam_layout(7, arr(3), 1, 3) == 0
    assert cpu.seam_layout(74, arr(3, 6), 2, 3) == 5 and cpu.seam_layout(74, arr(71), 1, 0) == 4 and cpu.seam_layout(2, None, 0, 3) == 3
    assert cpu.seam_layout(0, None, 0, 0) == 1 and cpu.seam_layout(5, None, 65, 0) == 2


# ---- binding ----------------------------------------------------------------------------------------------------------------------
def test_seam_prototypes_equal_the_header(monkeypatch):
    """abi.SEAM_PROTOTYPES against csrc/seam/stac_seam.h with the comparison that test_host.py makes for the main table; the library
    carries them; and the main table, the main header and the build's globs know nothing of the companion."""
    import re

    from stac_mjx_amd import abi, build

    header = hs.CSRC / "seam" / "stac_seam.h"
    monkeypatch.setattr(hs, "HEADER", header)
    protos, n_statements = hs.header_prototypes()
    declared = set(re.findall(r"\b(stac_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header.read_text(), flags=re.S)))
    assert n_statements == len(protos) == 3 and set(protos) == declared and tuple(abi.SEAM_PROTOTYPES) == tuple(protos)
    for name, (ret, args) in protos.items():
        restype, argtypes = abi.SEAM_PROTOTYPES[name]
        assert hs.ctypes_class(restype) == ret, name
        assert [hs.ctypes_class(t) for t in argtypes] == [c for c, _ in args], name
    lib = _seam_lib()
    for name, (restype, argtypes) in abi.SEAM_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name
    assert not set(abi.SEAM_PROTOTYPES) & (set(abi.PROTOTYPES) | set(abi.SELECT_PROTOTYPES) | set(abi.MMASK_PROTOTYPES)) and len(abi.PROTOTYPES) == 39
    assert build.SEAM_LIB.parent == hs.CSRC / "seam" and not any(p.parent == build.SEAM_DIR for p in build.SOURCES + build.HEADERS)
    assert set(build.SEAM_SOURCES) == set(build.SEAM_DIR.glob("*.hip")) and header in build.SEAM_HEADERS
    assert build.SEAM_DIR / "stac_seam.hpp" in build.SEAM_HEADERS
    text = (build.SEAM_DIR / "stac_seam.hpp").read_text()
    from stac_mjx_amd import seam

    assert f"kSeamMaxQuat = {seam.MAX_QUAT};" in text and f"kSeamMaxNq = {seam.MAX_NQ};" in text and "kSeamMaxRows = 1ll << 32;" in text
    assert not build.seam_is_stale() and build.SEAM_STAMP.read_text().strip() == build.seam_digest()


# ---- options, pre-flight, wrappers --------------------------------------------------------------------------------------------------
def test_options_and_the_preflight(rodent_cfg):
    from stac_mjx_amd.config import ConfigError, seam_options
    from stac_mjx_amd.main import _Preflight

    assert seam_options({}) == (1, False) and seam_options({"seam_passes": None, "seam_report": None}) == (1, False)
    assert seam_options({"seam_passes": 8, "seam_report": "on"}) == (8, True) and seam_options({"seam_passes": 2, "seam_report": True}) == (2, True)
    assert seam_options({"seam_report": False}) == (1, False) and seam_options({"seam_report": "off"}) == (1, False)
    for bad in (0, 9, -1, 2.0, "2", True, [2]):
        with pytest.raises(ConfigError, match=r"stac.seam_passes must be an integer in 1 \.\. 8"):
            hs.stage_cfg(rodent_cfg, seam_passes=bad)
    for bad in ("yes", "On", 1, 0, ["on"]):
        with pytest.raises(ConfigError, match="stac.seam_report must be off or on"):
            hs.stage_cfg(rodent_cfg, seam_report=bad)
    pre = _Preflight(hs.stage_cfg(rodent_cfg), 100, "fit.h5")
    pre.check_config()
    assert (pre.seam_passes, pre.seam_report) == (1, False)
    cfg = hs.stage_cfg(rodent_cfg, seam_passes=3, seam_report=True)
    assert cfg.stac.seam_report == "on" and cfg.to_dict()["stac"]["seam_passes"] == 3  # (what a result file stores)
    pre = _Preflight(cfg, 100, "fit.h5")
    pre.check_config()
    assert (pre.seam_passes, pre.seam_report) == (3, True)
    cfg.stac.seam_passes = 12  # (a config that was changed after it was validated: the pre-flight reads the key again)
    with pytest.raises(ValueError, match="stac.seam_passes must be an integer in 1 .. 8"):
        _Preflight(cfg, 100, "fit.h5").check_config()


def test_wrapper_refusals():
    """Engine-free: ik_only checks ``passes`` before any device work"""
    from stac_mjx_amd.stac import Stac

    stub = types.SimpleNamespace(cfg=types.SimpleNamespace(stac={}), engine=None)
    for bad in (0, 9, 1.5, "2", True):
        with pytest.raises(ValueError, match=r"ik_only: passes must be an integer in 1 \.\. 8"):
            Stac.ik_only(stub, np.zeros((4, 6), np.float32), np.zeros((2, 3), np.float32), passes=bad)


def test_summary_helpers():
    from stac_mjx_amd import seam

    assert [seam.kth_rank(pm, n) for pm, n in ((500, 1), (500, 2), (500, 3), (990, 100), (990, 101), (0, 5), (1000, 5))] == [1, 1, 2, 99, 100, 1, 5]
    assert seam.scalar_columns(12, (3,), 3).tolist() == [7, 8, 9, 10, 11] and seam.scalar_columns(5).tolist() == [0, 1, 2, 3, 4]
    assert seam.scalar_columns(12, (8, 0), 0).tolist() == [4, 5, 6, 7]
    np.testing.assert_allclose(seam.rot_degrees([0.0, 1.0, 1.0 - np.cos(np.radians(15.0)), -0.5]), [0.0, 180.0, 30.0, 0.0], atol=1e-9)


# ---- the rank exchange ------------------------------------------------------------------------------------------------------------------
def test_neighbour_rule_of_the_rank_exchange():
    """The clip in front of a rank's first one lives on the nearest earlier rank that owns a clip"""
    from stac_mjx_amd.dist import exchange_seam_rows, seam_neighbour, shard_range

    assert [seam_neighbour([True, True, True], r) for r in range(3)] == [-1, 0, 1]
    assert [seam_neighbour([True, False, False, True], r) for r in range(4)] == [-1, 0, 0, 0]
    assert [seam_neighbour([False, True, False, True, True], r) for r in range(5)] == [-1, -1, 1, 1, 3]
    assert [seam_neighbour([False, False], r) for r in range(2)] == [-1, -1] and seam_neighbour([True], 0) == -1
    # with the shards that shard_range hands out, the neighbour owns the clip lo - 1, for every split, ranks without clips included
    for n_clips in (1, 2, 3, 5, 8):
        for w in (1, 2, 3, 4, 7):
            ranges = [shard_range(n_clips, r, w) for r in range(w)]
            has = [hi > lo for lo, hi in ranges]
            for r, (lo, hi) in enumerate(ranges):
                src = seam_neighbour(has, r)
                if hi > lo and lo > 0:
                    assert src >= 0 and ranges[src][1] == lo, (n_clips, w, r)
                elif hi > lo:
                    assert src == -1
    assert exchange_seam_rows(None, 5, "cpu") is None  # (no process group: nothing to exchange)


# ---- the value of the passes ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def value_runs(rodent_setup, rodent_cfg, rodent_mocap):
    """The golden rodent recording, 1000 rows, offsets of helpers.oracle_fit_offsets(fs, cfg, kp[0:1000:16][:60], 3); per clip length
    F the outputs of 1, 2 and 3 passes by the float32 oracle (seam_cases.oracle_seam_passes)"""
    import helpers
    from oracle import Oracle

    fs, cfgm = rodent_setup, rodent_cfg
    kp = rodent_mocap[:1000].astype(np.float32)
    offsets, _ = helpers.oracle_fit_offsets(fs, cfgm, kp[0:1000:16][:60], 3)
    orc = Oracle(fs.tables, tol=float(cfgm["FTOL"]), maxiter=int(cfgm["N_ITER_Q"]))
    orc.set_site_pos(offsets)
    return {F: sc.oracle_seam_passes(orc, fs, kp.reshape(1000 // F, F, -1), 3) for F in (50, 250)}, kp


@pytest.mark.parametrize("F", (50, 250))
def test_warm_passes_close_the_seams(value_runs, rodent_setup, F):
    """Two passes against one: a lower mean marker error, a mean seam jump below half, a lower error of the first 5 frames of the
    clips 1 ..; three passes are not worse than two in mean seam jump (the design measured the jump ratios 0.19 at F = 50 and 0.08
    at F = 250: DESIGN.md "Warm-started clips and pose steps")"""
    import helpers
    from stac_mjx_amd import seam

    runs, kp = value_runs
    outs = runs[F]
    scalar = seam.scalar_columns(rodent_setup.tables.nq, (3,), 3)
    kp_clips = kp.reshape(1000 // F, F, -1)
    err = [helpers.marker_error_mm(o["marker_sites"], kp_clips) for o in outs]
    head = [helpers.marker_error_mm(o["marker_sites"][1:, :5], kp_clips[1:, :5]) for o in outs]
    jump = [float(sc.seam_jumps(o["qpos"], scalar).mean()) for o in outs]
    print(f"F = {F}: mean marker error {err} mm, first 5 frames of clips 1.. {head} mm, mean seam jump {jump} rad (1, 2, 3 passes)")
    assert np.array_equal(outs[1]["qpos"][0], outs[0]["qpos"][0]) and not np.array_equal(outs[1]["qpos"][1], outs[0]["qpos"][1])
    assert err[1] < err[0], err
    assert jump[1] < 0.5 * jump[0], jump
    assert head[1] < head[0], head
    assert jump[2] <= jump[1], jump
