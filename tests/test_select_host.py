"""Choosing calibration frames (stac.fit_frames), host side: the rule of csrc/select/stac_select.hpp, built for the CPU, against the
numpy float64 judge of tests/select_cases.py; ``select_strided``; every refusal of the pre-flight and of the two entry points that
needs no device; the binding table against csrc/select/stac_select.h; and the accuracy claim of DESIGN.md "Choosing calibration
frames", pinned with the oracle."""

import json
import types

import numpy as np
import pytest

import host_scaffold as hs
import select_cases as sc


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return sc.cpu_rule(tmp_path_factory)


@pytest.fixture(scope="module")
def recordings():
    kp = sc.golden_rodent()
    rest, rows = sc.resting(kp)
    for a in (kp, rest, rows):
        a.setflags(write=False)
    return kp, rest, rows


# ---- the rule against the float64 judge ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", sc.KS)
def test_rule_holds_the_judges_properties(rule, K):
    for T in sc.TS:
        for label, kp, cand, n in sc.shape_cases(K, T):
            sc.judge(kp, cand, n, *rule[0](kp, cand, n), label=label)


def test_rule_on_the_edges(rule):
    got = {}
    for label, kp, cand, n in sc.edge_cases():
        got[label] = rule[0](kp, cand, n)
        sc.judge(kp, cand, n, *got[label], label=label)
    assert got["all_candidates_T65"][2] == 65 and sorted(got["all_candidates_T65"][0]) == list(range(65))
    sel, _, n_sel = got["all_sparse_candidates_T65"]
    assert n_sel == sel.size and set(sel.tolist()) == {t for t in range(65) if t % 3}
    assert got["missing_first_last_block"][0][0] == 1  # frame 0 has a NaN: the first pick moves
    assert not set(got["missing_first_last_block"][0].tolist()) & ({0, 3, 599} | set(range(590, 597)))
    sel, r2, n_sel = got["ties_across_block_borders"]
    assert n_sel == 30 and sel[1] == 255 and 256 not in sel and 512 not in sel  # the lower index of two equal farthest frames
    assert not ({63, 64, 511} <= set(sel.tolist())) and len({63, 64, 511} & set(sel.tolist())) <= 1
    assert got["all_equal"][2] == 1 and got["all_equal"][0][0] == 0
    assert got["five_distinct"][2] == 5 and sorted(got["five_distinct"][0][:5]) == [0, 1, 2, 3, 4]
    assert got["no_candidate"][2] == 0 and got["none_allowed"][2] == 0


def test_rule_smallest_shapes(rule):
    """K = 2 (one distance), T = 1, n = 1, and a cand that excludes index 0"""
    kp = sc.series(9, 2, 11)
    sel, r2, n_sel = rule[0](kp, None, 9)
    d = sc.descriptors64(kp)[:, 0]
    assert n_sel == 9 and sel[0] == 0 and sel[1] == int(np.argmax(np.abs(d - d[0])))
    sel, r2, n_sel = rule[0](kp[:1], None, 1)
    assert (sel.tolist(), n_sel) == ([0], 1) and np.isposinf(r2[0])
    cand = np.ones(9, np.uint8)
    cand[0] = 0
    sel, r2, n_sel = rule[0](kp, cand, 1)
    assert (sel.tolist(), n_sel) == ([1], 1)


@pytest.mark.parametrize("n", [30, 100])
def test_rule_equals_float64_greedy_on_the_recordings(rule, recordings, n):
    kp, rest, rows = recordings
    for name, x in (("golden", kp), ("resting", rest)):
        sel, r2, n_sel = rule[0](x, None, n)
        assert n_sel == n and sel.tolist() == sc.greedy64(x, None, n), name
        sc.judge(x, None, n, sel, r2, n_sel, label=name)
    moving = int(np.count_nonzero(sel >= 880))  # (of the resting recording: measured 26 of 30 and 87 of 100)
    print(f"resting recording, n = {n}: {moving} picks in the 120 moving frames")
    assert moving >= {30: 24, 100: 80}[n]


def test_rule_stops_at_the_distinct_rows(rule, recordings):
    _, rest, rows = recordings
    sel, r2, n_sel = rule[0](rest, None, 1000)
    assert n_sel == 160 == np.unique(rows).size
    assert np.unique(rows[sel[:160]]).size == 160 and (sel[160:] == -1).all() and np.isnan(r2[160:]).all()
    # of equal frames the lowest index is picked
    first = {int(r): int(np.flatnonzero(rows == r)[0]) for r in np.unique(rows)}
    assert sorted(sel[:160].tolist()) == sorted(first.values())


# ---- select_strided ---------------------------------------------------------------------------------------------------------------
def test_select_strided():
    from stac_mjx_amd.select import select_strided

    assert select_strided(10, 3).tolist() == [0, 3, 6] and select_strided(10, 10).tolist() == list(range(10))
    assert select_strided(1000, 30).tolist() == [(i * 1000) // 30 for i in range(30)] and select_strided(7, 1).tolist() == [0]
    cand = np.array([0, 1, 1, 0, 1, 1, 1, 0, 0, 1])
    assert select_strided(10, 3, cand).tolist() == [1, 4, 6] and select_strided(10, 6, cand).tolist() == [1, 2, 4, 5, 6, 9]
    assert select_strided(10, 3, cand).dtype == np.int64
    for bad in (lambda: select_strided(10, 7, cand), lambda: select_strided(10, 11), lambda: select_strided(10, 0), lambda: select_strided(0, 1),
                lambda: select_strided(10, 3, cand[:9]), lambda: select_strided(10, 2.0)):
        with pytest.raises(ValueError):
            bad()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _select_lib():
    from stac_mjx_amd.build import build_extension
    from stac_mjx_amd.engine import load_select_library

    build_extension()
    return load_select_library()


def _refused(lib, rc, code):
    msg = lib.stac_select_last_error().decode()
    assert rc == code and lib.stac_select_last_error_code() == code and msg, (rc, code, msg)
    return msg


def test_workspace_function_and_its_refusals(rule):
    from stac_mjx_amd import select

    lib = _select_lib()
    for T, K in ((1, 2), (63, 3), (64, 3), (65, 23), (1000, 23), (16643, 23), (10**6, 23), (2**32 - 1, 64)):
        got = lib.stac_select_workspace(T, K)
        P, stride = K * (K - 1) // 2, (T + 63) // 64 * 64
        assert got == rule[1].select_bytes(T, K) == select.workspace_bytes(T, K) and got % 8 == 0
        assert got >= 4 * P * stride + 5 * T + 8 * 1024 + 4 * P + 8  # every array of the layout has its room
    for T, K, code in ((0, 3, hs.STAC_ERR_INVALID), (-1, 3, hs.STAC_ERR_INVALID), (10, 1, hs.STAC_ERR_INVALID), (10, 0, hs.STAC_ERR_INVALID),
                       (10, 65, hs.STAC_ERR_CAPACITY), (2**32, 3, hs.STAC_ERR_CAPACITY)):
        _refused(lib, lib.stac_select_workspace(T, K), code)
    with pytest.raises(select.StacHipError, match="n_kp"):
        select.workspace_bytes(10, 65)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Every refusal of stac_select_diverse comes before the device is touched: made-up addresses do on a machine without a GPU"""
    lib = _select_lib()
    T, K, n = 100, 3, 10
    need = lib.stac_select_workspace(T, K)
    base = 1 << 20
    good = dict(kp=base, T=T, K=K, cand=None, n=n, sel=base + (1 << 16), radius2=base + (2 << 16), n_selected=base + (3 << 16),
                work=base + (4 << 16), nbytes=need)

    def call(**over):
        a = dict(good)
        a.update(over)
        return lib.stac_select_diverse(a["kp"], a["T"], a["K"], a["cand"], a["n"], a["sel"], a["radius2"], a["n_selected"], a["work"],
                                       a["nbytes"], None)

    inv, cap = hs.STAC_ERR_INVALID, hs.STAC_ERR_CAPACITY
    for over, code, word in (
            (dict(T=0), inv, "n_frames"), (dict(K=1), inv, "n_kp"), (dict(K=65), cap, "n_kp"), (dict(T=2**32, n=1), cap, "2^32"),
            (dict(n=0), inv, "n_select"), (dict(n=T + 1), inv, "n_select"), (dict(kp=None), inv, "null"), (dict(sel=None), inv, "null"),
            (dict(radius2=None), inv, "null"), (dict(n_selected=None), inv, "null"), (dict(work=None), inv, "null"),
            (dict(nbytes=need - 1), inv, "workspace_bytes"), (dict(kp=base + 2), inv, "kp must be 4-byte aligned"),
            (dict(sel=good["sel"] + 4), inv, "sel must be 8-byte aligned"), (dict(radius2=good["radius2"] + 1), inv, "radius2 must be 4-byte"),
            (dict(n_selected=good["n_selected"] + 4), inv, "n_selected must be 8-byte"), (dict(work=good["work"] + 4), inv, "workspace must be 8-byte"),
            (dict(sel=base + 8), inv, "kp and sel overlap"), (dict(cand=base + 12 * T * K - 1), inv, "kp and cand overlap"),
            (dict(radius2=good["sel"] + 8 * n - 4), inv, "sel and radius2 overlap"), (dict(n_selected=good["sel"]), inv, "sel and n_selected overlap"),
            (dict(work=good["n_selected"] - need + 8), inv, "n_selected and workspace overlap"),
            (dict(cand=good["work"] + need - 1), inv, "cand and workspace overlap")):
        assert word in _refused(lib, call(**over), code), over


def test_wrapper_and_config_refusals(rodent_cfg):
    import torch

    from stac_mjx_amd import select
    from stac_mjx_amd.config import ConfigError, fit_frames_options
    from stac_mjx_amd.main import _Preflight

    with pytest.raises(ValueError, match="CUDA tensor"):
        select.select_diverse(torch.zeros(10, 9), 3)
    with pytest.raises(ValueError, match="CUDA tensor"):
        select.select_diverse(np.zeros((10, 9), np.float32), 3)
    assert fit_frames_options({}) == "first" and fit_frames_options({"fit_frames": None}) == "first"
    assert [fit_frames_options({"fit_frames": m}) for m in select.MODES] == list(select.MODES)
    for bad in ("random", "Diverse", True, 3, ["diverse"]):
        with pytest.raises(ConfigError, match="stac.fit_frames must be first, strided or diverse"):
            hs.stage_cfg(rodent_cfg, fit_frames=bad)
    # the pre-flight: more fit frames than the recording has, before a Stac is built (first keeps today's slice)
    for mode in ("strided", "diverse"):
        pre = _Preflight(hs.stage_cfg(rodent_cfg, fit_frames=mode, n_fit_frames=101), 100, "fit.h5")
        with pytest.raises(ValueError, match="n_fit_frames = 101 exceeds the 100 frames"):
            pre.check_config()
        with pytest.raises(ValueError, match="n_fit_frames must be at least 1"):
            _Preflight(hs.stage_cfg(rodent_cfg, fit_frames=mode, n_fit_frames=0), 100, "fit.h5").check_config()
        pre = _Preflight(hs.stage_cfg(rodent_cfg, fit_frames=mode, n_fit_frames=100), 100, "fit.h5")
        pre.check_config()
        assert pre.fit_frames == mode
        _Preflight(hs.stage_cfg(rodent_cfg, fit_frames=mode, n_fit_frames=101, skip_fit_offsets=True), 100, "fit.h5").check_config()  # (no fit)
    for cfg in (hs.stage_cfg(rodent_cfg, n_fit_frames=101), hs.stage_cfg(rodent_cfg, fit_frames="first", n_fit_frames=101)):
        pre = _Preflight(cfg, 100, "fit.h5")
        pre.check_config()
        assert pre.fit_frames == "first"


# ---- run_stac's selection on the host (strided needs no device) ----------------------------------------------------------------------
def test_fit_frames_pass_over_marked_frames(rodent_cfg, tmp_path, capsys):
    from stac_mjx_amd.main import _select_fit_frames, _Series, _write_frames, frames_path
    from stac_mjx_amd.stac import Stac

    T, K = 50, 23
    kp = sc.series(T, K, 21)
    gap, swapped = np.zeros((T, K), np.int32), np.zeros((T, K), np.uint8)
    gap[0:10, 3] = 10
    swapped[20, [1, 2]] = 1
    series = _Series(kp, {"kp_gap": gap, "kp_swapped": swapped})
    stub = types.SimpleNamespace(_kp_names=[f"k{i}" for i in range(K)], _log=print)
    stub.select_frames = types.MethodType(Stac.select_frames, stub)
    usable = [t for t in range(10, T) if t != 20]
    rows, info = _select_fit_frames(stub, hs.stage_cfg(rodent_cfg, fit_frames="strided", n_fit_frames=13), series, "strided")
    assert rows.tolist() == [usable[(i * 39) // 13] for i in range(13)] and info["mode"] == "strided" and info["n_selected"] == 13
    assert info["order"].tolist() == rows.tolist() and info["radius2"].size == 0
    assert "select_frames (strided): 13 of 50 frames; picks per tenth of the recording: 0 0 " in capsys.readouterr().out
    with pytest.raises(ValueError, match="n_fit_frames = 40, but only 39 of the 50 frames"):
        _select_fit_frames(stub, hs.stage_cfg(rodent_cfg, fit_frames="strided", n_fit_frames=40), series, "strided")
    # first through the method: the first candidates; and the refusals of the method itself
    rows1, info1 = stub.select_frames(kp, 4, "first", exclude=(gap != 0).any(axis=1))
    assert rows1.tolist() == [10, 11, 12, 13] and info1["n_selected"] == 4
    for bad in (lambda: stub.select_frames(kp, 4, "random"), lambda: stub.select_frames(kp[:, :66], 4, "strided"),
                lambda: stub.select_frames(kp, 0, "strided"), lambda: stub.select_frames(kp, 4, "strided", exclude=np.zeros(T - 1)),
                lambda: stub.select_frames(kp, T + 1, "first")):
        with pytest.raises(ValueError):
            bad()
    # the index form of attach, and the sidecar
    data = types.SimpleNamespace()
    series.attach_rows(data, rows)
    np.testing.assert_array_equal(data.kp_gap, gap[rows])
    np.testing.assert_array_equal(data.kp_swapped, swapped[rows])
    path = _write_frames(tmp_path / "fit.npz", rows, {"mode": "diverse", "order": rows[::-1], "radius2": np.array([np.inf, 2.5], np.float32)})
    assert path == frames_path(tmp_path / "fit.npz") and path.name == "fit.npz.frames.json"
    assert json.loads(path.read_text()) == {"mode": "diverse", "indices": rows.tolist(), "order": rows[::-1].tolist(), "radius2": [None, 2.5]}


# ---- binding ----------------------------------------------------------------------------------------------------------------------
def test_select_prototypes_equal_the_header(monkeypatch):
    """abi.SELECT_PROTOTYPES against csrc/select/stac_select.h with the comparison that test_host.py makes for the main table: the
    same names in the same order, the same number of arguments, every argument and return value of the same class; the library
    carries them; and the main table, the main header and the build's globs know nothing of the companion."""
    import re

    from stac_mjx_amd import abi, build

    header = hs.CSRC / "select" / "stac_select.h"
    monkeypatch.setattr(hs, "HEADER", header)
    protos, n_statements = hs.header_prototypes()
    declared = set(re.findall(r"\b(stac_[a-z0-9_]+)\s*\(", header.read_text()))
    assert n_statements == len(protos) == 4 and set(protos) == declared and tuple(abi.SELECT_PROTOTYPES) == tuple(protos)
    for name, (ret, args) in protos.items():
        restype, argtypes = abi.SELECT_PROTOTYPES[name]
        assert hs.ctypes_class(restype) == ret, name
        assert [hs.ctypes_class(t) for t in argtypes] == [c for c, _ in args], name
    lib = _select_lib()
    for name, (restype, argtypes) in abi.SELECT_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name
    assert not set(abi.SELECT_PROTOTYPES) & set(abi.PROTOTYPES) and len(abi.PROTOTYPES) == 39
    assert build.SELECT_LIB.parent == hs.CSRC / "select" and not any(p.parent == build.SELECT_DIR for p in build.SOURCES + build.HEADERS)
    assert set(build.SELECT_SOURCES) == set(build.SELECT_DIR.glob("*.hip")) and header in build.SELECT_HEADERS
    assert build.SELECT_DIR / "stac_select.hpp" in build.SELECT_HEADERS
    text = (build.SELECT_DIR / "stac_select.hpp").read_text()  # the capacities Python states are the kernel's
    from stac_mjx_amd import select

    assert "kSelectMaxKp = kPairwiseMaxKp;" in text and select.MAX_KP == 64 and "kSelectMaxFrames = 0xFFFFFFFFll;" in text
    assert select.MAX_FRAMES == 0xFFFFFFFF
    assert not build.select_is_stale() and build.SELECT_STAMP.read_text().strip() == build.select_digest()


# ---- the accuracy claim -----------------------------------------------------------------------------------------------------------
def test_diverse_frames_calibrate_better_on_a_resting_recording(rule, recordings, rodent_setup, rodent_cfg):
    """Offsets fitted by the float32 oracle (N_ITERS = 6 from the model's initial offsets) on 30 frames of the resting recording, scored
    by the mean marker-to-keypoint distance of a 4 x 250 ik_clips run over the ORIGINAL 1000 frames: diverse < strided < first and
    diverse <= 0.8 first (measured when the stage was designed: 1.707 / 2.213 / 2.656 mm)."""
    from helpers import marker_error_mm, oracle_fit_offsets
    from oracle import Oracle
    from stac_mjx_amd.select import select_strided

    kp, rest, _ = recordings
    fs, n = rodent_setup, 30
    sel, _, n_sel = rule[0](rest, None, n)
    assert n_sel == n
    chosen = {"first": np.arange(n), "strided": select_strided(1000, n), "diverse": np.sort(sel)}
    err = {}
    for mode, rows in chosen.items():
        offsets, _ = oracle_fit_offsets(fs, rodent_cfg, np.ascontiguousarray(rest[rows]), 6)
        orc = Oracle(fs.tables, tol=float(rodent_cfg["FTOL"]), maxiter=int(rodent_cfg["N_ITER_Q"]))
        orc.set_site_pos(offsets)
        out = orc.ik_clips(np.ascontiguousarray(kp.reshape(4, 250, -1)), fs.lb, fs.ub, fs.part_masks, fs.trunk_kps, fs.root_kp_idx, fs.root_dims)
        err[mode] = marker_error_mm(out["marker_sites"], kp)
    print("mean marker error over the original 1000 frames, mm:", {k: round(v, 4) for k, v in err.items()})
    assert err["diverse"] < err["strided"] < err["first"] and err["diverse"] <= 0.8 * err["first"], err
