"""Ground clearance (stac.ground), host side: the rule of csrc/ground/stac_ground.hpp, built for the CPU, against the numpy float32
judge of tests/ground_cases.py at tolerance 0; values that are not finite; every refusal of the entry point, which needs no device; the
binding table against csrc/ground/stac_ground.h; the options and the pre-flight; the table of the rodent; the sidecar and the levelled
result file; and the finding on the reference's stored fit, pinned with the CPU rule (DESIGN.md "Ground clearance")."""

import json
import types

import numpy as np
import pytest

import ground_cases as gc
import host_scaffold as hs


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return gc.cpu_rule(tmp_path_factory)


# ---- the rule against the judge ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbody", gc.NBODIES)
def test_rule_equals_the_judge(rule, nbody):
    clearance, _ = rule
    cases = gc.cases(nbody)
    assert {(c[1].shape[0], c[3].shape[0]) for c in cases} == {(N, G) for N in gc.NS for G in gc.GS}
    for label, *args in cases:
        gc.same(clearance(*args), gc.judge(*args), label)


def test_rule_equals_the_judge_on_the_special_cases(rule):
    clearance, _ = rule
    seen = {}
    for label, *args in gc.special_cases():
        got = clearance(*args)
        gc.same(got, gc.judge(*args), label)
        seen[label] = (got, args)
    assert set(seen) == {"twins", "nothing_included", "slots0", "slots1", "slots32", "meshes_own", "meshes_shared", "z_ref_hit"}
    got, _ = seen["twins"]  # two identical included geoms, 3 and 7: the smaller index wins in every frame
    assert (got["low_geom"] == 3).all() and np.array_equal(gc.bits(got["geom_min"][3]), gc.bits(got["geom_min"][7]))
    got, args = seen["nothing_included"]
    assert (got["low_geom"] == -1).all() and np.isposinf(got["low_z"]).all() and np.isfinite(got["track_z"]).all()
    assert np.isfinite(got["geom_min"]).all()  # (the per-geom outputs do not ask whether a geom is included)
    assert seen["slots0"][0]["track_z"].shape == (70, 0) and seen["slots32"][0]["track_z"].shape == (70, 32)
    got, args = seen["slots1"]
    meta = args[2]
    assert (meta[meta[:, 3] == 0, 2] == 0).any()  # (the slot holds a geom that is not included)
    assert np.array_equal(seen["meshes_own"][1][2][:, 5], seen["meshes_shared"][1][2][:, 5])
    assert len(seen["meshes_own"][1][4]) == 6 * 1193 and len(seen["meshes_shared"][1][4]) == 1193  # (1 + 63 + 64 + 65 + 1000 vertices)
    got, args = seen["z_ref_hit"]  # z_ref is the lowest z of frame 0: strictly below means that geom does not count frame 0
    z = gc.judge_z(*args[:5])
    g = int(z[0].argmin())
    assert z[0, g] == np.float32(args[6]) and got["geom_below"][g] == int((z[:, g] < np.float32(args[6])).sum())
    assert got["geom_below"][g] < int((z[:, g] <= np.float32(args[6])).sum())


def test_the_cases_cover_what_they_claim():
    """Every type in every table of six geoms or more, exact zeros and +-1 in the aligned cases, ties in the quantised ones"""
    labels = [c[0] for nb in gc.NBODIES for c in gc.cases(nb)]
    assert len(labels) == len(set(labels)) == 90 and sum("aligned" in lab for lab in labels) >= 20
    for S in (0, 1, 2, 32):
        assert any(f"_S{S}_" in lab for lab in labels), S
    for label, xpos, xquat, meta, data, verts, S, z_ref in gc.cases(5):
        if meta.shape[0] >= 6:
            assert set(meta[:, 0]) == set(gc.TYPES), label
        if "aligned" in label:
            w, x, y, z = (xquat[..., i] for i in range(4))
            assert set(np.unique(2 * (x * z - w * y))) <= {0.0} and set(np.unique(1 - 2 * (x * x + y * y))) <= {-1.0, 1.0}
            assert set(np.unique(data[:, 6:])) <= {-1.0, 0.0, 1.0}
    _, xpos, xquat, meta, data, verts, S, z_ref = next(c for c in gc.cases(5) if c[0].startswith("N130_G101_") and "aligned" in c[0])
    z = gc.judge_z(xpos, xquat, meta, data, verts)
    inc = meta[:, 2] != 0
    assert ((z[:, inc] == z[:, inc].min(axis=1, keepdims=True)).sum(axis=1) > 1).any()  # (two included geoms tie for the lowest)


@pytest.mark.parametrize("value,where,body", gc.POISONS)
def test_values_that_are_not_finite(rule, value, where, body):
    """A NaN or an infinity in a body's frame: the quiet NaN in low_z (and -1) where the body carries included geoms, in the slot's
    track_z where it carries tracked ones, the geom's own frame skipped in geom_min / geom_below, and nothing else"""
    clearance, _ = rule
    label, xpos, xquat, meta, data, verts, S, z_ref = gc.poisoned(value, where, body)
    got = clearance(xpos, xquat, meta, data, verts, S, z_ref)
    gc.same(got, gc.judge(xpos, xquat, meta, data, verts, S, z_ref), label)
    rows = np.flatnonzero(~np.isfinite(xpos).all(axis=(1, 2)) | ~np.isfinite(xquat).all(axis=(1, 2)))
    assert rows.tolist() == [1, 70]
    cp, cq = np.where(np.isfinite(xpos), xpos, np.float32(0.25)), np.where(np.isfinite(xquat), xquat, np.float32(0.25))
    ref = clearance(cp, cq, meta, data, verts, S, z_ref)
    keep = np.ones(xpos.shape[0], bool)
    keep[rows] = False
    for k in ("low_z", "low_geom", "track_z"):
        assert np.array_equal(gc.bits(got[k][keep]), gc.bits(ref[k][keep])), (label, k)
    if body == "included":
        assert (gc.bits(got["low_z"][rows]) == 0x7FC00000).all() and (got["low_geom"][rows] == -1).all()
        assert (gc.bits(got["track_z"][rows, 0]) == 0x7FC00000).all() and np.array_equal(gc.bits(got["track_z"][rows, 1]), gc.bits(ref["track_z"][rows, 1]))
    else:
        assert np.array_equal(gc.bits(got["low_z"]), gc.bits(ref["low_z"])) and np.array_equal(got["low_geom"], ref["low_geom"])
        assert np.array_equal(gc.bits(got["track_z"][:, 0]), gc.bits(ref["track_z"][:, 0]))
        if body == "tracked":
            assert (gc.bits(got["track_z"][rows, 1]) == 0x7FC00000).all()
        else:
            assert np.array_equal(gc.bits(got["track_z"]), gc.bits(ref["track_z"]))
    assert np.isfinite(got["geom_min"]).all() and (got["geom_below"] >= 0).all()
    hit = meta[:, 1] == {"included": 1, "tracked": 2, "untouched": 4}[body]
    assert np.array_equal(gc.bits(got["geom_min"][~hit]), gc.bits(ref["geom_min"][~hit])) and np.array_equal(got["geom_below"][~hit], ref["geom_below"][~hit])
    z = gc.judge_z(xpos, xquat, meta, data, verts)
    assert not np.isfinite(z[rows][:, hit]).any() and (got["geom_below"][hit] <= xpos.shape[0] - 2).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _ground_lib():
    from stac_mjx_amd.build import build_extension
    from stac_mjx_amd.engine import load_ground_library

    build_extension()
    return load_ground_library()


def _refused(lib, rc, code):
    msg = lib.stac_ground_last_error().decode()
    assert rc == code and lib.stac_ground_last_error_code() == code and msg, (rc, code, msg)
    return msg


def test_entry_point_refuses_bad_arguments_before_any_launch(rule):
    """Every refusal comes before the device is touched: made-up addresses do on a machine without a GPU"""
    import ctypes as C

    lib = _ground_lib()
    N, nbody, G, S, V = 100, 5, 3, 2, 10
    base, step = 1 << 24, 1 << 16
    names = ("xpos", "xquat", "meta", "data", "verts", "low_z", "low_geom", "track_z", "geom_min", "geom_below")
    good = dict(N=N, nbody=nbody, G=G, S=S, V=V, z_ref=0.0, rows=[[2, 1, 1, 0, 0, 0], [7, 4, 0, -1, 2, 8], [6, 2, 1, 1, 0, 0]],
                **{n: base + i * step for i, n in enumerate(names)})

    def call(**over):
        a = dict(good)
        a.update(over)
        host = None if a["rows"] is None else (C.c_int32 * (6 * len(a["rows"])))(*[v for r in a["rows"] for v in r])
        return lib.stac_ground_clearance(a["xpos"], a["xquat"], a["N"], a["nbody"], host, a["meta"], a["data"], a["G"], a["verts"], a["V"], a["S"],
                                         a["z_ref"], a["low_z"], a["low_geom"], a["track_z"], a["geom_min"], a["geom_below"], None)

    def row(i, col, v):
        rows = [list(r) for r in good["rows"]]
        rows[i][col] = v
        return dict(rows=rows)

    inv, cap = hs.STAC_ERR_INVALID, hs.STAC_ERR_CAPACITY
    many = [[2, 1, 1, -1, 0, 0]] * 4097
    for over, code, word in (
            (dict(N=0), inv, "n_frames"), (dict(N=-3), inv, "n_frames"), (dict(N=2**40 + 1), inv, "n_frames"), (dict(nbody=1), inv, "nbody >= 2"),
            (dict(nbody=0), inv, "nbody >= 2"), (dict(nbody=4097), cap, "nbody = 4097"), (dict(G=0), inv, "n_geoms >= 1"), (dict(G=-1), inv, "n_geoms >= 1"),
            (dict(G=4097, rows=many), cap, "n_geoms = 4097"), (dict(V=-1), inv, "n_verts >= 0"), (dict(V=2**20 + 1), cap, "n_verts = 1048577"),
            (dict(S=-1), inv, "n_slots = -1"), (dict(S=33), inv, "n_slots = 33"), (dict(rows=None), inv, "null geom_meta_host"),
            (row(0, 0, 1), inv, "geom 0: unknown type 1"), (row(2, 0, 8), inv, "geom 2: unknown type 8"), (row(0, 0, 0), inv, "unknown type 0"),
            (row(1, 1, 0), inv, "geom 1: body 0 is outside"), (row(1, 1, 5), inv, "body 5 is outside"), (row(1, 1, -1), inv, "body -1 is outside"),
            (row(0, 2, 2), inv, "include must be 0 or 1"), (row(0, 2, -1), inv, "include must be 0 or 1"), (row(0, 3, 2), inv, "slot 2 is outside"),
            (row(0, 3, -2), inv, "slot -2 is outside"), (dict(S=0), inv, "slot 0 is outside"), (row(1, 5, 0), inv, "mesh range 2 + 0 is empty"),
            (row(1, 5, 9), inv, "mesh range 2 + 9"), (row(1, 4, -1), inv, "mesh range -1 + 8"), (dict(V=0), inv, "outside the 0 vertices"),
            (row(1, 4, 2**31 - 1), inv, "mesh range"),
            *[(dict(**{n: None}), inv, f"null {'geom_' + n if n in ('meta', 'data') else n}") for n in names],
            (dict(xpos=base + 2), inv, "xpos must be 4-byte"), (dict(xquat=good["xquat"] + 4), inv, "xquat must be 16-byte"),
            (dict(xquat=good["xquat"] + 8), inv, "xquat must be 16-byte"), (dict(meta=good["meta"] + 1), inv, "geom_meta must be 4-byte"),
            (dict(data=good["data"] + 2), inv, "geom_data must be 4-byte"), (dict(verts=good["verts"] + 3), inv, "verts must be 4-byte"),
            (dict(low_z=good["low_z"] + 1), inv, "low_z must be 4-byte"), (dict(low_geom=good["low_geom"] + 2), inv, "low_geom must be 4-byte"),
            (dict(track_z=good["track_z"] + 2), inv, "track_z must be 4-byte"), (dict(geom_min=good["geom_min"] + 2), inv, "geom_min must be 4-byte"),
            (dict(geom_below=good["geom_below"] + 4), inv, "geom_below must be 8-byte"),
            (dict(xquat=base + 12 * N * nbody - 16), inv, "xpos and xquat overlap"), (dict(low_z=good["xquat"] + 16 * N * nbody - 4), inv, "xquat and low_z overlap"),
            (dict(low_geom=good["low_z"]), inv, "low_z and low_geom overlap"), (dict(track_z=good["low_geom"] + 4 * N - 4), inv, "low_geom and track_z overlap"),
            (dict(geom_min=good["track_z"] + 4 * N * S - 4), inv, "geom_min and track_z overlap"), (dict(geom_below=good["geom_min"] + 8), inv, "geom_min and geom_below overlap"),
            (dict(geom_below=good["data"] + 56), inv, "geom_data and geom_below overlap"), (dict(low_z=good["meta"] + 4), inv, "geom_meta and low_z overlap"),
            (dict(geom_min=good["verts"] + 116), inv, "geom_min and verts overlap"), (dict(low_z=base + 16), inv, "xpos and low_z overlap")):
        assert word in _refused(lib, call(**over), code), over
    # without slots and without meshes the two buffers are not looked at
    spheres = [[2, 1, 1, -1, 0, 0]] * 3
    assert "null low_z" in _refused(lib, call(S=0, V=0, rows=spheres, track_z=None, verts=None, low_z=None), inv)
    # the row check is the header's, whichever side asks
    _, cpu = rule
    arr = lambda *c: np.array(c, np.int32).ctypes.data  # noqa: E731
    assert cpu.ground_check(arr(2, 1, 1, 0, 0, 0), 5, 2, 10) == 0 and cpu.ground_check(arr(7, 4, 0, -1, 2, 8), 5, 2, 10) == 0
    assert [cpu.ground_check(arr(*r), 5, 2, 10) for r in ((1, 1, 1, 0, 0, 0), (2, 5, 1, 0, 0, 0), (2, 1, 3, 0, 0, 0), (2, 1, 1, 2, 0, 0), (7, 1, 1, 0, 3, 8))] == [1, 2, 3, 4, 5]
    assert [cpu.ground_tiles(n) for n in (1, 64, 65, 262144, 262145, 524288, 524289, 10**6, 10**7)] == [1, 1, 1, 1, 2, 2, 3, 4, 39]


# ---- binding ----------------------------------------------------------------------------------------------------------------------
def test_ground_prototypes_equal_the_header(monkeypatch):
    """abi.GROUND_PROTOTYPES against csrc/ground/stac_ground.h with the comparison that test_host.py makes for the main table; the
    library carries them; and the main table, the main header and the build's globs know nothing of the companion."""
    import re

    from stac_mjx_amd import abi, build, ground

    header = hs.CSRC / "ground" / "stac_ground.h"
    monkeypatch.setattr(hs, "HEADER", header)
    protos, n_statements = hs.header_prototypes()
    declared = set(re.findall(r"\b(stac_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header.read_text(), flags=re.S)))
    assert n_statements == len(protos) == 3 and set(protos) == declared and tuple(abi.GROUND_PROTOTYPES) == tuple(protos)
    for name, (ret, args) in protos.items():
        restype, argtypes = abi.GROUND_PROTOTYPES[name]
        assert hs.ctypes_class(restype) == ret, name
        assert [hs.ctypes_class(t) for t in argtypes] == [c for c, _ in args], name
    lib = _ground_lib()
    for name, (restype, argtypes) in abi.GROUND_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name
    others = set(abi.PROTOTYPES) | set(abi.SELECT_PROTOTYPES) | set(abi.MMASK_PROTOTYPES) | set(abi.SEAM_PROTOTYPES)
    assert not set(abi.GROUND_PROTOTYPES) & others and len(abi.PROTOTYPES) == 39
    assert build.GROUND_LIB.parent == hs.CSRC / "ground" and not any(p.parent == build.GROUND_DIR for p in build.SOURCES + build.HEADERS)
    assert set(build.GROUND_SOURCES) == set(build.GROUND_DIR.glob("*.hip")) and header in build.GROUND_HEADERS
    assert build.GROUND_DIR / "stac_ground.hpp" in build.GROUND_HEADERS
    text = (build.GROUND_DIR / "stac_ground.hpp").read_text()
    assert f"kGroundMaxGeoms = {ground.MAX_GEOMS};" in text and f"kGroundMaxBodies = {ground.MAX_BODIES};" in text
    assert "kGroundMaxVerts = 1 << 20;" in text and ground.MAX_VERTS == 1 << 20 and f"kGroundMaxSlots = {ground.MAX_SLOTS};" in text
    assert not build.ground_is_stale() and build.GROUND_STAMP.read_text().strip() == build.ground_digest()


# ---- options, pre-flight -----------------------------------------------------------------------------------------------------------
def test_options_and_the_preflight(rodent_cfg, rodent_setup, fly_setup):
    from stac_mjx_amd.config import ConfigError, ground_options
    from stac_mjx_amd.main import GROUND_LEVEL_FIXED_ROOT, _Preflight, check_ground_level

    default = dict(mode="off", geoms="fitted", geom_groups=None, track=[], z_ref=0.0, permille=50, contact=0.002)
    assert ground_options({}) == default and ground_options({k: None for k in ("ground", "ground_geoms", "ground_track", "ground_z")}) == default
    assert ground_options({"ground": False}) == default
    opt = ground_options({"ground": "level", "ground_geoms": ["foot_L", "torso"], "ground_geom_groups": [0, 2], "ground_track": ["foot_L", "foot_R"],
                          "ground_z": -0.01, "ground_permille": 1000, "ground_contact": 0})
    assert opt == dict(mode="level", geoms=["foot_L", "torso"], geom_groups=[0, 2], track=["foot_L", "foot_R"], z_ref=-0.01, permille=1000, contact=0.0)
    assert ground_options({"ground": "report", "ground_geoms": "all"})["geoms"] == "all"
    for key, bads, text in (
            ("ground", ("on", True, 1, "Level", ["report"]), "stac.ground must be off, report or level"),
            ("ground_geoms", ("some", [], [1], ["a", ""], 3, True), "stac.ground_geoms must be"),
            ("ground_geom_groups", ([], "0", [0.5], [-1], [True], 2), "stac.ground_geom_groups must be a list of geom groups"),
            ("ground_track", ("foot_L", [1], ["a", "a"], [f"b{i}" for i in range(33)], 5), "stac.ground_track must be a list of"),
            ("ground_z", ("0", True, float("nan"), float("inf"), [0]), "stac.ground_z must be a finite number"),
            ("ground_permille", (0, 1001, 50.0, "50", True), r"stac.ground_permille must be an integer in 1 \.\. 1000"),
            ("ground_contact", (-0.001, "x", True, float("inf")), "stac.ground_contact must be a finite number >= 0")):
        for bad in bads:
            with pytest.raises(ConfigError, match=text):
                hs.stage_cfg(rodent_cfg, **{key: bad})
    with pytest.raises(ConfigError, match="keys outside the schema"):
        hs.stage_cfg(rodent_cfg, ground_floor="x")
    # ground_floor_z is what a level run records in the config that its result file stores: a finite number, and with level only
    assert hs.stage_cfg(rodent_cfg, ground="level", ground_floor_z=0.003).stac.ground_floor_z == 0.003
    for bad in ("0.003", True, float("nan"), [0.003]):
        with pytest.raises(ConfigError, match="stac.ground_floor_z must be a finite number"):
            hs.stage_cfg(rodent_cfg, ground="level", ground_floor_z=bad)
    for mode in ("off", "report"):
        with pytest.raises(ConfigError, match="stac.ground_floor_z = 0.003 .* goes with level only"):
            hs.stage_cfg(rodent_cfg, ground=mode, ground_floor_z=0.003)
    pre = _Preflight(hs.stage_cfg(rodent_cfg), 100, "fit.h5")
    pre.check_config()
    assert pre.ground == default
    cfg = hs.stage_cfg(rodent_cfg, ground="level", ground_track=["foot_L", "foot_R"])
    assert cfg.to_dict()["stac"]["ground"] == "level" and hs.stage_cfg(rodent_cfg, ground=False).stac.ground == "off"  # (what a result file stores)
    pre = _Preflight(cfg, 100, "fit.h5")
    pre.check_config()
    assert pre.ground["mode"] == "level" and pre.ground["track"] == ["foot_L", "foot_R"]
    cfg.stac.ground_permille = 0  # (a config that was changed after it was validated: the pre-flight reads the key again)
    with pytest.raises(ValueError, match="stac.ground_permille must be an integer in 1 .. 1000"):
        _Preflight(cfg, 100, "fit.h5").check_config()
    # level takes its floor from the whole result: an explicit gather = none on more than one rank is refused before any work
    from stac_mjx_amd.main import GROUND_LEVEL_SHARDED

    for mode, refused in (("level", True), ("report", False)):
        sharded = _Preflight(hs.stage_cfg(rodent_cfg, ground=mode, gather="none"), 100, "fit.h5")
        sharded.check_config()
        sharded.check_run(1)
        if refused:
            with pytest.raises(ValueError) as exc:
                sharded.check_run(2)
            assert str(exc.value) == GROUND_LEVEL_SHARDED
        else:
            sharded.check_run(2)
    # level moves the model through a free root that the fit places: refused on the tethered fly, taken on the rodent; report is taken on both
    assert rodent_setup.freejoint and rodent_setup.do_root_opt and not fly_setup.do_root_opt
    check_ground_level("level", rodent_setup)
    check_ground_level("report", fly_setup)
    with pytest.raises(ValueError, match="free root joint"):
        check_ground_level("level", fly_setup)
    with pytest.raises(ValueError, match="free root joint"):
        check_ground_level("level", types.SimpleNamespace(freejoint=False, do_root_opt=True))
    from stac_mjx_amd.main import _check_ground_model

    asked = []
    stub = types.SimpleNamespace(setup=fly_setup, ground_table=lambda *a: asked.append(a))
    with pytest.raises(ValueError) as exc:
        _check_ground_model(pre.ground, stub)
    assert str(exc.value) == GROUND_LEVEL_FIXED_ROOT and not asked
    _check_ground_model(dict(pre.ground, mode="report"), stub)
    assert asked == [("fitted", None, ["foot_L", "foot_R"])]  # (the names are checked by building the table)
    _check_ground_model(default, types.SimpleNamespace())  # (off: the model is not looked at)


# ---- the table of the rodent ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stored_fit(reference_dir, demo_viz):
    return gc.reference_fit(reference_dir, demo_viz)


def test_ground_table_of_the_rodent(stored_fit):
    from stac_mjx_amd import ground

    scene, tables, xpos, xquat = stored_fit
    counts = {t: int((scene.geom_type == t).sum()) for t in range(8)}
    assert len(scene.geom_names) == 101 and scene.n_skipped == 0 and counts == {0: 1, 1: 0, 2: 46, 3: 25, 4: 22, 5: 0, 6: 7, 7: 0}
    fitted = ground.fitted_bodies(tables)
    assert int(fitted.sum()) == 31 and not fitted[0]
    table = ground.ground_table(scene, tables)
    assert table.n_geoms == 100 and int(table.include.sum()) == 47 and table.n_slots == 0 and table.verts.shape == (0, 3)
    assert len(set(table.meta[table.include, 1])) <= 31 and fitted[table.meta[table.include, 1]].all() and not fitted[table.meta[~table.include, 1]].any()
    assert "floor" not in table.names and "foot_R_collision" in table.names and "vertebra_C30_collision" in table.names
    assert table.include[table.names.index("foot_R_collision")] and not table.include[table.names.index("vertebra_C30_collision")]
    every = ground.ground_table(scene, tables, "all", track=("foot_L", "foot_R"))
    assert every.include.all() and np.array_equal(every.meta[:, [0, 1, 4, 5]], table.meta[:, [0, 1, 4, 5]]) and np.array_equal(every.data, table.data)
    assert every.track == ["foot_L", "foot_R"] and set(every.meta[:, 3]) == {-1, 0, 1}
    assert [b for b, s in zip(every.body_names, every.meta[:, 3]) if s == 1] == ["foot_R"] * int((every.meta[:, 3] == 1).sum())
    # the rotation is the matrix of geom_quat in float64, rounded once; sizes and positions are the scene's
    i = scene.geom_names.index("foot_R_collision")
    r = table.names.index("foot_R_collision")
    R = table.data[r, 6:].reshape(3, 3).astype(np.float64)
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=3e-7)
    assert np.array_equal(table.data[r, :3], scene.geom_size[i].astype(np.float32)) and np.array_equal(table.data[r, 3:6], scene.geom_pos[i].astype(np.float32))
    named = ground.ground_table(scene, tables, ["foot_R_collision", "skull"])
    assert named.include[r] and int(named.include.sum()) == 1 + int(sum(b == "skull" for b in named.body_names))
    some = ground.ground_table(scene, tables, geom_groups=[int(scene.geom_group[i])])
    assert 0 < some.n_geoms <= 100 and "foot_R_collision" in some.names
    for kw, text in ((dict(geoms=["no_such"]), "neither a geom nor a body"), (dict(geoms="most"), "geoms must be fitted, all or a list"),
                     (dict(track=["no_such"]), "not a body with geoms"), (dict(track=["foot_L", "foot_L"]), "twice"),
                     (dict(track=[f"b{i}" for i in range(33)]), "at most 32"), (dict(geom_groups=[7]), "no geom on a body")):
        with pytest.raises(ValueError, match=text):
            ground.ground_table(scene, tables, **kw)


# ---- the finding on the reference's stored fit -------------------------------------------------------------------------------------
def _cpu_clearance(rule, table, xpos, xquat, z_ref=0.0):
    clearance, _ = rule
    return clearance(xpos, xquat, table.meta, table.data, table.verts, table.n_slots, z_ref)


def test_the_unfitted_chains_of_the_stored_fit_are_under_the_floor(rule, stored_fit):
    """The reference's own stored fit, 50 frames.  Over every geom the lowest point of the animal is the last tail vertebra, some 7 cm
    below z = 0, and 23 geoms are below z = 0 in every frame, none of which the fit can move; over the geoms of the 31 bodies that
    the fit can move the lowest point is the right foot, 3 mm above z = 0.  (Centres measured with a float64 prototype: the median
    of the first -72.5 mm, the second 2.95 .. 3.64 mm; the widths are for float32 and for the scaling rule of the tables.)"""
    from stac_mjx_amd import ground

    scene, tables, xpos, xquat = stored_fit
    assert xpos.shape == (50, 67, 3)
    every = ground.ground_table(scene, tables, "all")
    got = _cpu_clearance(rule, every, xpos, xquat)
    print("all: low_z mm", np.sort(got["low_z"])[[0, 25, 49]] * 1e3, "lowest", {every.names[g] for g in got["low_geom"]})
    assert [every.names[g] for g in got["low_geom"]] == ["vertebra_C30_collision"] * 50
    assert -0.075 <= float(np.median(got["low_z"])) <= -0.070
    fitted = ground.ground_table(scene, tables, "fitted")
    fit = _cpu_clearance(rule, fitted, xpos, xquat)
    print("fitted: low_z mm", np.sort(fit["low_z"])[[0, 25, 49]] * 1e3, "lowest", {fitted.names[g] for g in fit["low_geom"]})
    assert [fitted.names[g] for g in fit["low_geom"]] == ["foot_R_collision"] * 50
    assert (fit["low_z"] >= 0.0025).all() and (fit["low_z"] <= 0.0040).all()
    always = fit["geom_below"] == 50
    print("below z = 0 in every frame:", [fitted.names[g] for g in np.flatnonzero(always)])
    assert int(always.sum()) == 23 and not fitted.include[always].any()
    assert np.array_equal(fit["geom_below"], got["geom_below"]) and np.array_equal(gc.bits(fit["geom_min"]), gc.bits(got["geom_min"]))
    # the summary says the same: the floor of the fitted geoms is near 3 mm, and the 23 geoms are the tail finding
    import torch

    summary = ground.summarize({k: torch.as_tensor(v) for k, v in fit.items()}, fitted, 0.0, 50, 0.002)
    assert summary["n_included"] == 47 and summary["floor_z"] == float(np.sort(fit["low_z"])[2])  # (rank ceil(50 * 50 / 1000) = 3)
    assert summary["low_z"]["min"] == float(fit["low_z"].min()) and summary["low_z"]["median"] == float(np.sort(fit["low_z"])[24])
    assert len(summary["unfitted_below"]) >= 23 and "vertebra_C30_collision" in summary["unfitted_below"]
    lowest = {g["name"]: g["frames_lowest"] for g in summary["geoms"]}
    assert lowest["foot_R_collision"] == 50 and sum(lowest.values()) == 50
    json.dumps(summary)


# ---- the sidecar and the levelled result -----------------------------------------------------------------------------------------------
def test_the_sidecar_and_the_levelled_result_file(tmp_path, rule, stored_fit, demo_viz, rodent_cfg):
    """run_stac's stage with the CPU rule in the place of the kernel: report leaves the result alone; level subtracts floor_z in
    float32 from the four z columns, counts the geoms below the new floor on the unshifted arrays, and the file, its stored config
    and the sidecar say so"""
    import torch

    from stac_mjx_amd import ground, io
    from stac_mjx_amd.main import _ground_config, _ground_stage, _write_ground, ground_path

    scene, tables, xpos, xquat = stored_fit
    N, K = 50, tables.nsite
    kp = np.ascontiguousarray(demo_viz["kp_data"][:N], dtype=np.float32).reshape(N, -1)

    def make():
        return io.StacData(qpos=demo_viz["qpos"][:N].astype(np.float32), xpos=xpos.copy(), xquat=xquat.copy(),
                           marker_sites=kp.reshape(N, K, 3) + np.float32(0.001), offsets=demo_viz["offsets"].astype(np.float32), kp_data=kp.copy(),
                           names_qpos=[f"q{i}" for i in range(tables.nq)], names_xpos=list(tables.body_names), kp_names=[f"k{i}" for i in range(K)])

    calls = []

    def clearance(data, geoms=None, track=None, z_ref=None, permille=None, contact=None):
        table = ground.ground_table(scene, tables, geoms, None, track)
        res = _cpu_clearance(rule, table, np.asarray(data.xpos), np.asarray(data.xquat), z_ref)
        calls.append((z_ref, np.asarray(data.xpos).copy()))
        return {"summary": ground.summarize({k: torch.as_tensor(v) for k, v in res.items()}, table, z_ref, permille, contact)}

    stub = types.SimpleNamespace(ground_clearance=clearance)
    cfg = hs.stage_cfg(rodent_cfg, ground="report", ground_track=["foot_L", "foot_R"])
    opt = _Preflight_ground(cfg)
    data = make()
    summary = _ground_stage(stub, data, opt)
    assert summary["mode"] == "report" and "level" not in summary and len(calls) == 1
    for name in ("qpos", "xpos", "marker_sites", "kp_data"):
        assert np.array_equal(getattr(data, name), getattr(make(), name)), name
    assert [t["body"] for t in summary["tracks"]] == ["foot_L", "foot_R"] and all(0.0 <= t["contact_fraction"] <= 1.0 for t in summary["tracks"])
    assert summary["tracks"][1]["contact_fraction"] > 0.5  # (the right foot is the lowest fitted geom in every frame)
    stored = _ground_config(cfg, opt, summary)
    assert stored.stac.ground == "report" and "ground_floor_z" not in stored.stac
    was_level = hs.stage_cfg(rodent_cfg, ground="level", ground_floor_z=0.01)  # (the config of a fit file that a level run wrote)
    assert "ground_floor_z" not in _ground_config(was_level, opt, summary).stac
    # level
    cfg = hs.stage_cfg(rodent_cfg, ground="level", ground_track=["foot_L", "foot_R"], ik_only_path="ik.npz")
    opt = _Preflight_ground(cfg)
    data, before = make(), make()
    del calls[:]
    summary = _ground_stage(stub, data, opt)
    floor = np.float32(summary["floor_z"])
    assert 0.0025 <= floor <= 0.0040 and summary["level"]["floor_z"] == float(floor)
    assert [c[0] for c in calls] == [0.0, float(floor)] and np.array_equal(calls[1][1], before.xpos)  # (the second call sees the unshifted arrays)
    assert np.array_equal(data.qpos[:, 2], before.qpos[:, 2] - floor) and np.array_equal(np.delete(data.qpos, 2, axis=1), np.delete(before.qpos, 2, axis=1))
    assert np.array_equal(data.xpos[..., 2], before.xpos[..., 2] - floor) and np.array_equal(data.xpos[..., :2], before.xpos[..., :2])
    assert np.array_equal(data.marker_sites[..., 2], before.marker_sites[..., 2] - floor) and np.array_equal(data.marker_sites[..., :2], before.marker_sites[..., :2])
    assert np.array_equal(data.kp_data[:, 2::3], before.kp_data[:, 2::3] - floor) and np.array_equal(data.kp_data[:, 0::3], before.kp_data[:, 0::3])
    assert np.array_equal(data.xquat, before.xquat) and np.array_equal(data.offsets, before.offsets)
    below = {g["name"]: g["frames_below"] for g in summary["level"]["geoms"]}
    assert below["foot_R_collision"] == 2 and below["vertebra_C30_collision"] == 50  # (rank 3 of 50: two frames are below the floor)
    stored = _ground_config(cfg, opt, summary)
    assert stored.stac.ground == "level" and stored.stac.ground_floor_z == float(floor) and stored.stac.ground_track == ["foot_L", "foot_R"]
    path = tmp_path / "ik.npz"
    io.save_data_to_h5(config=stored, file_path=path, **data.as_dict())
    side = _write_ground(path, summary)
    assert side == ground_path(path) and side.name == "ik.npz.ground.json"
    back_cfg, back = io.load_stac_data(path)
    assert back_cfg.stac.ground == "level" and back_cfg.stac.ground_floor_z == float(floor)
    for name in ("qpos", "xpos", "xquat", "marker_sites", "kp_data", "offsets"):
        assert np.array_equal(getattr(back, name), getattr(data, name)), name
    read = json.loads(side.read_text())
    assert read == json.loads(json.dumps(summary)) and read["level"]["floor_z"] == float(floor) and read["mode"] == "level"
    # a result without a finite lowest z has no floor to subtract
    nothing = types.SimpleNamespace(ground_clearance=lambda *a, **k: {"summary": {"floor_z": None}})
    with pytest.raises(ValueError, match="no floor to subtract"):
        _ground_stage(nothing, make(), opt)


def _Preflight_ground(cfg):
    from stac_mjx_amd.main import _Preflight

    pre = _Preflight(cfg, 50, "fit.h5")
    pre.check_config()
    return pre.ground


def test_summary_helpers():
    import torch

    from stac_mjx_amd import ground

    assert [ground.kth_rank(pm, n) for pm, n in ((50, 50), (50, 1), (500, 3), (1000, 7), (1, 1000), (1, 1001))] == [3, 1, 2, 7, 1, 2]
    low = torch.tensor([0.5, float("nan"), -1.0, float("inf"), 2.0, 0.25])
    assert float(ground.floor_level(low, 500)) == 0.25 and float(ground.floor_level(low, 1)) == -1.0 and float(ground.floor_level(low, 1000)) == 2.0
    assert ground.floor_level(torch.tensor([float("nan")]), 50) is None
