"""The q_phase kernels on trees whose depth and width sit on the host planner's limits, and the C. elegans config: HIP against the
oracle at tolerance 0.  The models and their facts come from tests/tree_cases.py; tests/test_tree_shapes_host.py asserts
on the CPU what the case names claim (program sizes, widths).  Every case names the instantiation stac_debug_last_q_kernel must
report after the launch, (G, NQR, WPE, SPECP) -- worked out from stac_shapes.hpp and plan_q, confirmed on the MI355X -- or a refusal
by name; the width cases also name bit 1 of the launch's flags word (set: fk_chain walks the level tables; clear: the step program,
four lanes per position when 4 * max_width <= G), read from the plan line of an engine created with STAC_HIP_VERBOSE.

Depth (lean): serial chains with a full P3 table (n3 = 252) inside the 16-lane and the 32-lane lean kernels, a full P1 table
(n1 = 254), the deepest model the shapes hold (250 levels, nq = 256), a program without any rotation, and the chains one body past
the full tables, which must run a generic kernel without any developer switch.  Each with the root optimisation on (trunk: the first
and the last site) and off (the free root moved by the full-body solve only, as in C. elegans).
Width (generic): stars under a fixed root at G / 4, G / 4 + 1, G, G + 1 and 2 G + 1 leaves for every lane count, 4 and 5 leaves, leaves
without a site, oriented leaves; free-root stars of 16 and 17 leaves through the automatic lane choice and the straggler hand-off; a
broom (40 levels, 20 leaves).
LM: chain(84) and star(33) bit for bit; serial chains of 192 coordinates (dense Gauss-Newton matrix, path depth 192), 193 refused.
C. elegans (configs/model/celegans.yaml): q_phase with five empty part groups and no root optimisation, Stac.fit_offsets through the
sampled offset phase, run_stac with the reference's own stac group; the keypoints are synthetic (the reference ships no recording).
"""

import json
import re

import numpy as np
import pytest

import kin_ref
import tree_cases as tc
from conftest import GOLDEN
from fk3_cases import lean_box
from test_gpu_fk3_rounds import LAUNCHES, _assert_same, _bits, _last_q_kernel

pytestmark = pytest.mark.gpu

THR2 = {"STAC_HIP_WPE": "2", "STAC_HIP_SPEC": "0"}
NOLEAN = dict(THR2, STAC_HIP_NOLEAN="1")


def _lat(g):
    return {"STAC_HIP_SPEC": "1", "STAC_HIP_SPECG": str(g)}


def _engine(monkeypatch, t, lb, ub, lanes, env, **kw):
    from stac_mjx_amd.engine import Engine

    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (read once, when the engine creates its model)
    return Engine(t, lb, ub, lanes_per_chain=lanes, **{"tol": tc.TOL, "maxiter": tc.MAXITER, **kw})


def _plan_fields(err):
    """The key=value numbers of the call's last launch-plan line (plan_q / plan_q_lm, STAC_HIP_VERBOSE)."""
    plan = [ln for ln in err.splitlines() if ln.startswith("[stac] q_phase") and " chains=" in ln]
    assert plan, err
    return {k: int(x) for k, x in re.findall(r"(\w+)=(-?\d+)\b", plan[-1])}


# ---- depth: the lean kernels at full split-kinematics tables ---------------------------------------------------------------------------
_THR16, _LAT16 = LAUNCHES["throughput"], LAUNCHES["latency"]
_SPACER = lambda: tc.spacer_chain_full_p3()[1]  # noqa: E731
# id -> (model, {launch: (lanes, environment, expected instantiation)}); the first launch of a case is compared with the others
DEPTH_CASES = {
    # n3 = 252 at nq = 80: the 16-lane lean kernels, the rodent's product path
    "full-p3-16": (_SPACER, {"lean-thr": (_THR16[1], dict(_THR16[0], STAC_HIP_WPE="2"), (16, 5, 2, 1)),
                             "lean-lat": (_LAT16[1], _LAT16[0], (16, 5, 2, 5)),
                             "generic": (16, NOLEAN, (16, 5, 2, 0))}),
    # n3 = 252 at nq = 91: 32 lanes
    "full-p3-32": (lambda: tc.chain(84), {"lean-thr": (32, THR2, (32, 3, 2, 1)), "lean-lat": (0, _lat(32), (32, 3, 2, 9)),
                                          "generic": (32, NOLEAN, (32, 3, 2, 0))}),
    # a 253rd rotation: no program, a generic kernel without any developer switch
    "past-p3": (lambda: tc.chain(85), {"no-switch": (32, {}, (32, 3, 2, 0))}),
    # n1 = 254
    "full-p1": (lambda: tc.chain(127, oriented=True, zero_jnt_pos=True), {"lean-thr": (32, THR2, (32, 8, 2, 1)),
                                                                          "generic": (32, NOLEAN, (32, 8, 2, 0))}),
    "past-p1": (lambda: tc.chain(128, oriented=True, zero_jnt_pos=True), {"no-switch": (32, {}, (32, 8, 2, 0))}),
    # 250 levels, nq = 256 (the latency layout of 256 coordinates does not fit the LDS: the throughput kernel takes the call,
    # test_gpu_boundaries._LDS_LIMITED_EDGES)
    "deepest": (lambda: tc.chain(249, zero_jnt_pos=True), {"lean-thr": (32, THR2, (32, 8, 2, 1)), "lat-fallback": (0, _lat(32), (32, 8, 2, 1))}),
    # n2 = n3 = 0
    "no-rotation": (lambda: tc.chain(249, zero_jnt_pos=True, zero_body_pos=True), {"lean-thr": (32, THR2, (32, 8, 2, 1))}),
}
_DEPTH_PARAMS = [(c, l, r) for c, (_, ls) in DEPTH_CASES.items() for l in ls for r in (True, False)]
_DEPTH_RES = {}


@pytest.mark.parametrize("case,launch,root_opt", _DEPTH_PARAMS, ids=[f"{c}-{l}-{'root' if r else 'noroot'}" for c, l, r in _DEPTH_PARAMS])
def test_depth_case(monkeypatch, case, launch, root_opt):
    make, launches = DEPTH_CASES[case]
    lanes, env, expect = launches[launch]
    t = make()
    lb, ub = lean_box(t)
    trunk = tc.trunk_two(t)
    kp, part, ref = tc.case(("depth", case), t, lb, ub, trunk, do_root_opt=root_opt)
    eng = _engine(monkeypatch, t, lb, ub, lanes, env)
    res = eng.q_phase(kp, part_masks=part, trunk_kps=trunk, root_kp_idx=0, root_dims=7, do_root_opt=root_opt)
    got = _last_q_kernel(eng)
    print(case, launch, root_opt, "kernel", got)
    if "past" in case:
        assert got[3] & 1 == 0  # one body past the full table: never lean
    _assert_same(res, ref, f"{case} {launch} root_opt={root_opt}")
    np.testing.assert_array_equal(_bits(res["marker_sites"]), _bits(ref["marker_sites"]))
    # two HIP launches of the same case: everything a launch returns
    first = _DEPTH_RES.setdefault((case, root_opt), {k: _bits(res[k]) for k in ("counters", "qpos", "frame_error", "marker_sites", "carry_qpos")})
    for k, v in first.items():
        np.testing.assert_array_equal(_bits(res[k]), v, err_msg=f"{case} {launch} against the case's first launch: {k}")
    eng.close()
    assert got == expect, (case, launch, got, expect)


# ---- width: the generic kernels' three kinematics paths ----------------------------------------------------------------------------------
def _gen_inst(G, nq):
    """The throughput instantiation of G lanes at two wavefronts per SIMD that holds nq (stac_shapes.hpp, STAC_Q_SHAPES)."""
    rows = {8: (10, 16), 16: (5, 8, 16), 32: (3, 4, 8), 64: (2, 4)}[G]
    return (G, next(r for r in rows if nq <= G * r), 2, 0)


def _fixed(G, w, **kw):
    # fixed_star(w): nq = w + 2 (the root body's hinge, the hub's, one per leaf), K = w + 1
    tag = "".join(f"-{k}" for k in kw)
    return (f"fixed{tag}-G{G}-w{w}", lambda: tc.fixed_star(w, **kw), G, w, THR2, _gen_inst(G, w + 2 + kw.get("idle", 0)), 2 if w > G else 0)


# (id, model, lanes, max_width, environment, expected instantiation, expected bit 1 of the flags word)
WIDTH_CASES = [_fixed(G, w) for G in (8, 16, 32, 64) for w in (G // 4, G // 4 + 1, G, G + 1, 2 * G + 1)] + [
    _fixed(8, 4), _fixed(8, 5), _fixed(64, 4), _fixed(64, 5),            # max_width0 > 4: every transform stored
    _fixed(32, 8, idle=1), _fixed(32, 32, idle=1), _fixed(8, 8, idle=3),  # leaves without a site do not count
    _fixed(32, 8, oriented=True), _fixed(16, 17, oriented=True),          # oriented leaves: fk_rec_words = 16
    ("broom-40x20", lambda: tc.broom(40, 20), 32, 20, NOLEAN, (32, 3, 2, 0), 0),
    ("broom-40x20-G16", lambda: tc.broom(40, 20), 16, 20, NOLEAN, (16, 5, 2, 0), 2),
]
# The automatic lane choice and the straggler hand-off (max_width <= kLatG = 16) under a free root.  With lanes_per_chain = 0 the
# eight chains of a case go to the latency mode (eight roles of 32 lanes, lean) before pick_lanes reaches its width test
# (max_width * 4 <= 32): that test is only read for thousands of chains of a model whose 16-lane residency is under half its 32-lane
# one, which no case of a few seconds has.  What is pinned is the launch the automatic choice does make at both widths.
AUTO_CASES = [
    # (id, leaves, lanes, environment, the last kernel, the main launch's instantiation, expected hand-off capacity or None)
    ("auto-w16", 16, 0, {}, (32, 2, 2, 9), (32, 2, 2, 9), None),
    ("auto-w17", 17, 0, {}, (32, 2, 2, 9), (32, 2, 2, 9), None),
    # (a hand-off's last kernel is the resume launch: the generic latency kernel, four roles of 16 lanes -- 16 leaves on 16 lanes)
    ("handoff-w16", 16, 32, dict(NOLEAN, STAC_HIP_HANDOFF="4"), (16, 5, 2, 4), (32, 3, 2, 0), 4),
    ("handoff-w17", 17, 32, dict(NOLEAN, STAC_HIP_HANDOFF="4"), (32, 3, 2, 0), (32, 3, 2, 0), 0),  # wider than the latency kernel's lane group
]


def _width_run(monkeypatch, capfd, name, t, lanes, env, do_root_opt):
    lb, ub = lean_box(t)
    trunk = tc.trunk_two(t)
    kp, part, ref = tc.case(("width", name), t, lb, ub, trunk, do_root_opt=do_root_opt)
    eng = _engine(monkeypatch, t, lb, ub, lanes, dict(env, STAC_HIP_VERBOSE="1"))
    capfd.readouterr()
    res = eng.q_phase(kp, part_masks=part, trunk_kps=trunk, root_kp_idx=0, root_dims=7, do_root_opt=do_root_opt)
    err = capfd.readouterr().err
    got = _last_q_kernel(eng)
    eng.close()
    return res, ref, got, err


@pytest.mark.parametrize("case", WIDTH_CASES, ids=[c[0] for c in WIDTH_CASES])
def test_width_case(monkeypatch, capfd, case):
    name, make, lanes, width, env, expect, flag2 = case
    t = make()
    assert tc.max_width(t) == width
    free = int(t.jnt_type[0]) == 0
    res, ref, got, err = _width_run(monkeypatch, capfd, name, t, lanes, env, free)
    v = _plan_fields(err)
    print(name, "kernel", got, "flags", v.get("flags"))
    if width > lanes:
        assert v["flags"] & 2  # a level wider than the lane group: never the step program
    _assert_same(res, ref, name)
    for k in ("marker_sites", "xpos", "xquat"):
        np.testing.assert_array_equal(_bits(res[k]), _bits(ref[k]), err_msg=f"{name}: {k}")
    assert got == expect, (name, got, expect)
    assert v["flags"] & 2 == flag2, (name, v)


@pytest.mark.parametrize("case", AUTO_CASES, ids=[c[0] for c in AUTO_CASES])
def test_free_root_star_auto_lanes_and_handoff(monkeypatch, capfd, case):
    name, w, lanes, env, expect, main, hcap = case
    t = tc.star(w)
    assert tc.max_width(t) == w
    res, ref, got, err = _width_run(monkeypatch, capfd, name, t, lanes, env, True)
    print(name, "kernel", got, [ln for ln in err.splitlines() if ln.startswith("[stac] q_phase")][-2:])
    _assert_same(res, ref, name)
    np.testing.assert_array_equal(_bits(res["marker_sites"]), _bits(ref["marker_sites"]))
    assert got == expect, (name, got, expect)
    plan = [ln for ln in err.splitlines() if ln.startswith("[stac] q_phase") and " chains=" in ln][-1]
    assert "inst={%d,%d,%d,%d}" % main in plan, (name, plan)
    if hcap is not None:
        assert _plan_fields(err)["handoff"] == hcap, (name, err)
        assert ("hand-off of up to 4 stragglers" in err) == (hcap > 0), (name, err)


# ---- LM ----------------------------------------------------------------------------------------------------------------------------------
LM_CAPACITY = ("kinematic path too deep for the LM solver", "model exceeds the LM q_phase kernel limits")
FITS, REFUSED = "equals ik_clips_lm bit for bit", "refused for capacity"
# (id, model, do_root_opt, observed outcome).  n = 192 on ONE path: 18 528 matrix entries and a path table of 192 x 192 words per
# chain -- more than the LDS of a workgroup: plan_q_lm refuses both with "model exceeds the LM q_phase kernel limits".
LM_DENSE_CASES = [
    ("lm-fixed-n192", lambda: tc.chain(191, free_root=False), REFUSED),
    ("lm-free-n192", lambda: tc.chain(185), REFUSED),
]


def _lm_case(t, rng, n_clips=2):
    from oracle import Oracle

    lb, ub = lean_box(t)
    orc = Oracle(t, tol=1e-4)
    q = np.tile(t.qpos0, (n_clips, 1)) + rng.normal(0, 0.15, (n_clips, t.nq)).astype(np.float32)
    q = np.clip(q, np.where(np.isfinite(lb), lb, -3), np.where(np.isfinite(ub), ub, 3)).astype(np.float32)
    kp = np.stack([orc.fk(x.copy())["site_xpos"].reshape(-1) for x in q]).astype(np.float32)
    kp = (kp + rng.normal(0, 2e-3, kp.shape)).astype(np.float32).reshape(n_clips, 1, 3 * t.nsite)
    return lb, ub, orc, kp


def _assert_lm_equal(res, ref, lb, ub, what):
    for key in ("qpos", "frame_error", "counters"):
        np.testing.assert_array_equal(_bits(res[key]), _bits(ref[key]), err_msg=f"{what}: {key}")
    q = res["qpos"].cpu().numpy()
    assert (q >= lb).all() and (q <= ub).all(), what  # the box is respected


@pytest.mark.parametrize("case", LM_DENSE_CASES, ids=[c[0] for c in LM_DENSE_CASES])
def test_lm_dense_chain_of_192_coordinates(case):
    """Every coordinate on one path: the Gauss-Newton matrix is fully dense.  The kernel either holds it and equals the oracle, or the
    host refuses it for capacity by name -- never a third thing.  (The only cases of this file with two admissible outcomes; the
    observed one stands in the table.)"""
    from stac_mjx_amd.engine import Engine, StacHipError

    name, make, observed = case
    t = make()
    assert t.nq == 192 and tc.path_depth(t) == t.nbody - 1 and tc.max_width(t) == 1
    lb, ub, orc, kp = _lm_case(t, np.random.default_rng(sum(map(ord, name))))
    part = np.ones((1, t.nq), np.uint8)
    kw = dict(part_masks=part, trunk_kps=tc.trunk_two(t), root_kp_idx=0, root_dims=7, do_root_opt=False)
    eng = Engine(t, lb, ub, tol=1e-4, solver="lm", lm_maxiter=6)
    try:
        res = eng.q_phase(kp, **kw)
    except StacHipError as e:
        print(name, "refused:", e)
        assert "error -3" in str(e) and any(m in str(e) for m in LM_CAPACITY), e
        assert observed == REFUSED, (name, e)
    else:
        ref = orc.ik_clips_lm(kp, lb, ub, part, kw["trunk_kps"], 0, 7, do_root_opt=False, maxiter=6)
        _assert_lm_equal(res, ref, lb, ub, name)
        assert observed == FITS, name
    eng.close()


def test_lm_refuses_193_coordinates_on_one_path():
    from stac_mjx_amd.engine import Engine, StacHipError

    t = tc.chain(192, free_root=False)
    assert t.nq == 193
    lb, ub, _, kp = _lm_case(t, np.random.default_rng(193))
    eng = Engine(t, lb, ub, tol=1e-4, solver="lm", lm_maxiter=6)
    with pytest.raises(StacHipError) as ei:
        eng.q_phase(kp, part_masks=np.ones((1, t.nq), np.uint8), trunk_kps=tc.trunk_two(t), root_kp_idx=0, root_dims=7, do_root_opt=False)
    assert "error -3" in str(ei.value) and "more than 192 optimised coordinates" in str(ei.value), ei.value
    eng.close()


@pytest.mark.parametrize("model", ["chain84", "star33"])
def test_lm_on_a_deep_and_a_wide_tree(model):
    from stac_mjx_amd.engine import Engine

    t = tc.chain(84) if model == "chain84" else tc.star(33)
    rng = np.random.default_rng(len(model) + t.nq)
    lb, ub, orc, kp = _lm_case(t, rng, n_clips=4)
    kp = kp.reshape(2, 2, -1)
    part = np.zeros((2, t.nq), np.uint8)
    part[0] = rng.random(t.nq) < 0.5
    part[1] = rng.random(t.nq) < 0.15
    trunk = tc.trunk_two(t)
    eng = Engine(t, lb, ub, tol=1e-4, solver="lm", lm_maxiter=8)
    res = eng.q_phase(kp, part_masks=part, trunk_kps=trunk, root_kp_idx=0, root_dims=7, do_root_opt=True)
    ref = orc.ik_clips_lm(kp, lb, ub, part, trunk, 0, 7, do_root_opt=True, maxiter=8)
    _assert_lm_equal(res, ref, lb, ub, model)
    eng.close()


# ---- the arrays a q_phase returns ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["chain84", "chain249", "star65"])
def test_returned_kinematics_equal_the_oracle_and_the_float64_statement(monkeypatch, model):
    """xpos, xquat and marker_sites of the launch == the oracle's bit for bit, and within the float32 bound of
    test_gpu_boundaries._fk_tol (16 ulp per level: the bound tests/test_tree_shapes_host.py holds the oracle to) of kin_ref.fk at
    the returned qpos."""
    from test_gpu_boundaries import _fk_tol

    t = {"chain84": lambda: tc.chain(84), "chain249": lambda: tc.chain(249, zero_jnt_pos=True), "star65": lambda: tc.star(65)}[model]()
    lb, ub = lean_box(t)
    trunk = tc.trunk_two(t)
    kp, part, ref = tc.case(("outputs", model), t, lb, ub, trunk, do_root_opt=True, chains=4)
    eng = _engine(monkeypatch, t, lb, ub, 32, THR2)
    res = eng.q_phase(kp, part_masks=part, trunk_kps=trunk, root_kp_idx=0, root_dims=7, do_root_opt=True)
    eng.close()
    _assert_same(res, ref, model)
    for k in ("xpos", "xquat", "marker_sites"):
        np.testing.assert_array_equal(_bits(res[k]), _bits(ref[k]), err_msg=f"{model}: {k}")
    qpos = res["qpos"].cpu().numpy().reshape(-1, t.nq)
    got = {k: res[k].cpu().numpy().reshape(len(qpos), -1, 4 if k == "xquat" else 3).astype(np.float64) for k in ("xpos", "xquat", "marker_sites")}
    worst = 0.0
    for i, x in enumerate(qpos):
        xpos, xquat, sites = kin_ref.fk(t, x)
        tol = _fk_tol(tc.path_depth(t), max(np.abs(xpos).max(), np.abs(sites).max()))
        for k, r in (("xpos", xpos), ("xquat", xquat), ("marker_sites", sites)):
            dev = np.abs(got[k][i] - r).max()
            worst = max(worst, dev)
            assert dev <= tol, (model, i, k, dev, tol)
    print(f"{model}: returned kinematics vs kin_ref.fk max {worst:.3g}")


# ---- the C. elegans config -----------------------------------------------------------------------------------------------------------
def celegans_fit_setup():
    """(FitSetup, {"model": ..., "stac": ...}) of configs/model/celegans.yaml from the committed fixtures."""
    from stac_mjx_amd.fit_model import finish_fit_setup
    from stac_mjx_amd.mjcf import ModelTables

    with open(GOLDEN / "celegans_model_cfg.json") as fh:
        cfg = json.load(fh)
    tables = ModelTables.load(GOLDEN / "celegans_tables.npz")
    return finish_fit_setup(tables, cfg["model"], list(cfg["model"]["KEYPOINT_MODEL_PAIRS"].keys())), cfg


@pytest.fixture(scope="module")
def celegans_setup():
    return celegans_fit_setup()[0]


@pytest.fixture(scope="module")
def celegans_cfg():
    return celegans_fit_setup()[1]


def celegans_keypoints(t, T, seed=2025):
    """The reference ships no C. elegans recording.  A travelling wave down the 24 hinges, qpos[t, 7 + i] = 0.35 sin(0.3 t + 0.5 i),
    under a tilted root with a millimetre of jitter on its position; the sites displaced by N(0, 2 mm) offsets, N(0, 0.2 mm) of noise
    on the keypoints.  -> kp [T, 75] float32"""
    from oracle import Oracle

    rng = np.random.default_rng(seed)
    q = np.tile(t.qpos0, (T, 1)).astype(np.float32)
    q[:, 7:] = 0.35 * np.sin(0.3 * np.arange(T)[:, None] + 0.5 * np.arange(t.nq - 7)[None])
    quat = np.array([0.96, 0.10, -0.15, 0.20])
    q[:, 3:7] = quat / np.linalg.norm(quat)
    q[:, :3] = t.qpos0[:3] + np.array([0.01, -0.02, 0.005]) + rng.normal(0, 1e-3, (T, 3))
    orc = Oracle(t)
    orc.set_site_pos((t.site_pos + rng.normal(0, 2e-3, (t.nsite, 3))).astype(np.float32))
    kp = np.stack([orc.fk(x.copy())["site_xpos"].reshape(-1) for x in q]).astype(np.float32)
    return (kp + rng.normal(0, 2e-4, kp.shape)).astype(np.float32)


def _celegans_cfg(cfg, **stac_over):
    from stac_mjx_amd.config import validate_config

    return validate_config({"model": dict(cfg["model"]), "stac": dict(cfg["stac"], data_path="none.mat", **stac_over)})


_CE_REF = {}


def _celegans_ref(fs, cfgm, solver):
    """6 chains of 4 frames at the config's own FTOL = 5e-3, N_ITER_Q = 400, and the oracle's answer."""
    if solver not in _CE_REF:
        from oracle import Oracle

        kp = celegans_keypoints(fs.tables, 24).reshape(6, 4, 75)
        orc = Oracle(fs.tables, tol=float(cfgm["FTOL"]), maxiter=int(cfgm["N_ITER_Q"]))
        args = (kp, fs.lb, fs.ub, fs.part_masks, fs.trunk_kps, max(fs.root_kp_idx, 0), fs.root_dims)
        _CE_REF[solver] = (kp, orc.ik_clips(*args, do_root_opt=False) if solver == "pg" else orc.ik_clips_lm(*args, do_root_opt=False, maxiter=20))
    return _CE_REF[solver]


@pytest.mark.parametrize("lanes,solver", [(16, "pg"), (0, "pg"), (0, "lm")])
def test_celegans_q_phase(celegans_setup, celegans_cfg, lanes, solver):
    """What Stac._q_phase passes for this config: no root optimisation, root_kp_idx = max(-1, 0), five EMPTY part masks -- five part
    solves per frame that optimise nothing and count one iteration each.  Every full-body solve runs to its bound of 400 iterations
    from qpos0 (the root is found by the full-body solve alone), beyond the 256 entries of the momentum table (stac_plan.hpp, kTTab)."""
    from helpers import marker_error_mm
    from stac_mjx_amd.engine import Engine

    fs, cfgm = celegans_setup, celegans_cfg["model"]
    kp, ref = _celegans_ref(fs, cfgm, solver)
    assert not fs.do_root_opt and fs.part_masks.shape == (5, 31) and not fs.part_masks.any()
    eng = Engine(fs.tables, fs.lb, fs.ub, tol=float(cfgm["FTOL"]), maxiter=int(cfgm["N_ITER_Q"]), lanes_per_chain=lanes, solver=solver, lm_maxiter=20)
    kw = dict(part_masks=fs.part_masks, trunk_kps=fs.trunk_kps, root_kp_idx=max(fs.root_kp_idx, 0), root_dims=fs.root_dims, do_root_opt=False)
    a, b = eng.q_phase(kp, **kw), eng.q_phase(kp, **kw)
    for k in ("counters", "qpos", "frame_error", "marker_sites", "carry_qpos"):
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"second launch differs in {k}")
        if k != "carry_qpos":
            np.testing.assert_array_equal(_bits(a[k]), _bits(ref[k]), err_msg=k)
    err = marker_error_mm(ref["marker_sites"], kp)
    print(f"celegans {solver} lanes={lanes}: iterations {int(ref['counters'][..., 0].min())}..{int(ref['counters'][..., 0].max())}, marker error {err:.2f} mm")
    if solver == "pg":
        assert (ref["counters"][..., 0] == 400 + 5).all()  # the full-body solve at its bound + five one-iteration empty part solves
    # A sanity bound beside the bit comparison: the sites sit N(0, 2 mm) per axis off the body origins the config starts from (3.2 mm
    # on average) under 0.2 mm of noise, and the segments are 40 mm long -- a fit that is a joint off misses by tens of millimetres.
    # Measured on the oracle: PG 3.47 mm, LM 3.14 mm.
    assert err < 5.0
    eng.close()


def test_celegans_lean_and_generic_agree(celegans_setup, celegans_cfg, monkeypatch):
    fs, cfgm = celegans_setup, celegans_cfg["model"]
    kp, ref = _celegans_ref(fs, cfgm, "pg")
    kw = dict(part_masks=fs.part_masks, trunk_kps=fs.trunk_kps, root_kp_idx=0, root_dims=fs.root_dims, do_root_opt=False)
    par = dict(tol=float(cfgm["FTOL"]), maxiter=int(cfgm["N_ITER_Q"]))
    lean_eng = _engine(monkeypatch, fs.tables, fs.lb, fs.ub, 16, dict(_THR16[0], STAC_HIP_WPE="2"), **par)
    lean = lean_eng.q_phase(kp, **kw)
    assert _last_q_kernel(lean_eng) == (16, 5, 2, 1), _last_q_kernel(lean_eng)  # (the 16-lane lean shape of two wavefronts per SIMD)
    # nq = 31 <= 48: at three wavefronts per SIMD the shape of three solver registers per lane, the fruit fly's
    lean3_eng = _engine(monkeypatch, fs.tables, fs.lb, fs.ub, 16, dict(_THR16[0], STAC_HIP_WPE="3"), **par)
    lean3 = lean3_eng.q_phase(kp, **kw)
    assert _last_q_kernel(lean3_eng) == (16, 3, 3, 1), _last_q_kernel(lean3_eng)
    lean3_eng.close()
    for k in ("counters", "qpos", "frame_error", "marker_sites", "carry_qpos"):
        np.testing.assert_array_equal(_bits(lean[k]), _bits(lean3[k]), err_msg=f"three registers per lane: {k}")
    gen_eng = _engine(monkeypatch, fs.tables, fs.lb, fs.ub, 16, NOLEAN, **par)
    gen = gen_eng.q_phase(kp, **kw)
    assert _last_q_kernel(gen_eng) == (16, 5, 2, 0), _last_q_kernel(gen_eng)
    _assert_same(lean, ref, "celegans, lean against the oracle")
    for k in ("counters", "qpos", "frame_error", "marker_sites", "carry_qpos"):
        np.testing.assert_array_equal(_bits(lean[k]), _bits(gen[k]), err_msg=k)
    lean_eng.close()
    gen_eng.close()


def test_celegans_fit_offsets_sampled_offset_phase(celegans_setup, celegans_cfg):
    """120 frames against N_SAMPLE_FRAMES = 100: the offset phase fits on the PRNGKey(0) sample.  Bit-equal to the oracle-driven
    restatement; and with no regularised site the closed form is the plain average, which the float64 statement gives on the same
    poses to TOL_NORTH_STAR."""
    from helpers import oracle_fit_offsets
    from stac_mjx_amd.prng import sample_time_indices
    from stac_mjx_amd.stac import Stac
    from test_gpu_parity import TOL_NORTH_STAR

    fs = celegans_setup
    cfgm = dict(celegans_cfg["model"], N_ITERS=1)
    kp = celegans_keypoints(fs.tables, 120)
    cfg = _celegans_cfg({"model": cfgm, "stac": celegans_cfg["stac"]}, n_fit_frames=120)
    assert int(cfg.model.N_SAMPLE_FRAMES) == 100 < 120 and float(cfg.model.M_REG_COEF) == 1 and not fs.is_regularized.any()
    stac = Stac(None, cfg, fs.kp_names, setup=fs, verbose=False)
    data = stac.fit_offsets(kp)
    stac.engine.close()
    history = []
    ref_off, ref = oracle_fit_offsets(fs, cfgm, kp, 1, history=history)
    np.testing.assert_array_equal(data.offsets, ref_off)
    for k in ("qpos", "marker_sites", "xpos", "xquat"):
        np.testing.assert_array_equal(getattr(data, k), ref[k], err_msg=k)
    idx = sample_time_indices(120, 100)
    m64, _ = kin_ref.m_opt(fs.tables, kp[idx], history[0][0]["qpos"][idx], fs.tables.site_pos, fs.is_regularized, 1.0)
    dev = np.abs(data.offsets - m64).max()
    print(f"celegans offsets vs kin_ref.m_opt: {dev:.3g}; |offsets| max {np.abs(data.offsets).max():.3g}")
    assert dev <= TOL_NORTH_STAR
    assert np.abs(data.offsets).max() > 1e-3  # the offsets moved off the body origins


def test_celegans_run_stac_with_the_reference_stac_group(celegans_setup, celegans_cfg, tmp_path, capsys):
    """configs/stac/stac_celegans.yaml as shipped (skip_ik_only, 250-frame clips, infer_qvels) with n_fit_frames cut to 12; then the
    ik_only phase on the same 12 frames in clips of 4."""
    from stac_mjx_amd.io import load_stac_data
    from stac_mjx_amd.main import run_stac

    fs = celegans_setup
    kp = celegans_keypoints(fs.tables, 12)
    cfg = _celegans_cfg(celegans_cfg, n_fit_frames=12)
    assert (cfg.stac.skip_ik_only, cfg.stac.n_frames_per_clip, cfg.stac.infer_qvels) == (True, 250, True)
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
    capsys.readouterr()
    fit_path, ik_path = run_stac(cfg, kp, fs.kp_names, base_path=tmp_path / "a", setup=fs)
    assert ik_path is None and "ROOT_OPTIMIZATION_KEYPOINT not specified" in capsys.readouterr().out
    _, fit = load_stac_data(fit_path)
    assert fit.qpos.shape == (12, 31) and fit.offsets.shape == (25, 3)
    cfg2 = _celegans_cfg(celegans_cfg, n_fit_frames=12, skip_ik_only=False, n_frames_per_clip=4)
    fit_path, ik_path = run_stac(cfg2, kp, fs.kp_names, base_path=tmp_path / "b", setup=fs)
    _, fit = load_stac_data(fit_path)
    _, ik = load_stac_data(ik_path)
    assert ik.qpos.shape == (12, 31) and ik.qvel.shape == (12, 30) and np.isfinite(ik.qvel).all()
    np.testing.assert_array_equal(ik.offsets, fit.offsets)
