"""Tree-shape edges of the q_phase plans on the host, and the C. elegans config's facts -- CPU only.

The models of tests/tree_cases.py sit on the limits the host planner decides by; what is asserted here is what the GPU module
(tests/test_gpu_tree_shapes.py) relies on when it names a case "full P3" or "width G + 1":
  * the split-kinematics program sizes (stac_debug_fk3_program: plan construction, no device) of serial chains, number for number:
    n3 = 252 is the last P3 table build_fk3_program accepts (84 hinge bodies with offsets and anchors), n1 = 254 the last P1 table
    (127 oriented hinge bodies); one body more and the model silently leaves the lean kernels (fk3 = 0);
  * a chain of 73 hinges (nq = 80: what the 16-lane lean shapes hold) with 33 jointless spacer bodies has n3 = 252 as well, 34 fall out;
  * the root passes' pruned programs of those chains;
  * max_width -- restated in Python from build_plan -- of every width case of the GPU module;
  * the oracle on these shapes against the independent float64 statement tests/kin_ref.py, and the float64 twin's gradient against
    central differences of its own loss.

Measured on chain(84), chain(249, zero_jnt_pos), chain(127, oriented), star(65) and C. elegans, 8 poses each (qpos0 + N(0, 0.4)):
  float64 twin vs kin_ref.fk     max 1.19e-7 (chain127; bound 2^-23 max(|ref|, 1) per element, derived)
  float32 oracle vs kin_ref.fk   chain84 9.55e-7 (bound 9.4e-5), chain249 2.55e-6 at 250 levels (bound 4.9e-4), chain127 1.48e-6
                                 (3.1e-4), star65 2.15e-7 (4.8e-6), C. elegans 4.22e-7 (2.6e-5): every model, the 250-level chain
                                 included, is inside test_gpu_boundaries._fk_tol (16 ulp per level, derived), so that bound is the
                                 one asserted at every depth and no measured value stands in for it
  q_loss gradient vs central differences (h = 1e-4), relative to max(1, |g|): at most 5.0e-7 (chain127), asserted at 5e-6 as in
                                 tests/test_oracle.py

Mutations that turn tests of this file red (checked on a scratch copy of the tree, CPU):
  * `n3 > 252` relaxed to `n3 > 256` in build_fk3_program: on its own this changes NOTHING and every test stays green -- build_plan
    probes the program with cap3 = 252 (`build_fk3_program(m, g, nullptr, 254, 4096, 252, probe)`), and `n3 > cap3` in the same
    line holds the same limit.  With that probe cap relaxed to 256 as well, test_program_sizes_of_serial_chains[chain85] (a program
    instead of fk3 = 0) and test_spacer_chain_fills_p3_inside_the_16_lane_shapes (37 spacers instead of 33) fail.  The limit is
    stated twice in the host; the tests hold the pair;
  * max_width over all bodies instead of the active ones (the default of tree_cases.max_width turned to all_bodies=True): the three
    `idle` cases of test_widths fail (fixed_star(8, idle=1): 9 instead of 8).
"""

import json

import numpy as np
import pytest

import kin_ref
import tree_cases as tc
from conftest import GOLDEN
from fk3_cases import fk3_program, lean_box
from test_gpu_boundaries import _fk_tol
from test_gpu_tree_shapes import WIDTH_CASES, celegans_fit_setup
from test_oracle import _fd_grad

SIZES = ("fk3", "n1", "n2", "n3", "nrot")


def _sizes(info):
    return tuple(info[k] for k in SIZES) if info["fk3"] else (0,)


@pytest.mark.parametrize("row", tc.PROGRAM_ROWS, ids=[r[0] for r in tc.PROGRAM_ROWS])
def test_program_sizes_of_serial_chains(row):
    name, make, nq, want = row
    t = make()
    assert t.nq == nq and tc.max_width(t) == 1 and tc.path_depth(t) == t.nbody - 1
    info, _ = fk3_program(t, *lean_box(t))
    print(name, {k: info[k] for k in SIZES})
    assert _sizes(info) == want, (name, info)


def test_spacer_chain_fills_p3_inside_the_16_lane_shapes():
    """73 hinge bodies (3 rotations each: body_pos, anchor, position) and 33 spacers (one each): 252 rotations, n3 = 252, at
    nq = 80; the 34th spacer is a 253rd rotation, n3 = 256: no program."""
    s, t, info = tc.spacer_chain_full_p3()
    assert (s, t.nq, t.nbody) == (33, 80, 2 + tc.SPACER_D + 33)
    assert _sizes(info) == (1, 74, 256, 252, 252), info
    over = tc.chain(tc.SPACER_D, spacers=s + 1)
    assert over.nq == 80 and _sizes(fk3_program(over, *lean_box(over))[0]) == (0,)


DEPTH_MODELS = [r for r in tc.PROGRAM_ROWS if r[3][0]] + [("spacer73", lambda: tc.spacer_chain_full_p3()[1], 80, None)]


@pytest.mark.parametrize("row", DEPTH_MODELS, ids=[r[0] for r in DEPTH_MODELS])
def test_pruned_root_programs(row):
    """The root passes evaluate the ancestors of the trunk keypoints only.  A trunk of the last site needs the whole chain (the pruned
    program is as large as the full one, never larger); a trunk of the first site -- on the root body -- needs that body alone and
    no product and no rotation at all."""
    name, make, _, _ = row
    t = make()
    lb, ub = lean_box(t)
    full, _ = fk3_program(t, lb, ub)
    first, last = np.zeros(t.nsite, np.uint8), np.zeros(t.nsite, np.uint8)
    first[0], last[-1] = 1, 1
    for trunk, nneed in ((last, full["nab"]), (first, 1)):
        root, _ = fk3_program(t, lb, ub, trunk)
        assert root["fk3"] == 1 and 0 < root["nneed"] <= root["nab"] == full["nab"] and root["nneed"] == nneed, (name, root)
        for k in ("n1", "n2", "n3", "nrot"):
            assert root[k] <= full[k], (name, k, root, full)
        assert root["n2"] <= full["cap2"] and root["cap2"] == full["cap2"]
        if nneed == 1:
            assert (root["n1"], root["n2"], root["n3"], root["nrot"]) == (0, 0, 0, 0)
        else:
            assert _sizes(root) == _sizes(full)
    two, _ = fk3_program(t, lb, ub, tc.trunk_two(t))  # the trunk the GPU cases run with
    assert _sizes(two) == _sizes(full)


@pytest.mark.parametrize("case", WIDTH_CASES, ids=[c[0] for c in WIDTH_CASES])
def test_widths(case):
    """max_width of every width case, and where the case stands against its lane count: fk_chain runs fk_program_quad when
    4 * max_width <= G, fk_program when max_width <= G, fk_levels beyond."""
    name, make, lanes, width = case[:4]
    t = make()
    assert tc.max_width(t) == width, (name, tc.max_width(t))
    d = tc.active_depths(t)
    assert set(d) == tc.active_bodies(t) and min(d.values()) == 1
    if "idle" in name:  # a leaf without a site is no active body: the widest level over ALL bodies is wider
        assert tc.max_width(t, all_bodies=True) > width
    else:
        assert tc.active_bodies(t) == set(range(1, t.nbody))  # every body is the ancestor of a site


def test_width_cases_stand_on_every_side_of_the_lane_count():
    have = {(c[2], c[3]) for c in WIDTH_CASES if c[0].startswith("fixed")}
    for G in (8, 16, 32, 64):
        for w in (G // 4, G // 4 + 1, G, G + 1, 2 * G + 1):
            assert (G, w) in have, (G, w)
    assert {4, 5} <= {c[3] for c in WIDTH_CASES}


# ---- the oracle on these shapes ----------------------------------------------------------------------------------------------------
ORACLE_MODELS = {
    "chain84": lambda: tc.chain(84), "chain249": lambda: tc.chain(249, zero_jnt_pos=True),
    "chain127-oriented": lambda: tc.chain(127, oriented=True), "star65": lambda: tc.star(65),
    "celegans": lambda: celegans_fit_setup()[0].tables,
}
ARRAYS = ("xpos", "xquat", "site_xpos")


@pytest.mark.parametrize("model", list(ORACLE_MODELS))
def test_oracle_kinematics_and_gradient_on_deep_and_wide_trees(model):
    from oracle import Oracle

    t = ORACLE_MODELS[model]()
    rng = np.random.default_rng(1300 + list(ORACLE_MODELS).index(model))
    q = (np.asarray(t.qpos0, np.float32)[None] + rng.normal(0, 0.4, (8, t.nq))).astype(np.float32)
    o32, o64 = Oracle(t), Oracle(t, precision="f64")
    depth = tc.path_depth(t)
    assert depth == int(np.asarray(t.body_depth).max())
    dev32 = dev64 = scale = 0.0
    for x in q:
        ref = dict(zip(ARRAYS, kin_ref.fk(t, x)))
        r32, r64 = o32.fk(x.copy()), o64.fk(x.copy())
        for k in ARRAYS:
            d64 = np.abs(r64[k].astype(np.float64) - ref[k])
            assert (d64 <= 2.0 ** -23 * np.maximum(np.abs(ref[k]), 1.0)).all(), (model, k, d64.max())
            dev64 = max(dev64, d64.max())
            dev32 = max(dev32, np.abs(r32[k].astype(np.float64) - ref[k]).max())
            scale = max(scale, np.abs(ref[k]).max())
    tol = _fk_tol(depth, scale)
    print(f"{model}: depth {depth}, |x| <= {scale:.3g}: float64 twin {dev64:.3g}, float32 oracle {dev32:.3g} (bound {tol:.3g})")
    assert dev32 <= tol, (model, dev32, tol)
    # the float64 twin's analytic gradient against central differences of its own loss
    x = q[0]
    kp = rng.normal(0, 0.3, 3 * t.nsite).astype(np.float32)
    qs, ks = np.ones(t.nq, bool), np.ones(3 * t.nsite, bool)
    _, g = o64.q_loss(x, kp, qs, ks, x)
    gfd = _fd_grad(o64, x, kp, qs, ks)
    print(f"{model}: gradient vs central differences {np.abs(g - gfd).max():.3g} at |g| <= {np.abs(g).max():.3g}")
    assert np.all(g != 0)  # every coordinate moves a site
    assert np.abs(g - gfd).max() <= 5e-6 * max(1.0, np.abs(g).max())


# ---- the C. elegans config -----------------------------------------------------------------------------------------------------------
def test_celegans_facts():
    """configs/model/celegans.yaml on models/celegans/celegans.xml, from the committed fixture: what makes it unlike the four
    configs that have a test."""
    from stac_mjx_amd.mjcf import JNT_FREE, JNT_HINGE

    fs, cfg = celegans_fit_setup()
    t, cfgm = fs.tables, cfg["model"]
    assert (t.nbody, t.njnt, t.nq, t.nsite) == (26, 25, 31, 25)
    assert (JNT_FREE, JNT_HINGE) == (0, 3) and t.jnt_type.tolist() == [0] + [3] * 24
    assert t.body_depth.tolist() == list(range(26)) and t.body_parentid.tolist() == [0] + list(range(25))
    np.testing.assert_array_equal(t.jnt_axis[1:], np.tile(np.array([0, 0, 1], np.float32), (24, 1)))
    assert fs.part_masks.shape == (5, 31) and fs.part_masks.sum(1).tolist() == [0, 0, 0, 0, 0]
    assert fs.root_kp_idx == -1 and not fs.do_root_opt and int(fs.trunk_kps.sum()) == 0 and fs.root_dims == 7
    assert int(fs.is_regularized.sum()) == 0 and float(np.abs(t.site_pos).max()) == 0.0
    assert not (t.body_quat[1:] != np.array([1, 0, 0, 0], np.float32)).any()  # no oriented body
    assert t.site_bodyid.tolist() == list(range(1, 26))  # one site on every body, at its origin
    bounds = np.unique(t.jnt_range[1:], axis=0)
    np.testing.assert_array_equal(bounds, np.array([[-1.7453293, 1.7453293], [-1.2217305, 1.2217305]], np.float32))
    np.testing.assert_array_equal(fs.lb[7:], t.jnt_range[1:, 0])
    np.testing.assert_array_equal(fs.ub[7:], t.jnt_range[1:, 1])
    assert "ROOT_OPTIMIZATION_KEYPOINT" not in cfgm and cfgm["TRUNK_OPTIMIZATION_KEYPOINTS"] == [] and cfgm["SITES_TO_REGULARIZE"] == []
    assert (cfgm["FTOL"], cfgm["N_ITER_Q"], cfgm["N_ITERS"], cfgm["N_SAMPLE_FRAMES"], cfgm["M_REG_COEF"]) == (5e-3, 400, 6, 100, 1)
    assert len(cfgm["INDIVIDUAL_PART_OPTIMIZATION"]) == 5 and not set(sum(cfgm["INDIVIDUAL_PART_OPTIMIZATION"].values(), [])) & set(t.jnt_names)
    stac = cfg["stac"]
    assert (stac["n_fit_frames"], stac["skip_ik_only"], stac["n_frames_per_clip"], stac["infer_qvels"]) == (500, True, 250, True)
    assert stac["n_fit_frames"] > cfgm["N_SAMPLE_FRAMES"] and "data_path" not in stac
    info, _ = fk3_program(t, fs.lb, fs.ub)
    print("celegans program:", {k: info[k] for k in SIZES + ("nrange",)})
    assert (info["fk3"], info["n1"]) == (1, 24)
    assert (info["n2"], info["n3"], info["nrot"], info["nrange"]) == (80, 72, 70, 25)
    assert tc.max_width(t) == 1 and tc.path_depth(t) == 25


def test_celegans_fixture_is_settings_only():
    c = json.load(open(GOLDEN / "celegans_model_cfg.json"))
    assert set(c) == {"model", "stac"} and c["model"]["MJCF_PATH"] == "models/celegans/celegans.xml"
