"""Host checks of the wrench-sum program of the lean 16-lane throughput kernels (build_wsum_program, stac_planner.hip): row sweeps for the
short site ranges, component tasks with a checkpoint for ranges with a common first site, whole ranges for the rest.  The program is
emulated in numpy float32 and compared bit for bit with the oracle's sum of every range -- left to right from zero -- on wrench entries
seeded with +0.0, -0.0, denormals, infinities and NaN.  No GPU."""

import json

import numpy as np
import pytest

from conftest import GOLDEN
from fk3_cases import _random_lean, fk3_program, lean_box
from wrench_sweep_cases import MAX_DEPTH, MODELS, NONE, check_program, spec_model, wsum_program

N_RANDOM = 300


def _check_layout(pr, what):
    """What the table says beyond the sums: rows of at most 16 sites that tile the sorted sites, lanes behind a row's end on the row's
    last site, store words that are a range's entry or the dump entry, a dump entry that no range sum and no site wrench lives in, and
    the LDS of a launch: what it staged before, plus the table."""
    assert pr.planned, what
    assert 0 <= pr.depth <= MAX_DEPTH and pr.nrows in ((0,) if pr.depth == 0 else (1, 2)), what
    if pr.nrows:
        rs = pr.row_start[:pr.nrows + 1]
        assert rs[0] == 0 and rs[-1] == pr.K and all(0 < b - a <= 16 for a, b in zip(rs, rs[1:])), (what, rs)
        for row in range(pr.nrows):
            want = np.minimum(rs[row] + np.arange(16), rs[row + 1] - 1) * pr.kxf
            assert (pr.rows[row, :, 0] == want).all(), (what, row)
    swept = pr.swept()
    for rid, (row, lane, s) in swept.items():
        lo, hi = pr.ranges[rid]
        assert hi - lo == s + 1 <= pr.depth and pr.row_start[row] <= lo and hi - 1 == pr.row_start[row] + lane < pr.row_start[row + 1], (what, rid)
    # the dump entry: six words that are neither a range sum's (they are read by the joints) nor a site wrench's (read by the tasks)
    d = set(range(pr.dump, pr.dump + pr.kxf))
    assert not d & set(range(pr.c_rw, pr.c_rw + pr.kxf * pr.nrange)), what
    assert not d & set(range(pr.c_sw, pr.c_sw + pr.kxf * pr.K)), what
    assert pr.c_rw + pr.kxf * pr.nrange <= pr.stride16 and pr.dump + pr.kxf <= pr.stride16, what
    # LDS: the launch stages the table in front of what it staged before, and nothing else grows
    assert pr.table_words == 4 * (pr.ntask + pr.nwhole) + 64 * pr.nrows and pr.table_words % 4 == 0, what
    assert pr.staged_words == pr.staged_words_without + pr.table_words, what
    assert pr.lds_bytes == 4 * (((pr.staged_words + 3) & ~3) + pr.mb_words + 4 * pr.stride16), what
    # every range is somebody's: swept, a task's, a checkpoint's or a whole one's (check_program asserts exactly once)
    return swept


def _fixture(name):
    from stac_mjx_amd.fit_model import finish_fit_setup
    from stac_mjx_amd.mjcf import ModelTables

    cfg = json.load(open(GOLDEN / f"{name}_model_cfg.json"))
    cfg = cfg.get("model", cfg)
    return finish_fit_setup(ModelTables.load(GOLDEN / f"{name}_tables.npz"), cfg, list(cfg["KEYPOINT_MODEL_PAIRS"].keys()))


@pytest.mark.parametrize("name", ["rodent", "fly", "synth"])
def test_fixtures_bit_equal_to_left_to_right_sums(name):
    fs = _fixture(name)
    pr = wsum_program(fs.tables, fs.lb, fs.ub)
    swept = _check_layout(pr, name)
    check_program(pr, np.random.default_rng(17), name, rounds=8)
    if name == "rodent":
        # 23 sites, 19 ranges: (0, 23) with (0, 11) as its checkpoint and (1, 11) are 12 component tasks of ONE round (they were 18, of
        # two); the 16 ranges of up to four sites are whole ranges -- or, in a build with the sweeps, two rows that no short range crosses
        assert (pr.nrange, pr.K, pr.ntask) == (19, 23, 2)
        assert pr.recs[:2].tolist() == [[0, 11, 23, 1 | 0 << 16], [1, 11, 11, 2 | 2 << 16]]
        assert (pr.nwhole, len(swept)) == ((0, 16) if pr.depth else (16, 0))
        if pr.depth:
            cut = pr.row_start[1]
            assert (pr.nrows, pr.depth) == (2, 4) and not any(lo < cut < hi for lo, hi in pr.ranges.tolist() if hi - lo <= 4)


def test_mouse_plans_nothing(mouse_setup):
    """34 sites and 181 joints: no 16-lane lean shape holds it (it runs the 32-lane kernel), so it has no program."""
    pr = wsum_program(mouse_setup.tables, mouse_setup.lb, mouse_setup.ub)
    assert not pr.planned and pr.table_words == 0 and (pr.ntask, pr.nwhole, pr.nrows, pr.depth) == (0, 0, 0, 0)


def test_planning_switch_gives_the_split_of_before(monkeypatch, rodent_setup):
    """STAC_HIP_NOWSUM: no sweeps, no checkpoints -- the first PlanHeader::rsplit ranges as component tasks, the others whole, in the
    order of the range table."""
    monkeypatch.setenv("STAC_HIP_NOWSUM", "1")
    fs = rodent_setup
    pr = wsum_program(fs.tables, fs.lb, fs.ub)
    _check_layout(pr, "rodent, switch")
    assert (pr.nrows, pr.depth, pr.ntask, pr.nwhole) == (0, 0, pr.rsplit, pr.nrange - pr.rsplit) and pr.rsplit == 3
    want = [[lo, hi, hi, r | r << 16] for r, (lo, hi) in enumerate(pr.ranges.tolist())]
    assert pr.recs.tolist() == want
    check_program(pr, np.random.default_rng(18), "rodent, switch")


# The hand-made models and what the shipped build (shared prefixes; no row sweeps: STAC_WSUM, stac_plan.hpp) must plan for them: the
# component tasks [lo, mid, hi], longest first.  A build with the sweeps plans rows as well; what holds for those is asserted where
# the program has a depth.
TASKS = {
    "prefix3": [[0, 13, 21], [13, 21, 21], [0, 8, 8], [8, 13, 13]],
    "prefix2": [[0, 16, 20], [0, 9, 9], [9, 16, 16], [16, 20, 20]],
    "one_site": [[0, 1, 1]],
    "body20": [[0, 20, 20]],
    "body32": [[0, 32, 32]],
}


@pytest.mark.parametrize("order", ["sorted", "interleaved"])
@pytest.mark.parametrize("name", list(MODELS))
def test_hand_made_models_plan_what_their_cases_are_about(name, order):
    t = spec_model(MODELS[name], order)
    lb, ub = lean_box(t)
    assert fk3_program(t, lb, ub)[0]["fk3"]
    pr = wsum_program(t, lb, ub)
    swept = _check_layout(pr, name)
    check_program(pr, np.random.default_rng(19), name)
    ranges = pr.ranges.tolist()
    if name in TASKS:
        assert pr.recs[:pr.ntask, :3].tolist() == TASKS[name] and pr.nwhole == 0 and not swept, name
    lens = sorted(int(hi - lo) for lo, hi in ranges)
    if name == "lengths":
        assert {1, 2, 3, 4, 5, 6} <= set(lens)
    if name == "prefix3":  # the root's checkpoint is A's range, 13 sites: the first site of a remainder; A1's, a third range from site 0, is a task of its own
        assert (pr.recs[0, 3] & 0xFFFF) == ranges.index([0, 13]) and (13 - 0) % 4 == 1
    if name == "prefix2":  # 16 sites: the last site of a loop trip
        assert (pr.recs[0, 3] & 0xFFFF) == ranges.index([0, 16]) and (16 - 0) % 4 == 0
    if pr.depth:  # (a build with the row sweeps)
        assert all(pr.ranges[r][1] - pr.ranges[r][0] <= pr.depth for r in swept)
        if name == "lengths":  # 1 .. 6 sites ending on one lane: four of them are that lane's captures
            assert sorted(s for r, (row, lane, s) in swept.items() if lane == 5) == [0, 1, 2, 3]
        if name == "cross16":  # (14, 18) crosses sorted position 16, the cut went elsewhere, and the range is swept
            assert ranges.index([14, 18]) in swept and pr.row_start[1] != 16
        if name == "row32":  # a range that ends on the last lane of row 0, one that starts on lane 0 of row 1
            assert swept[ranges.index([12, 16])] == (0, 15, 3) and swept[ranges.index([16, 20])] == (1, 3, 3)
        if name == "row32_cross":  # four sites, but across the only admissible cut: not a sweep's
            assert pr.row_start[1] == 16 and ranges.index([14, 18]) not in swept


def test_random_lean_models():
    """A few hundred models of the existing generator (tests/fk3_cases._random_lean): every one that the lean 16-lane kernels take has a
    program, and it is bit-equal to the left-to-right sums; the ones they do not take are counted, never skipped silently."""
    rng = np.random.default_rng(20)
    not_lean16, shapes = 0, set()
    for seed in range(N_RANDOM):
        t, _ = _random_lean(20000 + seed, 0.3 if seed % 3 == 0 else None)
        lb, ub = lean_box(t)
        pr = wsum_program(t, lb, ub)
        if not pr.planned:
            # no program: the model is not one of the split kinematics, or no 16-lane lean shape holds it (more than 80 coordinates)
            assert not fk3_program(t, lb, ub)[0]["fk3"] or t.nq > 80 or t.nsite > 32, seed
            not_lean16 += 1
            continue
        _check_layout(pr, seed)
        check_program(pr, rng, seed, rounds=1)
        shapes.add((pr.nrows, pr.depth, bool(pr.ntask), bool(pr.nwhole), bool((pr.recs[:, 1] != pr.recs[:, 2]).any())))
    assert not_lean16 < N_RANDOM / 4, not_lean16
    # the draws reach checkpoints and whole ranges, with and without component tasks
    assert any(s[4] for s in shapes) and any(s[3] for s in shapes) and {s[2] for s in shapes} == {False, True}, shapes
