"""Host checks of the split-kinematics rotation table (build_fk3_program, stac_planner.hip): P2 runs whole rounds of 16 lanes, so the
table is padded to a multiple of 16 tasks, and every padding task -- up to the area's capacity, which the 32-lane kernels' last round
reads -- is an exact no-op: it rotates the zero vector by a quaternion that exists and stores to the sink.  No GPU."""

import numpy as np
import pytest

from fk3_cases import fk3_program, lean_box, model_with_ranges, model_with_rotations


def _check_padding(info, t2, what):
    n2, nrot, cap2 = info["n2"], info["nrot"], info["cap2"]
    assert n2 % 16 == 0 and 0 <= n2 - nrot < 16, (what, n2, nrot)   # whole rounds of 16, and not one round more
    assert cap2 % 32 == 0 and cap2 >= max(n2, 32), (what, cap2, n2)  # the table behind n2 holds a whole round of 32 lanes
    assert t2.shape == (cap2, 4)
    sink, q0 = info["sink_word"], info["noop_quat_word"]
    pad = t2[nrot:]
    assert pad.shape[0] >= n2 - nrot
    assert (pad[:, :3] == 0).all(), what                             # the vector: +0.0 in every component (bits)
    assert ((pad[:, 3] & 0xFFFF) == q0).all(), what                  # the free root's quaternion: written by every pre-pass
    assert ((pad[:, 3] >> 16) == sink).all(), what                   # the result goes to the sink ...
    real = t2[:nrot]
    out = (real[:, 3] >> 16).astype(np.int64)
    assert not ((out[:, None] + np.arange(3)[None, :]) == sink).any(), what       # ... which is no real task's result,
    assert not (np.abs(out - sink) < 3).any(), what                               # and overlaps none
    assert len(set(out.tolist())) == nrot, what                      # every real task has its own slot


@pytest.mark.parametrize("model", ["rodent", "fly"])
def test_p2_is_padded_to_whole_rounds_of_16_with_exact_noops(rodent_setup, fly_setup, model):
    fs = rodent_setup if model == "rodent" else fly_setup
    full, t2 = fk3_program(fs.tables, fs.lb, fs.ub)
    assert full["fk3"] == 1
    _check_padding(full, t2, model)
    if model == "rodent":
        # 69 rotations: five rounds of 16 lanes, not three pairs; the root passes' pruned program 36: three rounds, not two pairs
        assert (full["nrot"], full["n2"]) == (69, 80)
        root, t2r = fk3_program(fs.tables, fs.lb, fs.ub, fs.trunk_kps)
        assert (root["nrot"], root["n2"]) == (36, 48)
        _check_padding(root, t2r, "rodent root passes")
        assert root["cap2"] == full["cap2"] == 96


@pytest.mark.parametrize("oriented", [False, True])
@pytest.mark.parametrize("residue", [1, 15, 16, 17, 31, 0])
def test_padding_of_random_lean_models_at_every_residue(residue, oriented):
    t, lb, ub, trunk, full, root = model_with_rotations(residue, oriented)
    assert full["nrot"] % 32 == residue and root["nrot"] % 32 != residue
    _, t2 = fk3_program(t, lb, ub)
    _check_padding(full, t2, f"residue {residue}")
    _, t2r = fk3_program(t, lb, ub, trunk)
    _check_padding(root, t2r, f"residue {residue}, root passes")
    assert root["n2"] <= root["cap2"] == full["cap2"]


def test_a_program_of_one_round_keeps_a_table_of_32_tasks():
    """A model of a few rotations: one round of 16 lanes in the 16-lane kernels, and a table that still holds the whole round a 32-lane
    kernel reads."""
    from helpers import _edge_tables

    t = _edge_tables(10, 3)
    lb, ub = lean_box(t)
    info, t2 = fk3_program(t, lb, ub)
    assert info["fk3"] == 1 and 0 < info["nrot"] <= 16 and info["n2"] == 16 and info["cap2"] == 32
    _check_padding(info, t2, "tiny")


@pytest.mark.parametrize("nrange", [16, 17])
def test_models_of_the_range_table_cases_exist(nrange):
    t, lb, ub, trunk, info = model_with_ranges(nrange)
    assert info["nrange"] == nrange and 0 <= info["rsplit"] <= nrange
