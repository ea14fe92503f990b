"""The solver transition of the lean throughput kernels -- the nq-sums of the line-search step, the accept that takes the candidate of
the sums, the stopping residual that a chain in ST_VG_X shares with the fused chains, literal zeros for the padding registers of the
trees -- on the smallest cases at which each can go wrong (tests/transition_cases.py), against the oracle at tolerance 0.

Every launch is forced onto the lean 16-lane throughput kernel (STAC_HIP_SPEC=0, 16 lanes per chain), the kernel that ran is asserted,
every launch runs twice on its engine, and both register caps are used.  What a case is meant to reach -- a line search that takes its
first candidate, a step taken without evaluation, coordinates on both sides of the box, root solves of different lengths -- is read
from the oracle's counters and answer on the host and asserted before the launch."""

import numpy as np
import pytest

from side_by_side_cases import MAXITER, TOL, hinge_model, root_solve_lengths, trunk_sites
from test_gpu_loop_head import _kw, _last_q_kernel, _part, _rodent_case, _throughput
from test_gpu_parity import _compare_phase, _np, _oracle, _q_phase_twice
from transition_cases import EDGE_HINGES, edge_model, forced_frames, single_evaluation_iterations, trans_case

pytestmark = pytest.mark.gpu

MIXED_TOL = 1e-2  # solver tolerance of the case with solves of different lengths (tests/test_gpu_side_by_side_rounds.py)


def _run(monkeypatch, t, lb, ub, kp, part, trunk, cap, tol=TOL, maxls=15):
    from stac_mjx_amd.engine import Engine

    monkeypatch.setenv("STAC_HIP_SPEC", "0")  # (read once, when the engine creates its model)
    monkeypatch.setenv("STAC_HIP_WPE", str(cap))
    eng = Engine(t, lb, ub, tol=tol, maxiter=MAXITER, maxls=maxls, lanes_per_chain=16)
    res = _q_phase_twice(eng, kp, part_masks=part, trunk_kps=trunk, root_kp_idx=0, root_dims=7, do_root_opt=True)
    got = _last_q_kernel(eng)
    assert got == (16, 3 if (t.nq <= 48 and cap == 3) else 5, cap, 1), (t.nq, got)  # the lean 16-lane throughput kernel
    return res


@pytest.mark.parametrize("cap", [3, 2])
@pytest.mark.parametrize("hinges", EDGE_HINGES)
def test_register_and_lane_edges(monkeypatch, hinges, cap):
    """nq = 8, 16, 17, 32, 48, 49 and 80: a last register partly filled, whole registers of padding (which the trees take as literal
    zeros), the boundary between the three- and the five-register kernels, every lane holding a coordinate in every register."""
    t = edge_model(hinges)
    assert t.nq == hinges + 7
    trunk = trunk_sites(t.nsite, 3)
    lb, ub, kp, part, ref, _ = trans_case(("edge", hinges), t, trunk)
    _compare_phase(_run(monkeypatch, t, lb, ub, kp, part, trunk, cap), ref)


@pytest.mark.parametrize("cap", [3, 2])
@pytest.mark.parametrize("chains", [1, 4, 5])
@pytest.mark.parametrize("hinges", [10, 25])
def test_first_candidate_accepted_next_trip_evaluates_x(monkeypatch, hinges, chains, cap):
    """Part solves over hinges alone: their line searches take the first candidate in some iterations (asserted from the oracle's
    counters: fewer than two evaluations per iteration on a frame's sum).  One chain alone in its wavefront has no neighbour whose
    gradient pass the candidate could share, so the trip after the accept is ST_VG_X and its stopping residual comes from the block
    of the fused chains; four and five chains put that state beside the others inside a wavefront."""
    t = hinge_model(hinges, 12, seed=0)
    trunk = trunk_sites(12, 3)
    lb, ub, kp, part, ref, _ = trans_case(("vgx", hinges), t, trunk, root_in_parts=False)
    single = single_evaluation_iterations(ref["counters"])
    assert single[0].all() and single[:chains].sum() >= min(chains, 3), single.tolist()
    res = _run(monkeypatch, t, lb, ub, kp[:chains], part, trunk, cap)
    _compare_phase(res, _part(ref, chains, 2))


@pytest.mark.parametrize("cap", [3, 2])
@pytest.mark.parametrize("chains", [1, 5])
@pytest.mark.parametrize("maxls", [1, 2])
def test_steps_taken_without_evaluation(monkeypatch, maxls, chains, cap):
    """`maxls` = 1 and 2: a line search that has rejected `maxls` candidates takes the next one, at the halved step, without evaluating it
    -- the one accept whose point is not the candidate of the sums -- and the next trip is ST_VG_X, in root solves (the short
    transition of a root fast trip) and in the others.  That it happens in the chains launched is asserted from the counters of the
    same keypoints under the default limit.  (Twelve keypoints at `maxls` = 2.  At `maxls` = 1 every step is the half of the one
    before or a doubled one, which no solve over the root's position survives with more than one keypoint -- the oracle's answer
    is NaN --; with one keypoint the oracle's answer stays finite, if large, and that model is used.)"""
    hinges, sites, ntrunk = ((10, 1, 1), (25, 12, 3))[maxls - 1]
    t = hinge_model(hinges, sites, seed=1)
    trunk = trunk_sites(sites, ntrunk)
    free = trans_case(("forced", maxls, 15), t, trunk, data=("forced", maxls))[4]["counters"]
    forced = forced_frames(free, maxls).any(axis=1)
    assert forced[0] and forced[:chains].sum() >= min(chains, 4), forced.tolist()
    lb, ub, kp, part, ref, _ = trans_case(("forced", maxls), t, trunk, maxls=maxls, data=("forced", maxls))
    assert (ref["counters"] != free).any() and np.isfinite(ref["qpos"]).all() and np.isfinite(ref["frame_error"]).all()
    res = _run(monkeypatch, t, lb, ub, kp[:chains], part, trunk, cap, maxls=maxls)
    _compare_phase(res, _part(ref, chains, 2))


@pytest.mark.parametrize("cap", [3, 2])
@pytest.mark.parametrize("hinges", [10, 42])
def test_both_sides_of_the_box_bind(monkeypatch, hinges, cap):
    """Keypoints generated from poses below and above the box: the clip binds on either side in the candidates and in the stopping
    residual, and the answer has coordinates on both bounds (asserted on the oracle's answer)."""
    t = hinge_model(hinges, 12, seed=4)
    trunk = trunk_sites(12, 3)
    lb, ub, kp, part, ref, _ = trans_case(("outside", hinges, 4), t, trunk, outside=True)
    q = ref["qpos"][..., 7:]
    assert (q == lb[7:]).any() and (q == ub[7:]).any()
    _compare_phase(_run(monkeypatch, t, lb, ub, kp, part, trunk, cap), ref)


@pytest.mark.parametrize("cap", [3, 2])
@pytest.mark.parametrize("chains", [5, 9])
def test_solves_ending_at_different_trips(monkeypatch, chains, cap):
    """The mixed-tolerance case of the side-by-side tests: root solves of different lengths (asserted on the host), so chains in ST_WAIT
    and ST_DONE sit beside live ones, root fast trips (the short transition) alternate with full ones, and the last wavefront is
    partly filled."""
    t = hinge_model(25, 12, seed=3)
    trunk = trunk_sites(12, 5)
    lb, ub, kp, part, ref, orc = trans_case("mixed", t, trunk, chains=9, frames=2, tol=MIXED_TOL)
    lens = root_solve_lengths(orc, t, lb, ub, kp, trunk, 4)
    assert len(set(lens)) > 1, lens
    res = _run(monkeypatch, t, lb, ub, kp[:chains], part, trunk, cap, tol=MIXED_TOL)
    _compare_phase(res, _part(ref, chains, 2))
    np.testing.assert_array_equal(_np(res["carry_qpos"]), ref["qpos"][:chains, 1])


@pytest.mark.parametrize("cap", [3, 2])
def test_rodent_clips(rodent_setup, rodent_mocap, monkeypatch, cap):
    """A few rodent clips on the bench's kernel (register cap 3) and on its uncapped twin."""
    fs = rodent_setup
    kp, ref = _rodent_case(fs, rodent_mocap)
    eng = _throughput(monkeypatch, fs, {"STAC_HIP_WPE": str(cap)})
    res = _q_phase_twice(eng, kp[:5, :2], **_kw(fs))
    assert _last_q_kernel(eng) == (16, 5, cap, 1)
    _compare_phase(res, _part(ref, 5, 2))


def test_tethered_fly(fly_setup, monkeypatch):
    """Tethered fly (43 coordinates, no root optimisation) on the three-register kernel: three chains of two frames."""
    fly = fly_setup
    orc = _oracle(fly, tol=TOL, maxiter=MAXITER)
    rng = np.random.default_rng(12)
    qt = fly.tables.qpos0[None] + np.clip(rng.normal(0, 0.1, (6, fly.tables.nq)), -0.2, 0.2).astype(np.float32)
    qt[:, 3:7] = fly.tables.qpos0[3:7]
    kp = np.stack([orc.fk(q)["site_xpos"].reshape(-1) for q in qt]).reshape(3, 2, 3 * fly.tables.nsite)
    kp = (kp + rng.normal(0, 1e-3, kp.shape)).astype(np.float32)
    eng = _throughput(monkeypatch, fly, {"STAC_HIP_WPE": "3"})
    res = _q_phase_twice(eng, kp, part_masks=fly.part_masks)
    assert _last_q_kernel(eng) == (16, 3, 3, 1)
    _compare_phase(res, orc.ik_clips(kp, fly.lb, fly.ub, fly.part_masks, fly.trunk_kps, 0, 7, do_root_opt=False))
