"""The rounds of lanes that the lean throughput kernels run side by side -- the joint-local pre-pass (three pinned rounds, then the
unpinned remainder loop), the joint gradients (records of three rounds, data of two and of one), the site pass (two rounds) -- and the
batched wrench sum of a root fast trip: the smallest models at which each part can go wrong, against the oracle at tolerance 0.

Every launch is forced onto the throughput kernel (STAC_HIP_SPEC=0), the kernel that ran is asserted, and every launch runs twice on
its engine (a value read before it is written shows in the second run).  Models: tests/side_by_side_cases.py."""

import numpy as np
import pytest

from side_by_side_cases import MAXITER, TOL, case, hinge_model, root_solve_lengths, trunk_sites
from test_gpu_loop_head import _kw, _last_q_kernel, _part, _rodent_case, _throughput
from test_gpu_parity import _compare_phase, _np, _q_phase_twice

pytestmark = pytest.mark.gpu

MIXED_TOL = 1e-2  # solver tolerance of the case with solves of different lengths


def _run(monkeypatch, t, lb, ub, kp, part, trunk, do_root_opt=True, tol=TOL, cap=3):
    from stac_mjx_amd.engine import Engine

    """A launch on the lean 16-lane throughput kernel at the register cap of three wavefronts per SIMD, as a batch that fills the chip
    runs it (cap 3; a few chains alone would get the variant of two per SIMD: cap 2, always five solver registers per lane)."""
    monkeypatch.setenv("STAC_HIP_SPEC", "0")  # (read once, when the engine creates its model)
    monkeypatch.setenv("STAC_HIP_WPE", str(cap))
    eng = Engine(t, lb, ub, tol=tol, maxiter=MAXITER, lanes_per_chain=16)
    res = _q_phase_twice(eng, kp, part_masks=part, trunk_kps=trunk, root_kp_idx=0, root_dims=7, do_root_opt=do_root_opt)
    got = _last_q_kernel(eng)
    # up to 48 coordinates (41 hinges) three solver registers per lane, beyond that five
    assert got == (16, 3 if (t.nq <= 48 and cap == 3) else 5, cap, 1), (t.nq, got)
    return res


@pytest.mark.parametrize("hinges", [1, 15, 16, 17, 31, 32, 33, 47, 48, 49])
def test_hinge_counts_at_the_edges_of_the_rounds(monkeypatch, hinges):
    """1 + 16 u hinges fill u rounds of lanes behind the free root: one hinge (rounds two and three are all duplicates of it), the last
    lane of each pinned round, its first duplicate lane and the first lane of the next round (15, 16, 17; 31, 32, 33; 47, 48), and the
    first joint of the unpinned remainder loop (49).  The gradient pass has the same rounds (two together, then one)."""
    t = hinge_model(hinges, 12, seed=1)
    trunk = trunk_sites(12, 4)
    lb, ub, kp, part, ref, _ = case(("hinges", hinges), t, trunk)
    _compare_phase(_run(monkeypatch, t, lb, ub, kp, part, trunk), ref)


@pytest.mark.parametrize("sites", [1, 15, 16, 17, 31, 32])
def test_site_counts_of_one_and_two_rounds(monkeypatch, sites):
    """One round of sites (1, 15, 16: its only, its last-but-one and its last lane) and two (17, 31, 32: the second round's first,
    last-but-one and last lane); the lanes without a site read the last site's body again and store nothing."""
    t = hinge_model(20, sites, seed=2)
    trunk = trunk_sites(sites, min(sites, 3))
    lb, ub, kp, part, ref, _ = case(("sites", sites), t, trunk)
    _compare_phase(_run(monkeypatch, t, lb, ub, kp, part, trunk), ref)


@pytest.mark.parametrize("count,one_body", [(1, False), (3, False), (4, False), (5, False), (8, False), (9, False), (32, False), (5, True)],
                         ids=["1", "3", "4", "5", "8", "9", "32", "5_on_one_body"])
def test_trunk_keypoint_counts_at_the_batch_edges_of_the_root_sum(monkeypatch, count, one_body):
    """32 sites, of which 1 ... 32 are trunk keypoints (site 0 and site 31 always: the first and the last bit of the mask): batches of
    eight with seven, five, four, three and no padding reads, a second batch of one, four full batches; once all sites on one body."""
    t = hinge_model(20, 32, seed=3, one_body=one_body)
    trunk = trunk_sites(32, count, seed=count) if count > 1 else np.eye(32, dtype=np.uint8)[0]
    if count > 1:
        assert trunk[0] and trunk[31]
    if one_body:
        assert len(set(t.site_bodyid.tolist())) == 1
    assert int(trunk.sum()) == count
    lb, ub, kp, part, ref, _ = case(("trunk", count, one_body), t, trunk)
    _compare_phase(_run(monkeypatch, t, lb, ub, kp, part, trunk), ref)


@pytest.mark.parametrize("cap", [3, 2])
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("chains", [5, 9])
def test_chains_whose_root_solves_differ_in_length(monkeypatch, chains, frames, cap):
    """Partly filled wavefronts of four chains whose root solves end at different trips: root fast trips and full trips alternate, chains
    wait for their neighbours, and trips in which no chain wants a gradient occur (the site pass without its stores).  The solver's
    tolerance is 1e-2 here: at 1e-4 every root solve of these models runs to the iteration bound, and all would be of one length.
    On both register caps of the kernel (`<16,3,3,1>` and `<16,5,2,1>`: the same source, another allocation)."""
    t = hinge_model(33, 17, seed=4)
    trunk = trunk_sites(17, 5)
    lb, ub, kp, part, ref, orc = case("mixed", t, trunk, chains=9, frames=3, tol=MIXED_TOL)
    lens = root_solve_lengths(orc, t, lb, ub, kp, trunk, 4)  # (on the host, before the launch)
    assert len(set(lens)) > 1, lens
    res = _run(monkeypatch, t, lb, ub, kp[:chains, :frames], part, trunk, tol=MIXED_TOL, cap=cap)
    _compare_phase(res, _part(ref, chains, frames))
    np.testing.assert_array_equal(_np(res["carry_qpos"]), ref["qpos"][:chains, frames - 1])


def test_no_root_optimisation(monkeypatch):
    """do_root_opt false: full trips only, no pruned program behind the site pass's records."""
    t = hinge_model(33, 17, seed=4)
    trunk = trunk_sites(17, 5)
    lb, ub, kp, part, ref, _ = case("no_root", t, trunk, do_root_opt=False)
    _compare_phase(_run(monkeypatch, t, lb, ub, kp, part, trunk, do_root_opt=False), ref)


@pytest.mark.parametrize("env,lean", [({}, 1), ({"STAC_HIP_WPE": "3"}, 1), ({"STAC_HIP_NOLEAN": "1"}, 0)], ids=["as_planned", "cap_3", "generic"])
def test_rodent_nine_clips(rodent_setup, rodent_mocap, monkeypatch, env, lean):
    """The bench's model (38 hinges: three pinned rounds, the last of six lanes; 23 sites; eight trunk keypoints: one batch), nine clips of
    three frames, on the kernel the host plans (`<16,5,2,1>` for so few chains), on the bench's `<16,5,3,1>` and on the generic kernel,
    whose code is the round-by-round one."""
    fs = rodent_setup
    kp, ref = _rodent_case(fs, rodent_mocap)
    eng = _throughput(monkeypatch, fs, env)
    res = _q_phase_twice(eng, kp, **_kw(fs))
    got = _last_q_kernel(eng)
    assert got[0] == 16 and got[3] == lean and (not lean or got[:3] == (16, 5, 3 if env else 2)), got
    _compare_phase(res, _part(ref, 9, 3))
    np.testing.assert_array_equal(_np(res["carry_qpos"]), ref["qpos"][:, 2])
