"""The wrench sums of the lean 16-lane throughput kernels by the host's program -- row sweeps, component tasks with a checkpoint, whole
ranges -- on the smallest models at which each part can go wrong (tests/wrench_sweep_cases.py), against the oracle at tolerance 0.

Every launch is forced onto the lean 16-lane throughput kernel (STAC_HIP_SPEC=0, 16 lanes per chain), the kernel that ran is asserted,
every launch runs twice on its engine, and both register caps are used.  What the host planned for a model is read from the program's
info entry and asserted before the launch (the same expectations as tests/test_wrench_sweep_host.py holds without a device)."""

import numpy as np
import pytest

from fk3_cases import lean_box
from side_by_side_cases import MAXITER, TOL, case, root_solve_lengths, trunk_sites
from test_gpu_loop_head import _kw, _last_q_kernel, _part, _rodent_case, _throughput
from test_gpu_parity import _compare_phase, _np, _oracle, _q_phase_twice
from test_wrench_sweep_host import TASKS
from wrench_sweep_cases import MODELS, spec_model, wsum_program

pytestmark = pytest.mark.gpu

MIXED_TOL = 1e-2  # solver tolerance of the case with solves of different lengths (tests/test_gpu_side_by_side_rounds.py)


def _run(monkeypatch, t, lb, ub, kp, part, trunk, cap, tol=TOL, env=None):
    from stac_mjx_amd.engine import Engine

    monkeypatch.setenv("STAC_HIP_SPEC", "0")  # (read once, when the engine creates its model)
    monkeypatch.setenv("STAC_HIP_WPE", str(cap))
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    eng = Engine(t, lb, ub, tol=tol, maxiter=MAXITER, lanes_per_chain=16)
    res = _q_phase_twice(eng, kp, part_masks=part, trunk_kps=trunk, root_kp_idx=0, root_dims=7, do_root_opt=True)
    got = _last_q_kernel(eng)
    assert got == (16, 3 if (t.nq <= 48 and cap == 3) else 5, cap, 1), (t.nq, got)  # the lean 16-lane throughput kernel
    return res


def _planned(t, lb, ub, name):
    pr = wsum_program(t, lb, ub)
    assert pr.planned, name
    if name in TASKS:
        assert pr.recs[:pr.ntask, :3].tolist() == TASKS[name], name
    return pr


@pytest.mark.parametrize("cap", [3, 2])
@pytest.mark.parametrize("name", list(MODELS))
def test_models_of_each_part(monkeypatch, name, cap):
    """Range lengths 1 .. 6 on one lane; rows of 16, 17 and 32 sites with ranges on their edges, across a cut that moves and across one
    that cannot; groups of two and three ranges with a common first site, checkpoints on the last site of a trip and on the first of a
    remainder, a range of two hinges; one site, 20 and 32 sites on one body.  Sites declared in sorted order."""
    t = spec_model(MODELS[name])
    lb, ub = lean_box(t)
    _planned(t, lb, ub, name)
    trunk = trunk_sites(t.nsite, min(t.nsite, 3))
    lb, ub, kp, part, ref, _ = case(("wsum", name), t, trunk)
    _compare_phase(_run(monkeypatch, t, lb, ub, kp, part, trunk, cap), ref)


@pytest.mark.parametrize("cap", [3, 2])
@pytest.mark.parametrize("name", ["lengths", "row32", "prefix3"])
def test_sites_declared_across_the_bodies(monkeypatch, name, cap):
    """The same bodies with their sites declared round-robin, as the rodent's are: site index (the lane of the site pass) and sorted
    position (the lane of the sweep) differ, and the wrenches reach the sweep through the chain's region."""
    t = spec_model(MODELS[name], "interleaved")
    assert (np.diff(t.site_bodyid) < 0).any()
    lb, ub = lean_box(t)
    _planned(t, lb, ub, name)
    trunk = trunk_sites(t.nsite, 3)
    lb, ub, kp, part, ref, _ = case(("wsum_interleaved", name), t, trunk)
    _compare_phase(_run(monkeypatch, t, lb, ub, kp, part, trunk, cap), ref)


@pytest.mark.parametrize("cap", [3, 2])
@pytest.mark.parametrize("frames", [1, 2])
@pytest.mark.parametrize("chains", [5, 9])
def test_partly_filled_wavefronts_with_solves_of_different_lengths(monkeypatch, chains, frames, cap):
    """Five and nine chains on wavefronts of four, one and two frames, root solves that end at different trips: trips without a gradient
    pass -- and so without sweeps -- occur between trips with one, and rows of idle chains sit beside rows that sweep."""
    t = spec_model(MODELS["row32_cross"], "interleaved")
    trunk = trunk_sites(32, 5)
    lb, ub, kp, part, ref, orc = case("wsum_mixed", t, trunk, chains=9, frames=2, tol=MIXED_TOL)
    lens = root_solve_lengths(orc, t, lb, ub, kp, trunk, 4)  # (on the host, before the launch)
    assert len(set(lens)) > 1, lens
    res = _run(monkeypatch, t, lb, ub, kp[:chains, :frames], part, trunk, cap, tol=MIXED_TOL)
    _compare_phase(res, _part(ref, chains, frames))
    np.testing.assert_array_equal(_np(res["carry_qpos"]), ref["qpos"][:chains, frames - 1])


@pytest.mark.parametrize("switch", [False, True], ids=["program", "nowsum"])
def test_rodent_with_and_without_the_planning_switch(rodent_setup, rodent_mocap, monkeypatch, switch):
    """A few rodent clips on the bench's kernel, as the host plans the sums and with STAC_HIP_NOWSUM (the split of before in the
    program's form): both equal to the oracle."""
    fs = rodent_setup
    kp, ref = _rodent_case(fs, rodent_mocap)
    eng = _throughput(monkeypatch, fs, {"STAC_HIP_WPE": "3", **({"STAC_HIP_NOWSUM": "1"} if switch else {})})
    pr = wsum_program(fs.tables, fs.lb, fs.ub)  # (the environment's switches are read by the call)
    assert (pr.ntask, pr.recs[0, 1] != pr.recs[0, 2]) == ((3, False) if switch else (2, True))
    res = _q_phase_twice(eng, kp[:5, :2], **_kw(fs))
    assert _last_q_kernel(eng) == (16, 5, 3, 1)
    _compare_phase(res, _part(ref, 5, 2))


@pytest.mark.parametrize("switch", [False, True], ids=["program", "nowsum"])
def test_fly_with_and_without_the_planning_switch(fly_setup, monkeypatch, switch):
    """Tethered fly (no root optimisation; its sites are declared in sorted order), three chains of two frames."""
    fly = fly_setup
    orc = _oracle(fly, tol=TOL, maxiter=MAXITER)
    rng = np.random.default_rng(12)
    qt = fly.tables.qpos0[None] + np.clip(rng.normal(0, 0.1, (6, fly.tables.nq)), -0.2, 0.2).astype(np.float32)
    qt[:, 3:7] = fly.tables.qpos0[3:7]
    kp = np.stack([orc.fk(q)["site_xpos"].reshape(-1) for q in qt]).reshape(3, 2, 3 * fly.tables.nsite)
    kp = (kp + rng.normal(0, 1e-3, kp.shape)).astype(np.float32)
    eng = _throughput(monkeypatch, fly, {"STAC_HIP_NOWSUM": "1"} if switch else {})
    pr = wsum_program(fly.tables, fly.lb, fly.ub)
    assert pr.planned and bool((pr.recs[:, 1] != pr.recs[:, 2]).any()) == (not switch)
    res = _q_phase_twice(eng, kp, part_masks=fly.part_masks)
    got = _last_q_kernel(eng)
    assert got[0] == 16 and got[3] == 1, got
    _compare_phase(res, orc.ik_clips(kp, fly.lb, fly.ub, fly.part_masks, fly.trunk_kps, 0, 7, do_root_opt=False))
