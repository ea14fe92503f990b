"""The head of a trip of the throughput kernel -- the launch-wide decisions behind the pinned control word (hand-off armed, chain queue
with root fast trips, root_fast, the pruned program's counts), the staging and the free root's pre-pass out of a 16-lane row -- on the
smallest launches that reach each path, against the oracle at tolerance 0 (outputs only)."""

import json

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_parity import _compare_phase, _engine, _np, _oracle, _q_phase_twice

pytestmark = pytest.mark.gpu

MAXITER, TOL = 30, 1e-4
# nine rodent clips of three frames from recordings far apart, in an order that puts root solves of different lengths into one wavefront
STARTS = (300, 0, 500, 400, 200, 700, 100, 600, 800)
_REF = {}


def _last_q_kernel(eng):
    import ctypes

    out = (ctypes.c_int32 * 4)()
    eng.lib.stac_debug_last_q_kernel(out)
    return tuple(out)


def _kw(fs, do_root_opt=True):
    return dict(part_masks=fs.part_masks, trunk_kps=fs.trunk_kps, root_kp_idx=fs.root_kp_idx, root_dims=fs.root_dims, do_root_opt=do_root_opt)


def _rodent_case(fs, mocap, maxiter=MAXITER, do_root_opt=True, q_init=None, key="rodent"):
    """Nine clips of three frames and the oracle's answer, computed once per (key, maxiter, root pass) and never changed: a launch of
    n <= 9 chains and F <= 3 frames is checked against the leading part (chains are independent, frames run in order)."""
    k = (key, maxiter, do_root_opt)
    if k not in _REF:
        kp = np.stack([mocap[s:s + 3] for s in STARTS]).reshape(9, 3, 69)
        ref = _oracle(fs, tol=TOL, maxiter=maxiter).ik_clips(kp, fs.lb, fs.ub, fs.part_masks, fs.trunk_kps, fs.root_kp_idx, fs.root_dims,
                                                            do_root_opt=do_root_opt, q_init=q_init)
        _REF[k] = (kp, ref)
    return _REF[k]


def _part(ref, n, F):
    return {k: (v[:n, :F] if v is not None else None) for k, v in ref.items()}


def _throughput(monkeypatch, fs, env=None, maxiter=MAXITER, lanes=16):
    for k, v in {"STAC_HIP_SPEC": "0", **(env or {})}.items():
        monkeypatch.setenv(k, v)  # (read once, when the engine creates its model)
    return _engine(fs, tol=TOL, maxiter=maxiter, lanes_per_chain=lanes)


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("chains", [1, 3, 4, 5, 9])
def test_chain_counts_and_frames_on_the_lean_throughput_kernel(rodent_setup, rodent_mocap, monkeypatch, chains, frames):
    """Partly filled groups and wavefronts (1, 3, 5 and 9 chains on wavefronts of four), chains of one wavefront that leave their root
    solves at different trips (lite and full trips alternate, ST_WAIT is entered), next frames behind the pinned control word."""
    fs = rodent_setup
    kp, ref = _rodent_case(fs, rodent_mocap)
    if "root_evals" not in _REF:  # (on the host, before the launch: the root solves of the first wavefront's chains differ in length)
        orc = _oracle(fs, tol=TOL, maxiter=MAXITER)
        ev = []
        for c in range(4):
            st = orc.root_optimization(kp[c], fs.tables.qpos0, fs.lb, fs.ub, fs.trunk_kps, fs.root_kp_idx, fs.root_dims)[1]
            ev.append(st["ls_evals"] + st["grad_evals"])
        _REF["root_evals"] = ev
    assert len(set(_REF["root_evals"][:3])) > 1, _REF["root_evals"]
    eng = _throughput(monkeypatch, fs)
    res = _q_phase_twice(eng, kp[:chains, :frames], **_kw(fs))
    got = _last_q_kernel(eng)
    assert got[:2] == (16, 5) and got[3] == 1, got  # the lean 16-lane throughput kernel
    _compare_phase(res, _part(ref, chains, frames))
    np.testing.assert_array_equal(_np(res["carry_qpos"]), ref["qpos"][:chains, frames - 1])


@pytest.mark.parametrize("variant", ["queue", "handoff", "queue_handoff"])
def test_launch_variants_behind_the_control_word(rodent_setup, rodent_mocap, monkeypatch, variant):
    """The chain queue forced (four slots for nine chains: the groups of a wavefront take their next chains together), the hand-off
    forced at a threshold of one finished chain (the other eight go to the latency kernel: the resume launch is the call's last), both."""
    env = {"queue": {"STAC_HIP_QUEUE": "4", "STAC_HIP_WPB": "1", "STAC_HIP_HANDOFF": "0"},
           "handoff": {"STAC_HIP_HANDOFF": "8"},
           "queue_handoff": {"STAC_HIP_QUEUE": "4", "STAC_HIP_WPB": "1", "STAC_HIP_HANDOFF": "4"}}[variant]
    fs = rodent_setup
    kp, ref = _rodent_case(fs, rodent_mocap)
    eng = _throughput(monkeypatch, fs, env)
    res = _q_phase_twice(eng, kp[:, :2], **_kw(fs))
    got = _last_q_kernel(eng)
    assert got[:2] == (16, 5) and got[3] == (1 if variant == "queue" else 5), got  # (hand-off: the lean latency kernel ran last)
    _compare_phase(res, _part(ref, 9, 2))
    np.testing.assert_array_equal(_np(res["carry_qpos"]), ref["qpos"][:, 1])


def test_no_root_optimisation(rodent_setup, rodent_mocap, monkeypatch):
    """do_root_opt false: no root pass, no root fast trip, no pruned program (fk3r_n = 0 behind the pinned word)."""
    fs = rodent_setup
    kp, ref = _rodent_case(fs, rodent_mocap, do_root_opt=False)
    eng = _throughput(monkeypatch, fs)
    res = _q_phase_twice(eng, kp[:5, :2], **_kw(fs, do_root_opt=False))
    assert _last_q_kernel(eng)[3] == 1
    _compare_phase(res, _part(ref, 5, 2))


@pytest.mark.parametrize("env,lean", [({}, 1), ({"STAC_HIP_NOLEAN": "1"}, 0),
                                      ({"STAC_HIP_NOLEAN": "1", "STAC_HIP_NOFREE0": "1", "STAC_HIP_NOFAST": "1"}, 0)],
                         ids=["as_planned", "generic", "generic_free0p_0_root_fast_0"])
def test_synth_fixture_on_the_throughput_kernels(monkeypatch, env, lean):
    """A body with one free joint and one marker (seven coordinates, no hinge), five chains of two frames, root optimisation on: as the
    host plans it (the lean kernel), on the generic kernel, and there with
    free0p == 0 and root_fast == 0 forced: the generic kernel takes its launch decisions as before."""
    from stac_mjx_amd.fit_model import finish_fit_setup
    from stac_mjx_amd.mjcf import ModelTables

    cfgm = json.load(open(GOLDEN / "synth_model_cfg.json"))["model"]
    fs = finish_fit_setup(ModelTables.load(GOLDEN / "synth_tables.npz"), cfgm, list(cfgm["KEYPOINT_MODEL_PAIRS"].keys()))
    rng = np.random.default_rng(8)
    kp = (np.load(GOLDEN / "synth_kp_1.npy").reshape(1, 1, 3) + rng.normal(0, 0.02, (5, 2, 3))).astype(np.float32)
    eng = _throughput(monkeypatch, fs, env)
    res = _q_phase_twice(eng, kp, **_kw(fs, do_root_opt=fs.do_root_opt))
    got = _last_q_kernel(eng)
    assert got[0] == 16 and got[3] == lean, got  # throughput; lean or generic
    ref = _oracle(fs, tol=TOL, maxiter=MAXITER).ik_clips(kp, fs.lb, fs.ub, fs.part_masks, fs.trunk_kps, fs.root_kp_idx, fs.root_dims,
                                                         do_root_opt=fs.do_root_opt)
    _compare_phase(res, ref)


def test_fly_small_batch(fly_setup, monkeypatch):
    """Tethered fly (no root optimisation), three chains of two frames on the throughput kernel."""
    fly = fly_setup
    orc = _oracle(fly, tol=TOL, maxiter=MAXITER)
    rng = np.random.default_rng(12)
    qt = fly.tables.qpos0[None] + np.clip(rng.normal(0, 0.1, (6, fly.tables.nq)), -0.2, 0.2).astype(np.float32)
    qt[:, 3:7] = fly.tables.qpos0[3:7]
    kp = np.stack([orc.fk(q)["site_xpos"].reshape(-1) for q in qt]).reshape(3, 2, 3 * fly.tables.nsite)
    kp = (kp + rng.normal(0, 1e-3, kp.shape)).astype(np.float32)
    eng = _throughput(monkeypatch, fly)
    res = _q_phase_twice(eng, kp, part_masks=fly.part_masks)
    got = _last_q_kernel(eng)
    assert got[0] == 16 and got[3] in (0, 1), got
    _compare_phase(res, orc.ik_clips(kp, fly.lb, fly.ub, fly.part_masks, fly.trunk_kps, 0, 7, do_root_opt=False))


def test_mouse_small_batch_start_pose_outside_the_box(mouse_setup, monkeypatch):
    """Mouse: ranges that do not contain the rest angle, so a chain's first root trips cannot run lite (`tail_ok` false until the first
    iteration has moved the coordinates onto the box); three chains of two frames."""
    ms = mouse_setup
    assert np.any((ms.tables.qpos0 < ms.lb) | (ms.tables.qpos0 > ms.ub))  # (on the host: the start pose is outside the box)
    real = np.load(GOLDEN / "mouse_mocap_200.npy")
    kp = real[[5, 41, 78, 121, 161, 198]].reshape(3, 2, 102)
    eng = _throughput(monkeypatch, ms)
    res = _q_phase_twice(eng, kp, **_kw(ms, do_root_opt=ms.do_root_opt))
    got = _last_q_kernel(eng)
    assert got[0] == 16 and got[3] in (0, 1), got
    _compare_phase(res, _oracle(ms, tol=TOL, maxiter=MAXITER).ik_clips(kp, ms.lb, ms.ub, ms.part_masks, ms.trunk_kps, ms.root_kp_idx,
                                                                       ms.root_dims, do_root_opt=ms.do_root_opt))


def test_solve_longer_than_the_momentum_table(rodent_setup, rodent_mocap, monkeypatch):
    """maxiter 300: the full-body solve does not reach the tolerance and runs past the 256 entries of the plan's momentum table, so
    t_next and beta come from the table first and from the square root and the division afterwards (five chains: two wavefronts)."""
    fs = rodent_setup
    kp, ref = _rodent_case(fs, rodent_mocap, maxiter=300)
    # (on the host: with a bound of 256 every chain takes fewer iterations, so some solve of each ran beyond the table)
    c256 = _oracle(fs, tol=TOL, maxiter=256).ik_clips(kp[:5, :1], fs.lb, fs.ub, fs.part_masks, fs.trunk_kps, fs.root_kp_idx, fs.root_dims,
                                                      want_bodies=False)["counters"]
    assert (ref["counters"][:5, 0, 0] > c256[:, 0, 0]).all()
    eng = _throughput(monkeypatch, fs, maxiter=300)
    res = eng.q_phase(kp[:5, :1], **_kw(fs))
    assert _last_q_kernel(eng)[3] == 1
    _compare_phase(res, _part(ref, 5, 1))


@pytest.mark.parametrize("do_root_opt", [True, False], ids=["root_fast_trips", "full_trips"])
def test_root_quaternion_of_norm_zero(rodent_setup, rodent_mocap, monkeypatch, do_root_opt):
    """q_init with a root quaternion of zeros: every evaluation point of the clip has |q| = 0 there (the gradient of a zero quaternion is
    zero, so it stays) -- the `n == 0` branch of the free root's pre-pass in root fast trips and in full trips."""
    fs = rodent_setup
    qi = np.tile(fs.tables.qpos0, (9, 1)).astype(np.float32)
    qi[:, 3:7] = 0.0
    kp, ref = _rodent_case(fs, rodent_mocap, do_root_opt=do_root_opt, q_init=qi, key="zero_quat")
    assert not ref["qpos"][:4, :2, 3:7].any()  # (on the host: the oracle's quaternion never left zero)
    eng = _throughput(monkeypatch, fs)
    res = _q_phase_twice(eng, kp[:4, :2], q_init=qi[:4], **_kw(fs, do_root_opt=do_root_opt))
    assert _last_q_kernel(eng)[3] == 1
    _compare_phase(res, _part(ref, 4, 2))
