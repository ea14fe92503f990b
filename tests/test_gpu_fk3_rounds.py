"""P2 of the split kinematics in whole rounds of 16 lanes (pairs of rounds and one single round behind them in the throughput
kernels, the shorter table in the latency kernels) and the range tables of the gradient pass at the lane count's edge: lean launches
against the oracle at tolerance 0.  The models come from tests/fk3_cases.py, which asserts their rotation / range counts on the host."""

import numpy as np
import pytest

from fk3_cases import fk3_program, model_with_ranges, model_with_rotations

pytestmark = pytest.mark.gpu

# the two lean launches of a 16-lane group, forced through the developer switches: (environment, lanes_per_chain, SPECP of the kernel)
LAUNCHES = {"throughput": ({"STAC_HIP_SPEC": "0"}, 16, 1), "latency": ({"STAC_HIP_SPEC": "1", "STAC_HIP_SPECG": "16"}, 0, 5)}
MAXITER, TOL = 10, 1e-5
_REF = {}


def _last_q_kernel(eng):
    import ctypes

    out = (ctypes.c_int32 * 4)()
    eng.lib.stac_debug_last_q_kernel(out)
    return tuple(out)


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.uint32)


def _assert_same(res, ref, what):
    for key in ("counters", "qpos", "frame_error"):
        np.testing.assert_array_equal(_bits(res[key]), _bits(ref[key]), err_msg=f"{what}: {key}")


def _case(key, t, lb, ub, trunk, chains=8, frames=2):
    """Keypoints, part masks and the oracle's answer for a model: computed once, shared by the launches that check it."""
    if key not in _REF:
        from oracle import Oracle

        rng = np.random.default_rng(4242 + sum(map(ord, str(key))))
        orc = Oracle(t, tol=TOL, maxiter=MAXITER)
        n = chains * frames
        q = np.tile(t.qpos0, (n, 1)) + rng.normal(0, 0.15, (n, t.nq)).astype(np.float32)
        q = np.clip(q, np.where(np.isfinite(lb), lb, -3), np.where(np.isfinite(ub), ub, 3)).astype(np.float32)
        kp = np.stack([orc.fk(x.copy())["site_xpos"].reshape(-1) for x in q]).astype(np.float32)
        kp = (kp + rng.normal(0, 2e-3, kp.shape)).astype(np.float32).reshape(chains, frames, 3 * t.nsite)
        part = np.zeros((2, t.nq), np.uint8)
        part[0] = rng.random(t.nq) < 0.5
        part[1] = rng.random(t.nq) < 0.15
        ref = orc.ik_clips(kp, lb, ub, part, trunk, 0, 7, do_root_opt=True)
        _REF[key] = (kp, part, ref)
    return _REF[key]


def _launch(monkeypatch, launch, t, lb, ub, kp, part, trunk, extra_env=None):
    from stac_mjx_amd.engine import Engine

    env, lanes, specp = LAUNCHES[launch]
    for k, v in {**env, **(extra_env or {})}.items():
        monkeypatch.setenv(k, v)  # (read once, when the engine creates its model)
    eng = Engine(t, lb, ub, tol=TOL, maxiter=MAXITER, lanes_per_chain=lanes)
    res = eng.q_phase(kp, part_masks=part, trunk_kps=trunk, root_kp_idx=0, root_dims=7, do_root_opt=True)
    got = _last_q_kernel(eng)
    assert got[0] == 16 and got[3] == specp, (launch, got)  # the lean kernel of this launch, 16 lanes per chain
    return res


@pytest.mark.parametrize("launch", list(LAUNCHES))
@pytest.mark.parametrize("residue", [1, 15, 16, 17, 31, 0])
def test_rotation_counts_at_every_residue_of_a_pair_of_rounds(monkeypatch, residue, launch):
    """Full programs of 1, 15, 16, 17, 31 and 0 rotations mod 32 (padded to a single round behind the pairs, or to whole pairs), each
    with a pruned root program of another residue class; 8 chains of 2 frames with the root optimisation on."""
    oriented = residue in (15, 17, 0)
    t, lb, ub, trunk, full, root = model_with_rotations(residue, oriented)
    assert full["nrot"] % 32 == residue and full["nrot"] >= 33 and root["nrot"] % 32 != residue  # (on the host, before the launch)
    assert full["n2"] == (full["nrot"] + 15) // 16 * 16 and root["n2"] == (root["nrot"] + 15) // 16 * 16
    assert bool(np.any(t.body_quat[1:] != np.array([1, 0, 0, 0], np.float32))) == oriented
    kp, part, ref = _case(("rot", residue), t, lb, ub, trunk)
    _assert_same(_launch(monkeypatch, launch, t, lb, ub, kp, part, trunk), ref, f"{full['nrot']} / {root['nrot']} rotations, {launch}")


@pytest.mark.parametrize("launch", list(LAUNCHES))
@pytest.mark.parametrize("rsplit", ["0", "max"])
@pytest.mark.parametrize("nrange", [16, 17])
def test_range_tables_of_16_and_17_ranges(monkeypatch, nrange, rsplit, launch):
    """As many distinct site ranges as lanes, and one more; none of them summed by component, and all of them (STAC_HIP_RSPLIT is
    clamped to the number of ranges)."""
    t, lb, ub, trunk, info = model_with_ranges(nrange)
    assert info["nrange"] == nrange  # (on the host, before the launch)
    env = {"STAC_HIP_RSPLIT": "0" if rsplit == "0" else "9999"}
    monkeypatch.setenv("STAC_HIP_RSPLIT", env["STAC_HIP_RSPLIT"])
    forced, _ = fk3_program(t, lb, ub)
    assert forced["rsplit"] == (0 if rsplit == "0" else nrange)
    kp, part, ref = _case(("range", nrange), t, lb, ub, trunk)
    _assert_same(_launch(monkeypatch, launch, t, lb, ub, kp, part, trunk, env), ref, f"{nrange} ranges, rsplit {rsplit}, {launch}")


def test_rodent_throughput_lean_equals_the_oracle_and_the_generic_kernel(rodent_setup, rodent_mocap, monkeypatch):
    """The bench's model, 64 chains of one frame: five rounds of P2 in a full trip, three in a root fast trip."""
    from oracle import Oracle
    from stac_mjx_amd.engine import Engine

    fs = rodent_setup
    kp = rodent_mocap[100:164].reshape(64, 1, 69)
    kw = dict(part_masks=fs.part_masks, trunk_kps=fs.trunk_kps, root_kp_idx=fs.root_kp_idx, root_dims=fs.root_dims, do_root_opt=True)
    monkeypatch.setenv("STAC_HIP_SPEC", "0")
    eng = Engine(fs.tables, fs.lb, fs.ub, tol=1e-4, maxiter=40, lanes_per_chain=16)
    lean = eng.q_phase(kp, **kw)
    got = _last_q_kernel(eng)
    assert got[:2] == (16, 5) and got[3] == 1, got
    ref = Oracle(fs.tables, tol=1e-4, maxiter=40).ik_clips(kp, fs.lb, fs.ub, fs.part_masks, fs.trunk_kps, fs.root_kp_idx, fs.root_dims)
    _assert_same(lean, ref, "rodent, lean against the oracle")
    monkeypatch.setenv("STAC_HIP_NOLEAN", "1")
    gen_eng = Engine(fs.tables, fs.lb, fs.ub, tol=1e-4, maxiter=40, lanes_per_chain=16)
    gen = gen_eng.q_phase(kp, **kw)
    assert gen_eng is not eng and _last_q_kernel(gen_eng)[3] == 0, _last_q_kernel(gen_eng)
    _assert_same(lean, gen, "rodent, lean against generic")
    for key in ("marker_sites", "carry_qpos"):
        np.testing.assert_array_equal(_bits(lean[key]), _bits(gen[key]), err_msg=key)
