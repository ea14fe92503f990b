"""The oracle's kinematics and offset phase against an independent float64 statement (tests/kin_ref.py) -- CPU only.

Everything on the GPU is "bit-exact to the restatement" (oracle/stac_oracle.c); the restatement's FK was pinned to real reference
output on the rodent only (free root, hinges with qpos0 = 0, no oriented body).  Here ball joints, slides, qpos - qpos0 and
body_quat != identity (fly, mouse, random trees, comb trees of up to 171 bodies) and `_m_opt` are held to a statement that
shares no code and no operation order with it.

Measured on the models below, 8 poses each (qpos0 + N(0, 0.4)), |x| <= 2.1:
  float64 twin vs kin_ref.fk        max 1.13e-7 (bound: one float32 rounding of the output, 2^-23 max(|ref|, 1), derived)
  float32 oracle vs kin_ref.fk      max MEASURED_F32_FK = 7.13e-7 (comb84; rodent 2.97e-7, fly 2.28e-7, mouse 5.12e-7, random trees
                                    6.86e-7 / 6.79e-7, comb40 5.34e-7, comb85 5.57e-7) -> asserted at F32_FK_FACTOR = 4 x that =
                                    2.85e-6 (<= 1e-5, a tenth of the north star); the margin is for other draws and deeper trees
  stored reference output (50 rodent poses of demos/demo_viz.p) vs kin_ref.fk: xpos 1.58e-7, sites 1.21e-7 (TOL_FK_GOLDEN 5e-7)
  m_opt offsets vs kin_ref.m_opt    f32 oracle max 5.1e-8, f64 twin max 1.7e-9 (both asserted at TOL_NORTH_STAR = 1e-4)
  m_opt err, relative               f32 oracle up to 4.8e-5 (rodent, T = 1000: z2 - 2 m.s + T m.m cancels to a hundredth of z2;
                                    recorded, not asserted), f64 twin max 5.3e-8 (asserted at 1e-6)
The twin reached that only once Oracle.m_opt kept its sums in double (orc_m_opt): through the float32 `partial` of
m_partial / m_finish its err is 3.4e-6 off, the same cancellation at work on the rounding of the sums.

kin_ref.rot is MuJoCo's mju_quat2Mat, q v q*: body_quat is stored in float32 and unit only to that rounding, and with the
"unit quaternion" form 1 - 2 (y^2 + z^2) instead the statement drifts from the twin by 1.8e-7 down the 85 levels of comb84.

Oracle mutations that turn tests of this file red (checked on a scratch copy): the slide without "- qpos0", body_quat (x) xquat[p]
for xquat[p] (x) body_quat, a ball quaternion left unnormalised -- each fails the twin, the float32 and the m_opt tests on the
random trees (the swapped product also on rodent, fly and the combs).
"""

import numpy as np
import pytest

import kin_ref
from conftest import GOLDEN
from test_gpu_offsets_fk import FK_MAX_SLOTS, FK_TREES, _chain_tables, _comb_tables, _fk_slots
from test_gpu_parity import TOL_FK_GOLDEN, TOL_NORTH_STAR, _random_tables

MEASURED_F32_FK = 7.13e-7  # largest |float32 oracle - kin_ref.fk| over MODELS x N_POSES (xpos, xquat, site_xpos), measured
F32_FK_FACTOR = 4
F32_FK_BOUND = F32_FK_FACTOR * MEASURED_F32_FK
assert F32_FK_BOUND <= 1e-5  # a tenth of the north-star 1e-4

MODELS = ["rodent", "fly", "mouse", "random_ball_slide", "random_fixed_root", "comb40", "comb84", "comb85"]
N_POSES = 8
ARRAYS = ("xpos", "xquat", "site_xpos")


def _tables(model):
    from stac_mjx_amd.mjcf import ModelTables

    if model in ("rodent", "fly", "mouse"):
        return ModelTables.load(GOLDEN / f"{model}_tables.npz")
    if model == "random_ball_slide":
        return _random_tables(np.random.default_rng(77), 37, True, p_slide=0.2, p_ball=0.2)
    if model == "random_fixed_root":
        return _random_tables(np.random.default_rng(78), 37, False, p_slide=0.2, p_ball=0.2)
    return _comb_tables(int(model[4:]))


@pytest.fixture(scope="module")
def fk_results():
    """{model: (tables, [per pose: {"ref" | "f32" | "f64": {array: values}}])}, computed once."""
    from oracle import Oracle

    out = {}
    for i, model in enumerate(MODELS):
        t = _tables(model)
        rng = np.random.default_rng(900 + i)
        q = (np.asarray(t.qpos0, np.float32)[None] + rng.normal(0, 0.4, (N_POSES, t.nq))).astype(np.float32)
        o32, o64 = Oracle(t), Oracle(t, precision="f64")
        rows = []
        for x in q:
            ref = dict(zip(ARRAYS, kin_ref.fk(t, x)))
            rows.append({"ref": ref, "f32": o32.fk(x.copy()), "f64": o64.fk(x.copy())})
        out[model] = (t, rows)
    return out


def _max_dev(rows, which):
    return max(np.abs(r[which][k].astype(np.float64) - r["ref"][k]).max() for r in rows for k in ARRAYS)


def test_models_cover_every_joint_kind_and_oriented_bodies(fk_results):
    """What the rodent does not have is in the set: ball joints, slides, hinges and slides with qpos0 != 0, oriented bodies, a fixed
    root, bodies with several joints."""
    from stac_mjx_amd.mjcf import JNT_BALL, JNT_FREE, JNT_HINGE, JNT_SLIDE

    kinds, flags = set(), set()
    for model, (t, _) in fk_results.items():
        kinds |= set(t.jnt_type.tolist())
        one = [j for j in range(t.njnt) if t.jnt_type[j] in (JNT_SLIDE, JNT_HINGE)]
        for ty in (JNT_SLIDE, JNT_HINGE):
            if any(t.jnt_type[j] == ty and t.qpos0[t.jnt_qposadr[j]] != 0 for j in one):
                flags.add(("qpos0", ty))
        if (np.abs(t.body_quat[1:] - [1, 0, 0, 0]).max(axis=1) > 0.1).any():
            flags.add("oriented")
        if t.jnt_type[0] != JNT_FREE:
            flags.add("fixed root")
        if (t.body_jntnum > 1).any():
            flags.add("several joints")
    assert kinds == {JNT_FREE, JNT_BALL, JNT_SLIDE, JNT_HINGE}
    assert flags == {("qpos0", JNT_SLIDE), ("qpos0", JNT_HINGE), "oriented", "fixed root", "several joints"}
    n_oriented = int((np.abs(fk_results["fly"][0].body_quat[1:] - [1, 0, 0, 0]).max(axis=1) > 0).sum())
    assert n_oriented == 42


@pytest.mark.parametrize("model", MODELS)
def test_float64_twin_equals_the_statement_to_output_rounding(model, fk_results):
    """The twin computes in double and returns float32 arrays: it differs from the float64 statement by one float32 rounding of the
    result -- half an ulp, 2^-24 |x|; asserted with a factor of two: 2^-23 max(|ref|, 1), element by element."""
    _, rows = fk_results[model]
    print(f"{model}: float64 twin vs kin_ref.fk max {_max_dev(rows, 'f64'):.3g}")
    for r in rows:
        for k in ARRAYS:
            ref = r["ref"][k]
            dev = np.abs(r["f64"][k].astype(np.float64) - ref)
            bound = 2.0 ** -23 * np.maximum(np.abs(ref), 1.0)
            assert (dev <= bound).all(), (model, k, dev.max())


@pytest.mark.parametrize("model", MODELS)
def test_float32_oracle_within_four_times_its_measured_deviation(model, fk_results):
    _, rows = fk_results[model]
    dev = _max_dev(rows, "f32")
    scale = max(np.abs(r["ref"][k]).max() for r in rows for k in ARRAYS)
    print(f"{model}: float32 oracle vs kin_ref.fk max {dev:.3g} at |x| <= {scale:.3g} (bound {F32_FK_BOUND:.3g})")
    assert dev <= F32_FK_BOUND, (model, dev)


def test_statement_reproduces_stored_reference_output(demo_viz):
    """kin_ref.fk on the 50 stored poses (legacy rodent tables, stored offsets) against the stored MJX xpos and marker sites."""
    from stac_mjx_amd.mjcf import ModelTables

    t = ModelTables.load(GOLDEN / "rodent_tables_legacy.npz").copy()
    t.site_pos = np.asarray(demo_viz["offsets"], np.float32).reshape(t.nsite, 3)
    dx = ds = 0.0
    for f in range(50):
        xpos, _, sites = kin_ref.fk(t, demo_viz["qpos"][f])
        dx = max(dx, np.abs(xpos - demo_viz["xpos"][f]).max())
        ds = max(ds, np.abs(sites - demo_viz["walker_body_sites"][f].reshape(-1, 3)).max())
    print(f"kin_ref.fk vs stored reference output: xpos {dx:.3g}, sites {ds:.3g}")
    assert dx <= TOL_FK_GOLDEN and ds <= TOL_FK_GOLDEN


@pytest.fixture(scope="module")
def m_opt_inputs():
    """{model: (tables, q[1000,nq], kp[1000,3K], m0, mask)}: keypoints are the sites of a perturbed offset set plus 1 mm of noise."""
    from oracle import Oracle

    out = {}
    for i, model in enumerate(("rodent", "random_ball_slide")):
        t = _tables(model)
        rng = np.random.default_rng(950 + i)
        q = (np.asarray(t.qpos0, np.float32)[None] + rng.normal(0, 0.4, (1000, t.nq))).astype(np.float32)
        orc = Oracle(t)
        orc.set_site_pos(t.site_pos + rng.normal(0, 3e-3, (t.nsite, 3)).astype(np.float32))
        kp = np.stack([orc.fk(x.copy())["site_xpos"].reshape(-1) for x in q])
        kp = (kp + rng.normal(0, 1e-3, kp.shape)).astype(np.float32)
        mask = (rng.random((t.nsite, 3)) < 0.5).astype(np.float32)
        out[model] = (t, q, kp, np.asarray(t.site_pos, np.float32), mask)
    return out


_SUMS = {}


@pytest.mark.parametrize("reg_coef", [0.0, 1.0])
@pytest.mark.parametrize("T", [9, 1000])
@pytest.mark.parametrize("model", ["rodent", "random_ball_slide"])
def test_m_opt_against_the_statement(model, T, reg_coef, m_opt_inputs):
    from oracle import Oracle

    t, q, kp, m0, mask = m_opt_inputs[model]
    if (model, T) not in _SUMS:  # (a thousand poses in numpy take seconds: once for both coefficients)
        _SUMS[model, T] = kin_ref.m_sums(t, kp[:T], q[:T])
    ref, ref_err = kin_ref.m_closed_form(_SUMS[model, T], m0, mask, reg_coef)
    assert ref_err > 0
    for precision in ("f32", "f64"):
        off, err = Oracle(t, precision=precision).m_opt(kp[:T], q[:T], m0, mask, reg_coef)
        if precision == "f32":  # (the one-call form is the two-call form the GPU is compared with, bit for bit)
            orc = Oracle(t)
            off2, err2 = orc.m_finish(orc.m_partial(kp[:T], q[:T]), m0, mask, reg_coef)
            np.testing.assert_array_equal(off, off2)
            assert err == err2
        dev, rel = np.abs(off.astype(np.float64) - ref).max(), abs(err - ref_err) / ref_err
        print(f"{model} T={T} reg_coef={reg_coef} {precision}: offsets {dev:.3g}, err relative {rel:.3g} (err {ref_err:.6g})")
        assert dev <= TOL_NORTH_STAR, (precision, dev)
        if precision == "f64":
            assert rel <= 1e-6, (rel, err, ref_err)


def test_hand_built_trees_park_what_they_claim():
    """The trees of tests/test_gpu_offsets_fk.py reach the edges they are named after: a replica of the slot allocator of
    stac_planner.hip (build_fk_tables) counts the parked transforms; 83 is the last count under fk_kernel's 160 KiB of LDS."""
    assert {k: _fk_slots(f().body_parentid.tolist()) for k, (f, _) in FK_TREES.items()} == {k: s for k, (_, s) in FK_TREES.items()}
    assert _fk_slots(_comb_tables(85).body_parentid.tolist()) == FK_MAX_SLOTS + 1
    assert (7 * FK_MAX_SLOTS + 57) * 256 == 163328 <= 160 * 1024 < (7 * (FK_MAX_SLOTS + 1) + 57) * 256
    assert [_chain_tables(n).nbody for n in (2, 8, 16, 17)] == [2, 8, 16, 17]
    assert _comb_tables(40).nbody == 81
