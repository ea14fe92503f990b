"""The offset phase (m_contrib_kernel, m_reduce_kernel, m_finish_kernel) and the stand-alone fk_kernel beyond the rodent: HIP vs
the CPU oracle at tolerance 0 (NaN equal to NaN) on models with oriented bodies, ball joints, slides and a fixed root, at the
frame counts and site counts where the launches change shape, and fk_kernel at its structural edges -- the smallest trees, a full
last staging chunk, and trees that park up to the largest number of transforms the kernel's LDS holds (one more is refused).

Largest shapes here: offset phase K = 70, T = 1000, nbody = 225; fk_kernel 83 parked transforms (nbody = 169), refusal at 84.
What the oracle itself is held to: tests/test_kin_ref_host.py (an independent float64 statement, CPU).
"""

import contextlib

import numpy as np
import pytest

from test_gpu_parity import _np, _random_tables

pytestmark = pytest.mark.gpu

FK_MAX_SLOTS = 83  # stac_kernels.hip, launch_fk: (7 * slots + 57) * 256 B of LDS <= 160 KiB


# ---- hand-built trees ------------------------------------------------------------------------------------------------------------
def _tree_tables(parent, joints, site_body, seed):
    """ModelTables of the tree `parent` (parent[b] < b, parent[0] = 0) with the joints
    {body: [joint types]} and one fit site per entry of site_body; random body offsets and orientations, joint anchors and axes."""
    from stac_mjx_amd.mjcf import JNT_BALL, JNT_FREE, JNT_HINGE, JNT_QPOS_DIMS, ModelTables

    rng = np.random.default_rng(seed)
    nbody, K = len(parent), len(site_body)
    assert all(parent[b] < b for b in range(1, nbody)) and parent[0] == 0

    def unit(v):
        return v / np.linalg.norm(v)

    depth = [0] * nbody
    for b in range(1, nbody):
        depth[b] = depth[parent[b]] + 1
    body_quat = np.stack([[1.0, 0, 0, 0]] + [unit(rng.normal(0, 1, 4)) for _ in range(1, nbody)])
    jt, jadr, jbody, jrange, qpos0 = [], [], [], [], []
    body_jntadr, body_jntnum = [-1] * nbody, [0] * nbody
    for b in range(1, nbody):
        for ty in joints.get(b, []):
            if body_jntadr[b] < 0:
                body_jntadr[b] = len(jt)
            body_jntnum[b] += 1
            jt.append(ty)
            jadr.append(len(qpos0))
            jbody.append(b)
            if ty == JNT_FREE:
                qpos0 += [0, 0, 0.1, 1, 0, 0, 0]
            elif ty == JNT_BALL:
                qpos0 += [1, 0, 0, 0]
            else:
                qpos0.append(float(rng.normal(0, 0.05)))
            jrange.append([-1.0, 1.2] if ty == JNT_HINGE else [0, 0])
            assert len(qpos0) == jadr[-1] + JNT_QPOS_DIMS[ty]
    nj = len(jt)
    return ModelTables(
        nbody=nbody, njnt=nj, nq=len(qpos0), nsite=K, body_parentid=np.array(parent, np.int32),
        body_pos=rng.normal(0, 0.05, (nbody, 3)).astype(np.float32), body_quat=body_quat.astype(np.float32),
        body_jntadr=np.array(body_jntadr, np.int32), body_jntnum=np.array(body_jntnum, np.int32), body_depth=np.array(depth, np.int32),
        jnt_type=np.array(jt, np.int32), jnt_qposadr=np.array(jadr, np.int32), jnt_bodyid=np.array(jbody, np.int32),
        jnt_pos=rng.normal(0, 0.02, (nj, 3)).astype(np.float32),
        jnt_axis=np.stack([unit(rng.normal(0, 1, 3)) for _ in range(nj)]).astype(np.float32).reshape(nj, 3),
        jnt_range=np.array(jrange, np.float32).reshape(nj, 2), qpos0=np.array(qpos0, np.float32),
        site_bodyid=np.array(sorted(site_body), np.int32), site_pos=rng.normal(0, 0.01, (K, 3)).astype(np.float32),
        body_names=[f"b{i}" for i in range(nbody)], jnt_names=[f"j{i}" for i in range(nj)], site_names=[f"s{i}" for i in range(K)])


def _chain_tables(nbody):
    """A chain under a fixed root, no transform parked: a hinge per body; body 3 a slide and a hinge, body 5 a ball joint."""
    from stac_mjx_amd.mjcf import JNT_BALL, JNT_HINGE, JNT_SLIDE

    joints = {b: [JNT_HINGE] for b in range(1, nbody)}
    if nbody > 3:
        joints[3] = [JNT_SLIDE, JNT_HINGE]
    if nbody > 5:
        joints[5] = [JNT_BALL]
    return _tree_tables([0] + list(range(nbody - 1)), joints,
                        [1, max(1, nbody // 2), nbody - 1, nbody - 1], 1000 + nbody)


def _star_tables(nleaf=20):
    """One hub (body 1) with nleaf leaf children, a hinge each: the hub's transform stays parked in one slot for nleaf bodies."""
    from stac_mjx_amd.mjcf import JNT_HINGE

    parent = [0, 0] + [1] * nleaf
    return _tree_tables(parent, {b: [JNT_HINGE] for b in range(1, nleaf + 2)}, [1, 2, 1 + nleaf // 2, nleaf + 1], 2000 + nleaf)


def _comb_tables(S):
    """A comb: the spine is bodies 1 .. S in a chain, then come S leaves, leaf i (body S + 1 + i) on spine body S - i: the
    leaf of a spine body comes after the whole rest of the spine.  Every spine body but the last waits for a child further down the list: S - 1 transforms
    are parked at once.  A free root, a hinge on every seventh body, random orientations, four sites on leaves."""
    from stac_mjx_amd.mjcf import JNT_FREE, JNT_HINGE

    parent = [0] + list(range(S)) + [S - i for i in range(S)]
    joints = {b: [JNT_HINGE] for b in range(2, 2 * S + 1) if b % 7 == 0}
    joints[1] = [JNT_FREE]
    return _tree_tables(parent, joints, [S + 1 + i for i in (0, S // 3, 2 * S // 3, S - 1)], 3000 + S)


def _fk_slots(parent):
    """How many LDS slots the host allots for fk_kernel (stac_planner.hip, build_fk_tables): a body with a child that does not follow
    it directly parks its transform until its last child has read it; a slot is free again from that child's step on."""
    nb = len(parent)
    last_child, far = [-1] * nb, [False] * nb
    for b in range(1, nb):
        last_child[parent[b]] = b
        far[parent[b]] |= parent[b] != b - 1
    owner = []
    for b in range(nb):
        if far[b]:
            free = [k for k, o in enumerate(owner) if last_child[o] <= b]
            if free:
                owner[free[0]] = b
            else:
                owner.append(b)
    return len(owner)


def _free_box(t):
    return np.full(t.nq, -np.inf, np.float32), np.full(t.nq, np.inf, np.float32)


def _poses(t, n, seed):
    """qpos0 + N(0, 0.4): free and ball quaternions are far from unit length (stac_fk and stac_m_phase_partial normalise)."""
    rng = np.random.default_rng(seed)
    return (np.asarray(t.qpos0, np.float32)[None] + rng.normal(0, 0.4, (n, t.nq))).astype(np.float32)


# ---- offset phase ----------------------------------------------------------------------------------------------------------------
def _resampled_rodent(fs, K, seed):
    """The rodent with K sites drawn from its 23 (as test_gpu_parity.test_more_than_64_sites does)."""
    rng = np.random.default_rng(seed)
    t = fs.tables.copy()
    pick = np.sort(rng.integers(0, 23, K))
    t.nsite = K
    t.site_bodyid = fs.tables.site_bodyid[pick].astype(np.int32)
    t.site_pos = (fs.tables.site_pos[pick] + rng.normal(0, 2e-3, (K, 3))).astype(np.float32)
    t.site_names = [f"s{i}" for i in range(K)]
    return t


M_MODELS = ["fly", "mouse", "random_ball_slide", "random_fixed_root", "rodent_K42", "rodent_K43", "rodent_K70"]
M_FRAMES = (1, 63, 64, 65, 130)  # the blocks of 64 frames of m_contrib_kernel and fk_kernel: below, at and above one and two


def _m_tables(model, fly_setup, mouse_setup, rodent_setup):
    if model == "fly":
        return fly_setup.tables
    if model == "mouse":
        return mouse_setup.tables
    if model == "random_ball_slide":
        return _random_tables(np.random.default_rng(77), 37, True, p_slide=0.2, p_ball=0.2)
    if model == "random_fixed_root":
        return _random_tables(np.random.default_rng(78), 37, False, p_slide=0.2, p_ball=0.2)
    return _resampled_rodent(rodent_setup, int(model.split("K")[1]), 70)


def _m_case(t, T, seed):
    """Engine, oracle, T poses and their keypoints: the sites of a perturbed offset set plus 1 mm of noise."""
    from oracle import Oracle
    from stac_mjx_amd.engine import Engine

    rng = np.random.default_rng(seed)
    eng, orc = Engine(t, *_free_box(t)), Oracle(t)
    q = _poses(t, T, seed + 1)
    orc.set_site_pos(t.site_pos + rng.normal(0, 3e-3, (t.nsite, 3)).astype(np.float32))
    kp = np.stack([orc.fk(x.copy())["site_xpos"].reshape(-1) for x in q])
    orc.set_site_pos(t.site_pos)
    return eng, orc, q, (kp + rng.normal(0, 1e-3, kp.shape)).astype(np.float32)


def _finish_cases(K, rng):
    masks = [np.zeros((K, 3), np.float32), np.ones((K, 3), np.float32), (rng.random((K, 3)) < 0.5).astype(np.float32)]
    return [(lam, d) for lam in (0.0, 1.0, 1e6) for d in masks]


def _assert_finish_equal(eng, orc, part, ref_part, m0, cases, what):
    for lam, d in cases:
        off, err = eng.m_finish(part, m0, d, lam)
        ref_off, ref_err = orc.m_finish(ref_part, m0, d, lam)
        np.testing.assert_array_equal(_np(off), ref_off, err_msg=f"{what} reg_coef={lam} mask sum={d.sum()}")
        np.testing.assert_array_equal(_np(err), np.array([ref_err], np.float32), err_msg=f"{what} err reg_coef={lam} mask sum={d.sum()}")


@pytest.mark.parametrize("model", M_MODELS)
def test_m_phase_bit_exact_models_sites_and_frame_blocks(model, fly_setup, mouse_setup, rodent_setup):
    """m_partial, then m_finish offsets and err, == the oracle bit for bit at every T of M_FRAMES (and T = 1000 on the rodent: a
    frame sum in another order than index order shows there), for reg_coef in {0, 1, 1e6} x is_regularized all 0 / all 1 / random.
    K = 42 is exactly one block of m_reduce_kernel (3K + 2 = 128), K = 43 the first with a second block -- which holds the thread
    that writes T."""
    t = _m_tables(model, fly_setup, mouse_setup, rodent_setup)
    K = t.nsite
    frames = M_FRAMES + ((1000,) if model.startswith("rodent") else ())
    eng, orc, q, kp = _m_case(t, max(frames), 100 + M_MODELS.index(model))
    rng = np.random.default_rng(7)
    m0 = (t.site_pos + rng.normal(0, 3e-3, (K, 3))).astype(np.float32)
    cases = _finish_cases(K, rng)
    for T in frames:
        part = eng.m_partial(kp[:T], q[:T])
        ref_part = orc.m_partial(kp[:T], q[:T])
        np.testing.assert_array_equal(_np(part), ref_part, err_msg=f"{model} T={T}")
        assert ref_part[3 * K + 1] == T and np.isfinite(ref_part).all()
        _assert_finish_equal(eng, orc, part, ref_part, m0, cases, f"{model} T={T}")
    eng.close()


@pytest.mark.parametrize("model", ["fly", "random_ball_slide", "rodent_K43"])
def test_m_phase_shards_zero_frames_and_nan_keypoint(model, fly_setup, mouse_setup, rodent_setup):
    """(1) The sum of two shard partials (T = 20 + 45), finished on both sides.  (2) A partial with T = 0: zeros, and the finish
    keeps m0 wherever denom == 0 (an unregularised coordinate, or reg_coef = 0).  (3) One keypoint coordinate NaN in one frame:
    the three sums of that site and z2 are NaN on both sides, every other component is finite and equal."""
    t = _m_tables(model, fly_setup, mouse_setup, rodent_setup)
    K = t.nsite
    eng, orc, q, kp = _m_case(t, 65, 300 + M_MODELS.index(model))
    rng = np.random.default_rng(8)
    m0 = (t.site_pos + rng.normal(0, 3e-3, (K, 3))).astype(np.float32)
    cases = _finish_cases(K, rng)
    # (1)
    pa, pb = eng.m_partial(kp[:20], q[:20]), eng.m_partial(kp[20:], q[20:])
    ra, rb = orc.m_partial(kp[:20], q[:20]), orc.m_partial(kp[20:], q[20:])
    np.testing.assert_array_equal(_np(pa), ra)
    np.testing.assert_array_equal(_np(pb), rb)
    np.testing.assert_array_equal(_np(pa + pb), ra + rb)
    assert (ra + rb)[3 * K + 1] == 65
    _assert_finish_equal(eng, orc, pa + pb, ra + rb, m0, cases, f"{model} shards")
    # (2)
    p0 = eng.m_partial(np.zeros((0, 3 * K), np.float32), np.zeros((0, t.nq), np.float32))
    r0 = orc.m_partial(np.zeros((0, 3 * K), np.float32), np.zeros((0, t.nq), np.float32))
    np.testing.assert_array_equal(_np(p0), np.zeros(3 * K + 2, np.float32))
    np.testing.assert_array_equal(r0, np.zeros(3 * K + 2, np.float32))
    _assert_finish_equal(eng, orc, p0, r0, m0, cases, f"{model} T=0")
    d = cases[-1][1]
    assert 0 < d.sum() < 3 * K
    off, err = eng.m_finish(p0, m0, d, 1.0)
    np.testing.assert_array_equal(_np(off), m0)  # denom == 0: m0 kept; denom == 1: (0 + m0) / 1
    assert float(err) == 0.0
    off, _ = eng.m_finish(p0, m0, np.ones((K, 3), np.float32), 0.0)
    np.testing.assert_array_equal(_np(off), m0)
    # (3)
    k, frame = K // 2, 41
    kpn = kp.copy()
    kpn[frame, 3 * k + 1] = np.nan
    pn, rn = _np(eng.m_partial(kpn, q)), orc.m_partial(kpn, q)
    np.testing.assert_array_equal(pn, rn)
    want_nan = np.zeros(3 * K + 2, bool)
    want_nan[[3 * k, 3 * k + 1, 3 * k + 2, 3 * K]] = True
    np.testing.assert_array_equal(np.isnan(pn), want_nan)
    np.testing.assert_array_equal(np.isnan(rn), want_nan)
    clean = _np(eng.m_partial(kp, q))
    np.testing.assert_array_equal(pn[~want_nan], clean[~want_nan])
    eng.close()


# ---- workspace and stream contract of stac_m_phase_partial (raw ABI) -----------------------------------------------------------------
GUARD = 256


def _raw_m_partial(eng, kp, q, T, fill=None, stream=None):
    """stac_m_phase_partial on a workspace of exactly stac_m_phase_workspace_floats(m, T) floats and a partial of exactly 3K + 2,
    each in front of a guard of 256 bytes of 0xA5; the workspace prefilled with the 32-bit pattern `fill`.  Returns the partial and
    the two guards."""
    import torch
    from stac_mjx_amd.engine import _ptr

    K = eng.K
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        n = int(eng.lib.stac_m_phase_workspace_floats(eng._h, T))
        assert n == T * (7 * eng.nbody + 3 * K + 1)
        wbuf = torch.full((4 * n + GUARD,), 0xA5, dtype=torch.uint8, device=eng.device)
        pbuf = torch.full((4 * (3 * K + 2) + GUARD,), 0xA5, dtype=torch.uint8, device=eng.device)
        if fill is not None and n:
            wbuf[:4 * n].view(torch.int32).fill_(fill)
        kd = torch.from_numpy(kp[:T]).to(eng.device) if T else None
        qd = torch.from_numpy(q[:T]).to(eng.device) if T else None
        assert wbuf.data_ptr() % 4 == 0 and pbuf.data_ptr() % 4 == 0
        eng._check(eng.lib.stac_m_phase_partial(eng._h, _ptr(kd), _ptr(qd), T, _ptr(wbuf), _ptr(pbuf), eng._stream()))
        part = pbuf[:4 * (3 * K + 2)].view(torch.float32).clone()
        wg, pg = wbuf[4 * n:].clone(), pbuf[4 * (3 * K + 2):].clone()
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return _np(part), _np(wg), _np(pg)


@pytest.mark.parametrize("model", ["fly", "rodent_K43"])
def test_m_partial_workspace_guard_stale_content_and_stream(model, fly_setup, mouse_setup, rodent_setup):
    import torch

    t = _m_tables(model, fly_setup, mouse_setup, rodent_setup)
    K = t.nsite
    eng, orc, q, kp = _m_case(t, 65, 500 + M_MODELS.index(model))
    for T in (1, 64, 65):
        ref = orc.m_partial(kp[:T], q[:T])
        for fill in (None, 0x00000000, -1, 0x7FC00000):  # (None: the guard pattern itself, 0xA5A5A5A5)
            part, wg, pg = _raw_m_partial(eng, kp, q, T, fill=fill)
            assert (wg == 0xA5).all(), f"T={T}: written beyond the {T * (7 * eng.nbody + 3 * K + 1)} floats of the workspace"
            assert (pg == 0xA5).all(), f"T={T}: written beyond partial[3K+2]"
            np.testing.assert_array_equal(part, ref, err_msg=f"T={T} workspace prefilled with {fill}")
    ref = orc.m_partial(kp, q)
    part, wg, pg = _raw_m_partial(eng, kp, q, 65, fill=-1, stream=torch.cuda.Stream(device=eng.device))
    assert (wg == 0xA5).all() and (pg == 0xA5).all()
    np.testing.assert_array_equal(part, ref, err_msg="non-default stream")
    # T = 0 with null kp / q: zeros, partial[3K+1] = 0, nothing else touched
    for fill in (None, -1):
        part, wg, pg = _raw_m_partial(eng, kp, q, 0, fill=fill)
        np.testing.assert_array_equal(part, np.zeros(3 * K + 2, np.float32))
        assert (wg == 0xA5).all() and (pg == 0xA5).all()
    eng.close()


# ---- fk_kernel at its structural edges ----------------------------------------------------------------------------------------------
FK_TREES = {
    "chain2": (lambda: _chain_tables(2), 0),      # one hinge
    "chain8": (lambda: _chain_tables(8), 0),      # the last staged chunk of 8 bodies is exactly full
    "chain16": (lambda: _chain_tables(16), 0),    # two full chunks
    "chain17": (lambda: _chain_tables(17), 0),    # full chunks plus one body
    "star20": (lambda: _star_tables(20), 1),      # one slot held for 20 bodies
    "comb40": (lambda: _comb_tables(40), 39),
    "comb84": (lambda: _comb_tables(84), 83),     # 163 328 B of LDS: the largest under the cap
}
FK_WANTS = [("qpos", "xpos", "xquat", "site_xpos"), ("xpos", "xquat", "site_xpos"), ("site_xpos",), ("xpos", "xquat"), ("xquat", "site_xpos"),
            ("qpos",)]


@pytest.mark.parametrize("tree", list(FK_TREES))
def test_fk_structural_edges_bit_exact(tree):
    """Every output subset of stac_fk, on 65 poses (a full block and one pose) and on one pose, == the oracle bit for bit."""
    from oracle import Oracle
    from stac_mjx_amd.engine import Engine

    t = FK_TREES[tree][0]()
    eng, orc = Engine(t, *_free_box(t)), Oracle(t)
    q = _poses(t, 65, 11)
    ref = [orc.fk(x.copy()) for x in q]
    names = FK_WANTS[0]
    for want in FK_WANTS:
        for n in (65, 1):
            out = eng.fk(q[:n], want=want)
            for k in names:
                if k in want:
                    exp = np.stack([np.asarray(r[k], np.float32).reshape(-1) for r in ref[:n]])
                    np.testing.assert_array_equal(_np(out[k]).reshape(n, -1), exp, err_msg=f"{tree} {want} N={n} {k}")
                else:
                    assert out[k] is None
    eng.close()


def test_fk_refuses_one_parked_transform_too_many():
    """84 transforms parked at once do not fit fk_kernel's LDS: stac_fk and stac_m_phase_partial refuse on the host, before any
    launch, with STAC_ERR_CAPACITY and a message that names the cause; the engine of another model works afterwards."""
    import torch
    from oracle import Oracle
    from stac_mjx_amd.engine import Engine, StacHipError, _ptr

    t = _comb_tables(85)
    eng = Engine(t, *_free_box(t))
    q = _poses(t, 3, 12)
    qd = torch.from_numpy(q).to(eng.device)
    xpos = torch.full((3, t.nbody, 3), 7.0, dtype=torch.float32, device=eng.device)
    rc = eng.lib.stac_fk(eng._h, _ptr(qd), 3, None, _ptr(xpos), None, None, eng._stream())
    msg = eng._err()
    assert rc == -3 and eng.lib.stac_last_error_code() == -3, (rc, msg)  # STAC_ERR_CAPACITY
    assert "84" in msg and "83" in msg and "parked" in msg, msg
    torch.cuda.synchronize()
    assert bool((xpos == 7.0).all())  # nothing ran
    with pytest.raises(StacHipError, match="error -3"):
        eng.m_partial(np.zeros((3, 3 * t.nsite), np.float32), q)
    eng.close()
    t2 = _comb_tables(40)
    eng2, orc2 = Engine(t2, *_free_box(t2)), Oracle(t2)
    q2 = _poses(t2, 2, 13)
    out = eng2.fk(q2)
    for i in range(2):
        r = orc2.fk(q2[i].copy())
        for k in ("xpos", "xquat", "site_xpos", "qpos"):
            np.testing.assert_array_equal(_np(out[k][i]), r[k], err_msg=k)
    eng2.close()
