"""The offset phase on observed keypoints only (stac.offset_mask) on the GPU: the kernels of csrc/mmask/stac_mmask.hip against the CPU
build of their rule (tests/mmask_cases.py) at tolerance 0 on every output word, the entry points' refusals with real buffers, the
all-valid case against stac_m_phase_partial / stac_m_phase_finish, Stac.fit_offsets(valid=...) against a restatement driven by
the oracle and the CPU rule, and stac.offset_mask: observed through run_stac."""

import ctypes as C

import numpy as np
import pytest
import torch

import host_scaffold as hs
import mmask_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return mc.cpu_rule(tmp_path_factory)


@pytest.fixture(scope="module")
def lib():
    from stac_mjx_amd.build import build_extension
    from stac_mjx_amd.engine import load_mmask_library

    build_extension()
    return load_mmask_library()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).cuda()


def gpu_partial(lib, kp, xpos, xquat, bodyid, valid, calls=1):
    """stac_mmask_partial on the current stream -> list of ``calls`` partials [4K + 2] (numpy), each into a poisoned buffer with a
    poisoned workspace of its own"""
    T, nbody, K = xpos.shape[0], xpos.shape[1], len(bodyid)
    d = [_dev(kp, np.float32), _dev(xpos, np.float32), _dev(xquat, np.float32), _dev(bodyid, np.int32), _dev(np.asarray(valid) != 0, np.uint8)]
    nbytes = lib.stac_mmask_workspace(T, K)
    assert nbytes >= 8
    out = []
    for i in range(calls):
        ws = torch.full((nbytes // 4,), float("nan") if i % 2 == 0 else 1e30, dtype=torch.float32, device="cuda")
        partial = torch.full((4 * K + 2,), -7.0, dtype=torch.float32, device="cuda")
        rc = lib.stac_mmask_partial(_p(d[0]), _p(d[1]), _p(d[2]), nbody, _p(d[3]), _p(d[4]), T, K, _p(ws), nbytes, _p(partial),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.stac_mmask_last_error().decode()
        out.append(partial.cpu().numpy())
    return out


def gpu_finish(lib, partial, m0, dreg, lam):
    K = (len(partial) - 2) // 4
    d = [_dev(partial, np.float32), _dev(m0, np.float32), _dev(dreg, np.float32)]
    off = torch.full((K, 3), -7.0, dtype=torch.float32, device="cuda")
    err = torch.full((1,), -7.0, dtype=torch.float32, device="cuda")
    n = torch.full((K,), -7, dtype=torch.int32, device="cuda")
    rc = lib.stac_mmask_finish(_p(d[0]), K, _p(d[1]), _p(d[2]), float(lam), _p(off), _p(err), _p(n), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.stac_mmask_last_error().decode()
    return off.cpu().numpy(), err.cpu().numpy()[0], n.cpu().numpy()


def _same_finish(a, b, label):
    assert np.array_equal(_bits(a[0]), _bits(b[0])), (label, "offsets")
    assert _bits(a[1]) == _bits(b[1]), (label, "err", a[1], b[1])
    assert np.array_equal(a[2], b[2]), (label, "n")


# ---- kernel against the CPU rule, tolerance 0 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", mc.TS)
def test_kernels_equal_the_cpu_rule(lib, rule, T):
    partial, finish, _ = rule
    for K in mc.KS:
        for kind in mc.MASKS:
            label, kp, xpos, xquat, bodyid, valid, m0, dreg, lam = mc.case(T, K, kind)
            want = partial(kp, xpos, xquat, bodyid, valid)
            got = gpu_partial(lib, kp, xpos, xquat, bodyid, valid)[0]
            assert np.array_equal(_bits(got), _bits(want)), (label, np.flatnonzero(_bits(got) != _bits(want))[:8])
            for lam_i in (lam, 0.0):
                _same_finish(gpu_finish(lib, got, m0, dreg, lam_i), finish(want, m0, dreg, lam_i), f"{label}_lam{lam_i}")


def test_fillers_and_a_second_call_give_the_same_bits(lib, rule):
    partial, _, _ = rule
    label, kp, xpos, xquat, bodyid, valid, m0, dreg, lam = mc.case(1000, 23, "random30")
    assert not np.isfinite(kp).all()
    a, b, c = gpu_partial(lib, kp, xpos, xquat, bodyid, valid, calls=3)  # (workspaces poisoned with NaN, 1e30, NaN)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c)) and np.isfinite(a).all()
    clean = np.where(np.repeat(valid, 3, axis=1), kp, 0.0).astype(np.float32)
    assert np.array_equal(_bits(gpu_partial(lib, clean, xpos, xquat, bodyid, valid)[0]), _bits(a))
    _same_finish(gpu_finish(lib, a, m0, dreg, lam), gpu_finish(lib, a, m0, dreg, lam), label)
    # a NaN that the mask calls an observation propagates, as in the rule
    t, k = (int(i) for i in np.argwhere(valid)[11])
    kp2 = kp.copy()
    kp2[t, 3 * k] = np.nan
    got, want = gpu_partial(lib, kp2, xpos, xquat, bodyid, valid)[0], partial(kp2, xpos, xquat, bodyid, valid)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[3 * k]) and np.isnan(got[4 * 23])
    ok = ~np.isnan(want)
    assert np.array_equal(_bits(got[ok]), _bits(want[ok]))


def test_body_outside_the_model(lib, rule):
    partial, _, _ = rule
    _, kp, xpos, xquat, bodyid, valid, *_ = mc.case(65, 23, "all_valid")
    b = bodyid.copy()
    b[[0, 22]] = [-1, mc.NBODY]
    assert np.array_equal(_bits(gpu_partial(lib, kp, xpos, xquat, b, valid)[0]), _bits(partial(kp, xpos, xquat, b, valid)))


def test_no_frames(lib, rule):
    partial, finish, _ = rule
    K = 23
    _, kp, xpos, xquat, bodyid, valid, m0, dreg, lam = mc.case(1, K, "all_valid")
    bid = _dev(bodyid, np.int32)
    ws = torch.full((2,), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.full((4 * K + 2,), -7.0, dtype=torch.float32, device="cuda")
    assert lib.stac_mmask_workspace(0, K) == 8
    rc = lib.stac_mmask_partial(None, None, None, mc.NBODY, _p(bid), None, 0, K, _p(ws), 8, _p(out), None)
    assert rc == 0, lib.stac_mmask_last_error().decode()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got), np.zeros(4 * K + 2, np.uint32))  # (+0 everywhere, T = 0 among them)
    assert np.array_equal(_bits(got), _bits(partial(kp[:0], xpos[:0], xquat[:0], bodyid, valid[:0])))
    _same_finish(gpu_finish(lib, got, m0, dreg, lam), finish(got, m0, dreg, lam), "T0")
    off, err, n = gpu_finish(lib, got, m0, np.zeros_like(dreg), lam)
    assert np.array_equal(_bits(off), _bits(m0)) and err == 0 and not n.any()


def test_refusals_with_real_buffers(lib):
    """Misaligned, overlapping and NULL arguments are refused before a launch: the outputs keep their poison"""
    T, K, nbody = 64, 3, mc.NBODY
    _, kp, xpos, xquat, bodyid, valid, m0, dreg, lam = mc.case(T, K, "all_valid")
    nbytes = lib.stac_mmask_workspace(T, K)
    big = torch.full((T * 3 * K + 16,), 0.25, dtype=torch.float32, device="cuda")  # kp lives in it, so that neighbours can overlap it
    big[: T * 3 * K] = _dev(kp, np.float32).reshape(-1)
    d = dict(kp=big.data_ptr(), xpos=_dev(xpos, np.float32), xquat=_dev(xquat, np.float32), bodyid=_dev(bodyid, np.int32),
             valid=_dev(valid, np.uint8), ws=torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda"),
             partial=torch.full((4 * K + 2,), -7.0, dtype=torch.float32, device="cuda"))
    ptr = lambda v: C.c_void_p(v) if isinstance(v, int) else _p(v)  # noqa: E731

    def call(**over):
        a = dict(d)
        a.update(over)
        return lib.stac_mmask_partial(ptr(a["kp"]), ptr(a["xpos"]), ptr(a["xquat"]), nbody, ptr(a["bodyid"]), ptr(a["valid"]), T, K, ptr(a["ws"]),
                                      a.get("nbytes", nbytes), ptr(a["partial"]), None)

    for over, word in ((dict(kp=big.data_ptr() + 2), "kp must be 4-byte aligned"), (dict(partial=d["partial"].data_ptr() + 1), "partial must be 4-byte"),
                       (dict(ws=d["ws"].data_ptr() + 2), "workspace must be 4-byte"), (dict(partial=big.data_ptr() + 8), "kp and partial overlap"),
                       (dict(ws=d["xquat"]), "xquat and workspace overlap"), (dict(partial=d["ws"].data_ptr() + nbytes - 4), "workspace and partial overlap"),
                       (dict(kp=None), "null kp"), (dict(valid=None), "null valid"), (dict(partial=None), "null partial"), (dict(ws=None), "null workspace"),
                       (dict(nbytes=nbytes - 1), "workspace_bytes")):
        rc = call(**over)
        msg = lib.stac_mmask_last_error().decode()
        assert rc == hs.STAC_ERR_INVALID and lib.stac_mmask_last_error_code() == rc and word in msg, (over, rc, msg)
    torch.cuda.synchronize()
    assert (d["partial"] == -7.0).all() and not d["ws"].any() and (big[T * 3 * K:] == 0.25).all()
    part = _dev(np.zeros(4 * K + 2), np.float32)
    m0d, dd = _dev(m0, np.float32), _dev(dreg, np.float32)
    off = torch.full((K, 3), -7.0, dtype=torch.float32, device="cuda")
    for args, word in (((_p(part), K, _p(m0d), _p(dd), 1.0, _p(m0d), None, None, None), "m0 and offsets_out overlap"),
                       ((_p(part), K, _p(m0d), _p(dd), 1.0, None, None, None, None), "null offsets_out"),
                       ((_p(part), K, _p(m0d), _p(dd), 1.0, C.c_void_p(off.data_ptr() + 2), None, None, None), "offsets_out must be 4-byte")):
        rc = lib.stac_mmask_finish(*args)
        assert rc == hs.STAC_ERR_INVALID and word in lib.stac_mmask_last_error().decode(), word
    assert lib.stac_mmask_finish(_p(part), K, _p(m0d), _p(dd), 1.0, _p(off), None, None, None) == 0  # (err_out and n_out are optional)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(off.cpu().numpy()), _bits(m0))  # (no frames, lam = 1, d in {0, 1}: 1 * 1 * m0 / 1 where regularised, m0 else)


# ---- the model's path ------------------------------------------------------------------------------------------------------------
def _cfg(rodent_cfg, **stac_over):
    return hs.stage_cfg(rodent_cfg, n_fit_frames=30, **stac_over)


def test_all_valid_equals_the_unmasked_offset_phase_on_the_rodent(rodent_setup, rodent_cfg, rodent_mocap):
    from stac_mjx_amd.stac import Stac

    fs = rodent_setup
    stac = Stac(None, _cfg(rodent_cfg), fs.kp_names, setup=fs, verbose=False)
    eng = stac.engine
    kp = torch.as_tensor(rodent_mocap[:30].astype(np.float32)).to(eng.device)
    res = stac._q_phase(kp[None], do_root_opt=True)
    K = eng.K
    valid = np.ones((30, K), bool)
    masked = eng.m_partial_masked(kp, res["xpos"][0], res["xquat"][0], valid)
    plain = eng.m_partial(kp, res["qpos"][0])
    assert torch.equal(masked[: 3 * K].view(torch.int32), plain[: 3 * K].view(torch.int32))
    assert torch.equal(masked[4 * K:].view(torch.int32), plain[3 * K:].view(torch.int32))  # z2 and T
    assert (masked[3 * K: 4 * K] == 30).all()
    # ... and with the kinematics that fit_offsets feeds it: stac_fk of the poses
    fk = eng.fk(res["qpos"][0], want=("xpos", "xquat"))
    assert torch.equal(eng.m_partial_masked(kp, fk["xpos"], fk["xquat"], valid).view(torch.int32), masked.view(torch.int32))
    m0, lam = eng.get_site_pos(), float(rodent_cfg["M_REG_COEF"])
    off, err, n = eng.m_finish_masked(masked, m0, fs.is_regularized, lam)
    off0, err0 = eng.m_finish(plain, m0, fs.is_regularized, lam)
    assert torch.equal(off.view(torch.int32), off0.view(torch.int32)) and (n == 30).all()
    # err differs by the rounding of its sum n (v v) against T * sum v v alone: each is a serial sum of 3 K terms with one or two more
    # products, within (3 K + 2) U of X = T sum v^2, and the three operations that follow add 4 U of the larger of z2 and X
    X = 30.0 * float((off.double() ** 2).sum())
    assert abs(float(err) - float(err0)) <= (2 * (3 * K + 2) + 4) * mc.U * max(float(plain[3 * K]), X)
    # the seam
    core = stac.stac_core_obj
    r = core.m_opt(None, None, kp, res["qpos"][0], m0, torch.as_tensor(fs.is_regularized), lam, valid=valid)
    assert torch.equal(r.params.view(torch.int32), off.view(torch.int32)) and torch.equal(r.error, err[0])


def test_fit_offsets_with_holes_equals_the_restatement(rule, rodent_setup, rodent_cfg, rodent_mocap):
    """Stac.fit_offsets(valid=...), N_ITERS = 2, on 30 strided golden rows with holes in 4 keypoints, against the reference's
    sequencing driven by the oracle's pose_optimization and kinematics and the CPU rule: offsets and final qpos at tolerance 0."""
    from oracle import Oracle
    from stac_mjx_amd.prng import sample_time_indices
    from stac_mjx_amd.select import select_strided
    from stac_mjx_amd.stac import Stac

    partial, finish, _ = rule
    fs, n_iters = rodent_setup, 2
    rows = select_strided(1000, 30)
    filled, valid, which = mc.cut_holes(rodent_mocap[rows].astype(np.float32), 4, 10, 5)
    cfg = _cfg(rodent_cfg)
    cfg.model.N_ITERS = n_iters
    logs = []
    stac = Stac(None, cfg, fs.kp_names, setup=fs, verbose=True)
    stac._log = lambda *a: logs.append(" ".join(str(x) for x in a))
    data = stac.fit_offsets(filled, valid=valid)
    # the restatement (helpers.oracle_fit_offsets with the masked offset phase)
    orc = Oracle(fs.tables, tol=float(rodent_cfg["FTOL"]), maxiter=int(rodent_cfg["N_ITER_Q"]))
    offsets = fs.tables.site_pos.astype(np.float32).copy()
    q = fs.tables.qpos0
    if fs.do_root_opt:
        q, _ = orc.root_optimization(filled, q, fs.lb, fs.ub, fs.trunk_kps, fs.root_kp_idx, fs.root_dims)
    idx = sample_time_indices(30, int(rodent_cfg["N_SAMPLE_FRAMES"]))
    for _ in range(n_iters):
        out = orc.pose_optimization(filled, q, fs.lb, fs.ub, fs.part_masks)
        q = out["carry_qpos"]
        xpos, xquat = mc.oracle_bodies(orc, out["qpos"][idx])
        offsets, _, n = finish(partial(filled[idx], xpos, xquat, fs.tables.site_bodyid, valid[idx]), offsets, fs.is_regularized,
                               float(rodent_cfg["M_REG_COEF"]))
        orc.set_site_pos(offsets)
    out = orc.pose_optimization(filled, q, fs.lb, fs.ub, fs.part_masks)
    np.testing.assert_array_equal(data.offsets, offsets)
    np.testing.assert_array_equal(data.qpos, out["qpos"])
    np.testing.assert_array_equal(data.marker_sites, out["marker_sites"])
    assert np.array_equal(stac.offset_counts["n"], n) and stac.offset_counts["n_sampled"] == len(idx)
    assert (n[which] < len(idx)).all() and (np.delete(n, which) == len(idx)).all()
    assert sum("offset phase on observed keypoints: 0 of 23 keypoints" in line for line in logs) == n_iters
    # the mask changes the fit: the same call without it gives other offsets for the holed keypoints
    plain = Stac(None, cfg, fs.kp_names, setup=fs, verbose=False).fit_offsets(filled)
    assert np.abs(plain.offsets[which] - data.offsets[which]).max() > 1e-5


def test_run_stac_with_the_offset_mask(tmp_path, rodent_setup, rodent_cfg, rodent_mocap):
    """stac.offset_mask: observed through run_stac: kp_gap of fill_missing is the mask, sliced with the strided fit rows that
    stac.fit_frames_min_observed admits; both sidecars are written; the offsets are those of Stac.fit_offsets(valid=...) on those rows"""
    import json

    from stac_mjx_amd.io import load_stac_data
    from stac_mjx_amd.main import frames_path, offset_counts_path, run_stac
    from stac_mjx_amd.stac import Stac

    fs = rodent_setup
    kp = rodent_mocap[:40].astype(np.float32).copy()
    holes = kp.reshape(40, 23, 3)
    holes[5:12, 4] = np.nan
    holes[20:35, 9] = np.nan
    holes[0, 1:4] = np.nan  # (three missing: 20 of 23 observed, below the 21 that q = 0.9 wants)
    over = dict(n_fit_frames=12, fill_missing="linear", offset_mask="observed", fit_frames="strided", fit_frames_min_observed=0.9, skip_ik_only=True)
    cfg = hs.stage_cfg(rodent_cfg, **over)
    cfg.model.N_ITERS = 1
    fit_path, _ = run_stac(cfg, kp, fs.kp_names, base_path=tmp_path, setup=fs)
    _, fit = load_stac_data(fit_path)
    rows = [1 + (i * 39) // 12 for i in range(12)]
    frames = json.loads(frames_path(fit_path).read_text())
    assert frames["indices"] == rows and frames["min_observed"] == 0.9 and frames["mode"] == "strided"
    gap = np.asarray(fit.kp_gap)
    missing = np.isnan(holes[rows]).any(axis=-1)
    assert gap.shape == (12, 23) and np.array_equal(gap != 0, missing) and np.isfinite(fit.kp_data).all()
    counts = json.loads(offset_counts_path(fit_path).read_text())
    assert counts["kp_names"] == list(fs.kp_names) and counts["n_sampled"] == 12 and counts["never_observed"] == []
    assert counts["n"] == (12 - missing.sum(axis=0)).tolist() and counts["n"][4] < 12 and counts["n"][9] < 12
    direct = Stac(None, cfg, fs.kp_names, setup=fs, verbose=False).fit_offsets(fit.kp_data, valid=gap == 0)
    np.testing.assert_array_equal(fit.offsets, direct.offsets)
    np.testing.assert_array_equal(fit.qpos, direct.qpos)
    # without the option: no sidecar of the counts
    cfg_off = hs.stage_cfg(rodent_cfg, n_fit_frames=12, fill_missing="linear", skip_ik_only=True, fit_offsets_path="plain.h5")
    cfg_off.model.N_ITERS = 1
    plain_path, _ = run_stac(cfg_off, kp, fs.kp_names, base_path=tmp_path, setup=fs)
    assert not offset_counts_path(plain_path).exists()


# ---- shards ----------------------------------------------------------------------------------------------------------------------
def _two_rank_masked_fit(rank, port, tmp, kp, valid, fpc):
    import json
    import os

    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2")
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        from conftest import GOLDEN as G
        from stac_mjx_amd.fit_model import finish_fit_setup
        from stac_mjx_amd.mjcf import ModelTables
        from stac_mjx_amd.stac import Stac

        mcfg = json.load(open(G / "rodent_model_cfg.json"))
        fs = finish_fit_setup(ModelTables.load(G / "rodent_tables.npz"), mcfg, list(mcfg["KEYPOINT_MODEL_PAIRS"].keys()))
        cfg = hs.stage_cfg(mcfg, n_fit_frames=10, fit_frames_per_clip=fpc)
        cfg.model.N_ITERS = 2
        stac = Stac(None, cfg, fs.kp_names, setup=fs, verbose=False)
        data = stac.fit_offsets(kp, valid=valid)
        np.savez(f"{tmp}/rank{rank}.npz", offsets=data.offsets, qpos=data.qpos, n=stac.offset_counts["n"])
    finally:
        dist.destroy_process_group()


def test_fit_offsets_with_a_mask_two_ranks_on_one_gpu(tmp_path, rodent_setup, rodent_cfg, rodent_mocap):
    """fit_frames_per_clip with a real process group (2 ranks sharing cuda:0, gloo): clips split 3 + 2, each rank's masked 4K + 2
    sums all-reduced in fixed rank order: both ranks end with the same offsets and the counts of the whole; the result agrees with the
    single-process run (the sums associate differently: 1e-5, as for the unmasked phase)."""
    import torch.multiprocessing as mp

    from stac_mjx_amd.stac import Stac

    fs = rodent_setup
    kp = rodent_mocap[300:311].astype(np.float32)  # 5 clips of 2, the ragged frame is dropped
    valid = np.ones((11, 23), bool)
    valid[2:5, 3] = False   # rank 0 owns clips 0 .. 2 = frames 0 .. 5
    valid[7:9, 11] = False  # rank 1 owns clips 3 .. 4 = frames 6 .. 9
    valid[10] = False       # (the dropped frame)
    cfg = hs.stage_cfg(rodent_cfg, n_fit_frames=10, fit_frames_per_clip=2)
    cfg.model.N_ITERS = 2
    stac = Stac(None, cfg, fs.kp_names, setup=fs, verbose=False)
    one = stac.fit_offsets(kp, valid=valid)
    assert np.array_equal(stac.offset_counts["n"], valid[:10].sum(axis=0)) and stac.offset_counts["n_sampled"] == 10
    port = 29900 + int(torch.randint(0, 90, (1,)).item())
    mp.spawn(_two_rank_masked_fit, args=(port, str(tmp_path), kp, valid, 2), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    np.testing.assert_array_equal(r0["offsets"], r1["offsets"])
    np.testing.assert_array_equal(r0["n"], valid[:10].sum(axis=0))
    np.testing.assert_array_equal(r1["n"], r0["n"])
    assert np.abs(r0["offsets"] - one.offsets).max() < 1e-5
    plain = Stac(None, cfg, fs.kp_names, setup=fs, verbose=False).fit_offsets(kp)
    assert np.abs(plain.offsets[[3, 11]] - one.offsets[[3, 11]]).max() > 1e-6  # (the mask is not a no-op)


def test_fit_offsets_with_a_mask_and_no_sampled_frame(rodent_setup, rodent_cfg, rodent_mocap):
    """What a rank sees whose shard holds no sampled frame: empty tensors, T = 0, zero sums; alone, nothing determines the offsets"""
    from stac_mjx_amd.stac import Stac

    fs = rodent_setup
    cfg = hs.stage_cfg(rodent_cfg, n_fit_frames=4)
    cfg.model.N_ITERS = 1
    logs = []
    stac = Stac(None, cfg, fs.kp_names, setup=fs, verbose=True)
    stac._log = lambda *a: logs.append(" ".join(str(x) for x in a))
    data = stac.fit_offsets(rodent_mocap[:4].astype(np.float32), time_indices=np.zeros(0, np.int64), valid=np.ones((4, 23), bool))
    assert not stac.offset_counts["n"].any() and stac.offset_counts["n_sampled"] == 0
    np.testing.assert_array_equal(data.offsets, fs.tables.site_pos.astype(np.float32))  # (lam = 1, d in {0, 1}: m0 either way)
    assert any("23 of 23 keypoints were observed in none of the 0 sampled frames" in line and fs.kp_names[0] in line for line in logs)
