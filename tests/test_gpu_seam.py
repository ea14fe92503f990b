"""Warm-started clips (stac.seam_passes) and pose steps (stac.seam_report) on the GPU: the kernel of csrc/seam/stac_seam.hip against
the CPU build of its rule (tests/seam_cases.py) at tolerance 0 on every output word, twice; Stac.ik_only(passes=P) against a
restatement driven by the oracle's ik_clips at tolerance 0, also continuous, with the LM solver, with one clip and with two ranks of a
real process group; and both keys through run_stac."""

import json

import numpy as np
import pytest
import torch

import host_scaffold as hs
import seam_cases as sc

pytestmark = pytest.mark.gpu

FIELDS = ("qpos", "xpos", "xquat", "marker_sites")


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return sc.cpu_rule(tmp_path_factory)


def gpu_steps(q, L, cols, n_lin, poison):
    """seam.seam_steps of a host series -> the six outputs as numpy; the allocator's blocks are filled with ``poison`` first, so an
    output word that the call leaves unwritten shows"""
    from stac_mjx_amd import seam

    N, nq = q.shape
    junk = [torch.full((n,), poison, dtype=torch.float32, device="cuda") for n in (N, N, N, N, nq, nq)]
    del junk
    out = seam.seam_steps(torch.as_tensor(q).cuda(), L, cols, n_lin)
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- kernel against the CPU rule, tolerance 0 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", sc.NQS)
def test_kernel_equals_the_rule(rule, nq):
    steps, _ = rule
    for label, q, L, cols, n_lin in sc.cases(nq):
        want = steps(q, L, cols, n_lin)
        sc.same(gpu_steps(q, L, cols, n_lin, float("nan")), want, label)
        sc.same(gpu_steps(q, L, cols, n_lin, 1e30), want, label + " (second call)")


def test_kernel_on_many_workgroups_and_on_the_widest_row(rule):
    """1000 rows are 8 workgroups whose column maxima meet in the atomic maximum; 4096 columns are the most a call takes (64 columns
    per lane, 48 KiB of LDS)"""
    steps, _ = rule
    for N, nq, L in ((1000, 74, 250), (1000, 74, 50), (130, 4096, 13)):
        for cols, n_lin in sc.layouts(nq)[-2:]:
            q = sc.series(N, nq, cols, N + nq, quantised=False)
            want = steps(q, L, cols, n_lin)
            for poison in (float("nan"), 1e30):
                sc.same(gpu_steps(q, L, cols, n_lin, poison), want, f"N{N}_nq{nq}_L{L}_quat{len(cols)}")


@pytest.mark.parametrize("value,where", sc.POISONS)
def test_kernel_with_values_that_are_not_finite(rule, value, where):
    steps, _ = rule
    for N, nq in ((65, 74), (130, 230)):
        label, q, L, cols, n_lin = sc.poisoned(N, nq, value, where)
        sc.same(gpu_steps(q, L, cols, n_lin, 1e30), steps(q, L, cols, n_lin), label)


def test_kernel_past_2_31_elements(rule):
    """524 416 rows of 4096 columns: the last rows lie behind element 2^31 (8.6 GB).  Every row's step_joint against torch's
    subtraction, absolute value and maximum (exact operations: the same bits), in slabs; the last rows against the CPU rule"""
    from stac_mjx_amd import seam

    steps, _ = rule
    N, nq, L = 4097 * 128, 4096, 4097
    assert (N - 3) * nq > 2**31
    q = torch.empty((N, nq), dtype=torch.float32, device="cuda")
    torch.manual_seed(5)
    slab = 1 << 15
    for lo in range(0, N, slab):
        q[lo:lo + slab].normal_(0.0, 0.3)
    out = seam.seam_steps(q, L)
    col_in = torch.zeros(nq, device="cuda")
    col_seam = torch.zeros(nq, device="cuda")
    for lo in range(1, N, slab):
        d = (q[lo:lo + slab] - q[lo - 1:min(lo + slab, N) - 1]).abs()
        best, arg = d.max(dim=1)
        assert torch.equal(out["step_joint"][lo:lo + slab], best), lo
        col = out["step_col"][lo:lo + slab].to(torch.int64)
        assert torch.equal(d.gather(1, col[:, None])[:, 0], best) and bool((col <= arg).all()), lo  # (it attains the maximum, and no later than torch's)
        seam_rows = (torch.arange(lo, lo + d.shape[0], device="cuda") % L) == 0
        col_seam = torch.maximum(col_seam, d[seam_rows].amax(dim=0)) if bool(seam_rows.any()) else col_seam
        col_in = torch.maximum(col_in, d[~seam_rows].amax(dim=0))
    assert torch.equal(out["col_max_in"], col_in) and torch.equal(out["col_max_seam"], col_seam)
    tail = q[N - 4:].cpu().numpy()
    want = steps(tail, 4)
    for k in ("step_joint", "step_col", "step_rot", "step_lin2"):
        assert np.array_equal(sc.bits(out[k][N - 3:].cpu().numpy()), sc.bits(want[k][1:])), k
    assert float(out["step_joint"][0]) == 0.0 and int(out["step_col"][0]) == -1


def test_wrapper_refusals_on_the_device():
    from stac_mjx_amd import seam
    from stac_mjx_amd.engine import StacHipError

    q = torch.zeros((10, 7), device="cuda")
    with pytest.raises(ValueError, match="CUDA tensor"):
        seam.seam_steps(q.cpu(), 5)
    with pytest.raises(StacHipError, match="not whole clips"):
        seam.seam_steps(q, 3)
    with pytest.raises(StacHipError, match="overlap"):
        seam.seam_steps(q, 5, (0, 2))
    out = seam.seam_steps(q, 5, (3,), 3)  # (the refusals leave the library usable)
    assert not out["step_joint"].any() and (out["step_col"] == -1).all()


# ---- Stac.ik_only(passes=P) against the oracle-driven restatement -------------------------------------------------------------------
def _stac(rodent_setup, rodent_cfg, logs=None, **over):
    from stac_mjx_amd.stac import Stac

    stac = Stac(None, hs.stage_cfg(rodent_cfg, **over), rodent_setup.kp_names, setup=rodent_setup, verbose=logs is not None)
    if logs is not None:
        stac._log = lambda *a: logs.append(" ".join(str(x) for x in a))
    return stac


def _oracle(rodent_setup, rodent_cfg, offsets):
    from oracle import Oracle

    orc = Oracle(rodent_setup.tables, tol=float(rodent_cfg["FTOL"]), maxiter=int(rodent_cfg["N_ITER_Q"]))
    orc.set_site_pos(offsets)
    return orc


def _flat(out, name):
    a = out[name]
    return a.reshape((-1,) + a.shape[2:])


def _assert_equal(data, out, frame_error=None, label=""):
    for name in FIELDS:
        np.testing.assert_array_equal(getattr(data, name), _flat(out, name), err_msg=f"{label} {name}")
    if frame_error is not None:
        np.testing.assert_array_equal(frame_error, out["frame_error"], err_msg=f"{label} frame_error")


@pytest.fixture(scope="module")
def offsets(rodent_setup):
    rng = np.random.default_rng(11)
    return (rodent_setup.tables.site_pos + rng.normal(0.0, 0.002, rodent_setup.tables.site_pos.shape)).astype(np.float32)


@pytest.fixture(scope="module")
def clips_3x4(rodent_setup, rodent_cfg, rodent_mocap, offsets):
    """The rodent, 3 clips x 4 frames, and the oracle's three passes over them, computed once"""
    kp = rodent_mocap[300:312].astype(np.float32)
    outs = sc.oracle_seam_passes(_oracle(rodent_setup, rodent_cfg, offsets), rodent_setup, kp.reshape(3, 4, -1), 3)
    return kp, outs


def test_ik_only_passes_equal_the_restatement(rodent_setup, rodent_cfg, offsets, clips_3x4):
    from stac_mjx_amd import seam

    kp, outs = clips_3x4
    scalar = seam.scalar_columns(rodent_setup.tables.nq, (3,), 3)
    # the oracle sees the pass: clips 1 .. move, clip 0 does not
    moved = np.abs(outs[1]["qpos"][1:][..., scalar] - outs[0]["qpos"][1:][..., scalar]).max()
    assert moved > 0.05 and np.array_equal(outs[1]["qpos"][0], outs[0]["qpos"][0]), moved
    errors = {}
    for passes in (1, 2, 3):
        logs = []
        stac = _stac(rodent_setup, rodent_cfg, logs, n_frames_per_clip=4)
        keep = {}
        q_phase = stac.engine.q_phase

        def spy(kp_dev, **kw):
            res = q_phase(kp_dev, **kw)
            keep.setdefault("calls", []).append((int(kp_dev.shape[0]), bool(kw["do_root_opt"]), kw.get("q_init") is not None))
            keep["frame_error"] = res["frame_error"]
            return res

        stac.engine.q_phase = spy
        data = stac.ik_only(kp, offsets, passes=passes)
        assert keep["calls"] == [(3, rodent_setup.do_root_opt, False)] + [(2, False, True)] * (passes - 1)
        _assert_equal(data, outs[passes - 1], label=f"passes={passes}")
        errors[passes] = keep["frame_error"].cpu().numpy()
        assert sum(line.startswith("seam_passes: pass") for line in logs) == passes - 1, logs
    # frame_error of the last pass: its launch wrote into the slice behind clip 0 of pass 1's tensor
    for passes in (2, 3):
        np.testing.assert_array_equal(errors[passes], outs[passes - 1]["frame_error"][1:])
    # with the config key instead of the argument, and passes=1 against a call without the argument
    by_key = _stac(rodent_setup, rodent_cfg, seam_passes=2, n_frames_per_clip=4).ik_only(kp, offsets)
    _assert_equal(by_key, outs[1], label="stac.seam_passes: 2")
    plain = _stac(rodent_setup, rodent_cfg, n_frames_per_clip=4)
    a, b = plain.ik_only(kp, offsets), plain.ik_only(kp, offsets, passes=1)
    for name in FIELDS:
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name))
    _assert_equal(a, outs[0], label="no argument")
    over = _stac(rodent_setup, rodent_cfg, seam_passes=3, n_frames_per_clip=4).ik_only(kp, offsets, passes=1)  # (the argument wins)
    _assert_equal(over, outs[0], label="passes=1 over stac.seam_passes: 3")


def test_the_warm_start_row_is_the_carry(rodent_setup, rodent_cfg, offsets, clips_3x4):
    """Row F - 1 of a clip's qpos is bit for bit the clip's carry_qpos, on the device as in the oracle's pose_optimization"""
    kp, outs = clips_3x4
    stac = _stac(rodent_setup, rodent_cfg, n_frames_per_clip=4)
    stac.engine.set_site_pos(torch.as_tensor(offsets))
    res = stac._q_phase(torch.as_tensor(kp.reshape(3, 4, -1)).cuda(), do_root_opt=rodent_setup.do_root_opt)
    assert torch.equal(res["qpos"][:, 3].contiguous().view(torch.int32), res["carry_qpos"].view(torch.int32))
    orc, fs = _oracle(rodent_setup, rodent_cfg, offsets), rodent_setup
    out = orc.pose_optimization(kp[:4], outs[0]["qpos"][0, 0], fs.lb, fs.ub, fs.part_masks)
    assert np.array_equal(out["qpos"][3].view(np.uint32), out["carry_qpos"].view(np.uint32))


def test_ik_only_passes_continuous(rodent_setup, rodent_cfg, rodent_mocap, offsets):
    """36 rows, F = 12: three windows of 22 rows; the warm start of window c is row 11 of window c - 1, the frame in front of it"""
    from stac_mjx_amd import utils

    kp = rodent_mocap[300:336].astype(np.float32)
    windows = utils.batch_kp_data(kp, 12, continuous=True)
    assert windows.shape[:2] == (3, 22) and np.array_equal(windows[1, 0], kp[12]) and np.array_equal(windows[0, 11], kp[11])
    outs = sc.oracle_seam_passes(_oracle(rodent_setup, rodent_cfg, offsets), rodent_setup, windows, 2, F=12)
    assert not np.array_equal(outs[1]["qpos"][1], outs[0]["qpos"][1])
    stac = _stac(rodent_setup, rodent_cfg, n_frames_per_clip=12, continuous=True)
    _assert_equal(stac.ik_only(kp, offsets, passes=2), outs[1], label="continuous")
    _assert_equal(stac.ik_only(kp, offsets), outs[0], label="continuous, one pass")


def test_ik_only_passes_with_the_lm_solver(rodent_setup, rodent_cfg, offsets, clips_3x4):
    kp, pg = clips_3x4
    outs = sc.oracle_seam_passes(_oracle(rodent_setup, rodent_cfg, offsets), rodent_setup, kp.reshape(3, 4, -1), 2, solver="lm", maxiter=20,
                                 lambda0=1e-2)
    assert not np.array_equal(outs[1]["qpos"][1], outs[0]["qpos"][1]) and not np.array_equal(outs[1]["qpos"], pg[1]["qpos"])
    stac = _stac(rodent_setup, rodent_cfg, n_frames_per_clip=4, solver="lm")
    _assert_equal(stac.ik_only(kp, offsets, passes=2), outs[1], label="lm")


def test_ik_only_passes_with_one_clip(rodent_setup, rodent_cfg, offsets, clips_3x4):
    kp, _ = clips_3x4
    logs = []
    stac = _stac(rodent_setup, rodent_cfg, logs, n_frames_per_clip=12)
    calls = []
    q_phase = stac.engine.q_phase
    stac.engine.q_phase = lambda *a, **kw: calls.append(1) or q_phase(*a, **kw)
    data = stac.ik_only(kp, offsets, passes=3)
    assert len(calls) == 1 and sum("seam_passes" in line for line in logs) == 1 and any("one clip" in line for line in logs)
    one = _stac(rodent_setup, rodent_cfg, n_frames_per_clip=12).ik_only(kp, offsets)
    for name in FIELDS:
        np.testing.assert_array_equal(getattr(data, name), getattr(one, name))


# ---- two ranks ------------------------------------------------------------------------------------------------------------------------
def _two_rank_ik(rank, port, tmp, kp, offsets, gather):
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
        stac = Stac(None, hs.stage_cfg(mcfg, n_frames_per_clip=4), fs.kp_names, setup=fs, verbose=False)
        data = stac.ik_only(kp, offsets, gather=gather, passes=3)
        np.savez(f"{tmp}/{gather}_rank{rank}.npz", **{name: getattr(data, name) for name in FIELDS})
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("gather", ("rank0", "none"))
def test_ik_only_passes_two_ranks_on_one_gpu(tmp_path, clips_3x4, offsets, gather):
    """A real process group (2 ranks sharing cuda:0, gloo): the clips split 2 + 1, so clip 2 on rank 1 starts from the row that
    rank 0's clip 1 ended in, which the all-gather of every pass brings: the bits of the single-process run"""
    import torch.multiprocessing as mp

    kp, outs = clips_3x4
    port = 29700 + int(torch.randint(0, 90, (1,)).item())
    mp.spawn(_two_rank_ik, args=(port, str(tmp_path), kp, offsets, gather), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / f"{gather}_rank0.npz"), np.load(tmp_path / f"{gather}_rank1.npz")
    for name in FIELDS:
        want = _flat(outs[2], name)
        np.testing.assert_array_equal(r1[name], want[8:], err_msg=f"rank 1 {name}")  # (its shard under both modes)
        np.testing.assert_array_equal(r0[name], want if gather == "rank0" else want[:8], err_msg=f"rank 0 {name}")


# ---- run_stac -----------------------------------------------------------------------------------------------------------------------
def test_run_stac_with_seam_passes_and_the_report(tmp_path, rodent_setup, rodent_cfg, rodent_mocap):
    from stac_mjx_amd import seam
    from stac_mjx_amd.io import load_stac_data
    from stac_mjx_amd.main import run_stac, seams_path

    fs = rodent_setup
    kp = rodent_mocap[300:312].astype(np.float32)
    over = dict(n_fit_frames=4, n_frames_per_clip=4, postprocess="gpu", infer_qvels=True)
    cfg = hs.stage_cfg(rodent_cfg, seam_passes=2, seam_report="on", **over)
    cfg.model.N_ITERS = 1
    fit_path, ik_path = run_stac(cfg, kp, fs.kp_names, base_path=tmp_path, setup=fs)
    stored, ik = load_stac_data(ik_path)
    assert int(stored.stac.seam_passes) == 2 and stored.stac.seam_report == "on"
    _, fit = load_stac_data(fit_path)
    direct = _stac(rodent_setup, rodent_cfg, **over)
    two, one = direct.ik_only(kp, fit.offsets, passes=2), direct.ik_only(kp, fit.offsets)
    for name in FIELDS:
        np.testing.assert_array_equal(getattr(ik, name), getattr(two, name), err_msg=name)
    assert not np.array_equal(two.qpos, one.qpos) and np.asarray(ik.qvel).shape[0] == 12
    summary = json.loads(seams_path(ik_path).read_text())
    scalar = seam.scalar_columns(fs.tables.nq, (3,), 3)
    jumps = np.abs(ik.qpos[[4, 8]][:, scalar] - ik.qpos[[3, 7]][:, scalar])
    assert summary["n_rows"] == 12 and summary["clip_len"] == 4 and summary["n_seams"] == 2 and summary["seams"]["row"] == [4, 8]
    assert summary["seams"]["step_joint"] == [float(v) for v in jumps.max(axis=1)]
    assert summary["seams"]["step_col"] == [fs.part_names[scalar[j]] for j in jumps.argmax(axis=1)]
    assert summary["seam_max"] == float(jumps.max()) and summary["within"]["n"] == 9 and len(summary["col_max_seam"]) == fs.tables.nq
    assert summary["marker_error_mm"] > 0 and summary["marker_error_first_frames_mm"] > 0
    steps = direct.seam_steps(ik_path)  # (the stored config decides the clips)
    assert steps["summary"] == summary and steps["step_joint"].shape == (12,) and steps["step_col"][0] == -1
    lin = np.linalg.norm(np.diff(ik.qpos[:, :3].astype(np.float64), axis=0), axis=1)
    np.testing.assert_allclose(np.sqrt(steps["step_lin2"][1:]), lin, rtol=1e-5, atol=1e-9)
    # the seams that the second pass closed, measured by the same instrument on a run without it
    cfg1 = hs.stage_cfg(rodent_cfg, seam_report=True, skip_fit_offsets=True, ik_only_path="ik1.h5", **over)
    _, ik1_path = run_stac(cfg1, kp, fs.kp_names, base_path=tmp_path, setup=fs)
    stored1, ik1 = load_stac_data(ik1_path)
    assert int(stored1.stac.seam_passes) == 1 and stored1.stac.seam_report == "on"  # (the fit file's said 2: this run's is recorded)
    np.testing.assert_array_equal(ik1.qpos, one.qpos)
    assert json.loads(seams_path(ik1_path).read_text())["seam_mean"] > summary["seam_mean"]
    # without the key: no sidecar
    cfg0 = hs.stage_cfg(rodent_cfg, skip_fit_offsets=True, ik_only_path="ik0.h5", **over)
    _, ik0_path = run_stac(cfg0, kp, fs.kp_names, base_path=tmp_path, setup=fs)
    assert not seams_path(ik0_path).exists()
