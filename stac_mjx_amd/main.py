"""User-level pipeline with the reference's signatures (``stac_mjx/main.py``)."""

from __future__ import annotations

import time
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from . import dist, io, utils
from .config import (DONORS_NEED_FILL, GATHER_NONE_CONTINUOUS, OFFSET_MASK_NEEDS_FILL, PAIRWISE_NEEDS_FILL, POSTPROCESS_GPU_MARKER_ORDER, RESAMPLE_SHARDED, compose_config,
                     donor_options, fill_missing_options, fit_frames_options, ground_options, offset_mask_options, outlier_options, pairwise_options, postprocess_options, report_options, resample_options,
                     seam_options, smooth_options, swaps_candidates, swaps_options)
from .stac import Stac


def load_configs(config_dir, config_name: str = "config"):
    """``stac_mjx.main.load_configs`` (main.py:18-30)."""
    cfg = compose_config(config_dir, config_name=config_name)
    print("Config loaded and validated.")
    return cfg


def run_stac(cfg, kp_data, kp_names, base_path=None, *, setup=None, device=None):
    """``stac_mjx.main.run_stac`` (main.py:33-139): fit_offsets (unless skipped) then ik_only (unless skipped).

    Returns ``(fit_offsets_path, ik_only_path or None)``.  Raises ``ValueError`` when ``kp_data`` columns
    do not match ``3 * len(kp_names)`` or ``n_frames_per_clip`` does not divide the frame count.
    ``infer_qvels`` runs the reference's finite-difference post-processing on the host, or, like the
    cross-fade of a continuous run, on the device with ``stac.postprocess: gpu`` (DESIGN.md "Post-processing on the GPU").
    ``stac.fill_missing: linear | hold`` fills missing keypoints (NaN / infinite) of the whole series on the GPU before the fit
    and adds ``kp_gap`` to both files (DESIGN.md "Filling missing keypoints"); a keypoint without any valid frame is a ``ValueError``.
    ``stac.reject_outliers: hampel`` (needs ``fill_missing``) first turns keypoints that are finite but off their track's sliding
    median into missing ones, on the GPU, and adds ``kp_rejected`` to both files (DESIGN.md "Rejecting keypoint outliers").
    ``stac.reject_pairwise: mad`` (needs ``fill_missing``) does the same, ahead of it and on the raw series, to keypoints that leave
    the distributions of their distances to the other keypoints over the whole series, however long the defect lasts: ``kp_rejected``
    is then what either detector rejected and ``kp_rejected_pairwise`` this one's share (DESIGN.md "Rejecting keypoints by pairwise
    distances").
    ``stac.repair_swaps: lr`` (or a list of ``[nameA, nameB]`` pairs; needs no ``fill_missing``) first of all exchanges back, frame
    by frame, two keypoints of a pair that carry each other's label, on the GPU: ``kp_data`` of both files is the repaired series and
    ``kp_swapped`` marks both keypoints of every repaired pair (DESIGN.md "Repairing keypoint swaps"); unknown names and a keypoint
    in two pairs are a ``ValueError`` before any work.
    ``stac.fill_donors: auto`` (needs ``fill_missing``) fills, after the rejecters and directly in front of ``fill_missing``, a missing
    keypoint from the local frame of three rigid partners that are still tracked, on the GPU; what it cannot fill stays missing for
    ``fill_missing``, and ``kp_gap`` marks both kinds (DESIGN.md "Filling gaps from donor keypoints").
    ``stac.report: on`` computes the marker errors of each phase's final result on the GPU and writes them as
    ``<result file>.report.json`` next to the file (DESIGN.md "Fit report"); the result files themselves do not change.
    ``stac.smooth: savgol | gaussian`` (needs ``postprocess: gpu``) low-pass filters the ``qpos`` of the ik_only run along time on
    the GPU, per clip, after the stitch and before ``qvel``: the file's ``qpos`` / ``xpos`` / ``xquat`` / ``marker_sites`` / ``qvel``
    are those of the smoothed pose and ``qpos_raw`` keeps the fitted one (DESIGN.md "Smoothing fitted poses"); clips shorter than
    the window of ``2 * smooth_window + 1`` frames are a ``ValueError``.
    ``stac.resample: kaiser`` with ``stac.mocap_hz`` and ``stac.resample_hz`` (needs ``postprocess: gpu``) writes, after the ik_only
    file and without changing it, a second file next to it (``resampled_path``) that holds the result at the other rate, resampled per
    clip on the GPU by ``Stac.resample_result`` (DESIGN.md "Resampling fitted poses"); the two paths returned are those of today.
    ``stac.fit_frames: strided | diverse`` calibrates the offsets on ``n_fit_frames`` rows chosen from the whole prepared series
    instead of its first ones -- even steps, or the frames whose pairwise keypoint distances differ most, chosen on the GPU -- never
    on a frame that a preparation stage marked, and writes the choice as ``<fit file>.frames.json`` (DESIGN.md "Choosing calibration
    frames"); more ``n_fit_frames`` than frames, or than usable frames, is a ``ValueError``.
    ``stac.offset_mask: observed`` (needs ``fill_missing``) fits the offsets to observed keypoints only: the offset phase of
    ``fit_offsets`` leaves out every value with ``kp_gap > 0``, on the GPU, while the pose phase still sees the filled series, and
    ``<fit file>.offsets.json`` lists how many sampled frames observed each keypoint (DESIGN.md "Offsets from observed keypoints").
    With it ``stac.fit_frames_min_observed: q`` lets ``strided`` / ``diverse`` take a frame of which at least ``ceil(q K)`` keypoints
    are observed (default 1.0: all of them).
    ``stac.seam_passes: P`` (1 .. 8, default 1) lets ``ik_only`` solve the clips behind the first ``P - 1`` times more, each
    warm-started from the pose that the clip in front of it ended in, so that the clip borders stop carrying the jump of a cold start;
    ``stac.seam_report: on`` measures the pose steps of the ik_only result on the GPU and writes them as ``<ik file>.seams.json``
    (DESIGN.md "Warm-started clips and pose steps"); the ik_only file's stored config carries both keys.
    ``stac.ground: report`` measures on the GPU how far the geoms of the ik_only result are from the floor and writes
    ``<ik file>.ground.json`` (DESIGN.md "Ground clearance"); the result does not change.  ``stac.ground: level`` (models with a free
    root that the fit places) also subtracts ``floor_z``, the ``stac.ground_permille`` quantile of the per-frame lowest z, from ``qpos[:, 2]`` and from the
    z of ``xpos``, ``marker_sites`` and ``kp_data`` of the ik_only file, and records it in the sidecar and in the stored config; the
    fit file and the offsets are not touched.  Unknown geom or body names are a ``ValueError`` before any work.
    """
    base_path = Path.cwd() if base_path is None else Path(base_path)
    kp_data = np.asarray(kp_data)
    expected_cols = len(kp_names) * 3
    if kp_data.shape[1] != expected_cols:
        raise ValueError(
            f"kp_data has {kp_data.shape[1]} columns but expected {expected_cols} ({len(kp_names)} keypoints x 3). "
            "Ensure kp_data is shaped (n_frames, n_keypoints * 3) and that kp_names length matches the number of "
            "keypoints in kp_data.")
    start = time.time()
    fit_offsets_path = base_path / cfg.stac.fit_offsets_path
    ik_only_path = base_path / cfg.stac.ik_only_path
    pre = _Preflight(cfg, kp_data.shape[0], fit_offsets_path, kp_names=kp_names)
    pre.check_config()
    stac = Stac(base_path / cfg.model.MJCF_PATH, cfg, kp_names, setup=setup, device=device)
    pre.check_run(dist.world()[1])
    _check_ground_model(pre.ground, stac)
    series = _prepare_series(stac, cfg, kp_data, pre)
    if not cfg.stac.skip_fit_offsets:
        fit_offsets_path = _run_fit(stac, cfg, series, fit_offsets_path, pre.report, pre.fit_frames, pre.offset_mask, pre.min_observed)
    else:
        print("Skipping fit_offsets. To change this behavior, set cfg.stac.skip_fit_offsets to False.")
    if cfg.stac.skip_ik_only:
        print("Skipping IK-only phase. To change this behavior, set cfg.stac.skip_ik_only to False.")
        return fit_offsets_path, None
    return _run_ik(stac, series, fit_offsets_path, ik_only_path, pre, start)


def _run_fit(stac, cfg, series, fit_offsets_path, report, fit_frames="first", offset_mask="off", min_observed=1.0) -> Path:
    """``fit_offsets`` on ``n_fit_frames`` rows of the series -- the first ones, or with ``stac.fit_frames`` those of
    ``_select_fit_frames`` in ascending time order -- and the fit file -> the name the file really has.  With ``stac.offset_mask:
    observed`` the same rows of ``kp_gap == 0`` go along as the ``valid`` of the offset phase."""
    rows = info = None
    masked = offset_mask == "observed"
    if fit_frames == "first":
        kps = series.kp_data[: cfg.stac.n_fit_frames]
    else:
        rows, info = _select_fit_frames(stac, cfg, series, fit_frames, min_observed if masked else None)
        kps = series.kp_data[rows]
    print(f"Running fit. Mocap data shape: {kps.shape}")
    if masked:
        gap = np.asarray(series.marks["kp_gap"])  # (the pre-flight refused the mask without fill_missing)
        fit_data = stac.fit_offsets(kps, valid=(gap[: cfg.stac.n_fit_frames] if rows is None else gap[rows]) == 0)
    else:
        fit_data = stac.fit_offsets(kps)
    if rows is None:
        series.attach(fit_data, 0, fit_data.kp_data.shape[0])  # (the rows of the fit file are the first rows of the series, in order)
    else:
        series.attach_rows(fit_data, rows[: fit_data.kp_data.shape[0]])  # (fit_frames_per_clip drops a ragged tail)
    # multi-GPU: rank 0 holds the gathered result and writes it
    writes = dist.world()[0] == 0
    fit_offsets_path = _write_result(stac, cfg, fit_data, fit_offsets_path, report, writes)
    if rows is not None and writes:
        _write_frames(fit_offsets_path, rows, info)
    if masked and writes and stac.offset_counts is not None:  # (None: N_ITERS = 0, no offset phase ran)
        _write_offset_counts(fit_offsets_path, stac._kp_names, stac.offset_counts)
    print(f"saved fit to {fit_offsets_path}", flush=True)
    return fit_offsets_path


def min_observed_count(q: float, K: int) -> int:
    """``ceil(q K)``: how many of a frame's K keypoints ``stac.fit_frames_min_observed: q`` wants observed (the product is rounded
    to nine decimals first: 0.7 * 10 is 7, not the 7.000000000000001 of its float product)."""
    import math

    return int(math.ceil(round(float(q) * int(K), 9)))


def fit_frame_exclude(kp_gap, kp_swapped, q: float) -> np.ndarray:
    """The ``exclude`` [T] of ``Stac.select_frames`` under ``stac.offset_mask: observed``: a frame is a candidate iff at least
    ``ceil(q K)`` of its keypoints have ``kp_gap == 0`` and it carries no ``kp_swapped`` mark (None: the stage was off)."""
    gap = np.asarray(kp_gap)
    T, K = gap.shape
    exclude = np.count_nonzero(gap == 0, axis=1) < min_observed_count(q, K)
    if kp_swapped is not None:
        exclude |= (np.asarray(kp_swapped).reshape(T, -1) != 0).any(axis=1)
    return exclude


def _select_fit_frames(stac, cfg, series, mode, min_observed=None):
    """``stac.fit_frames: strided | diverse`` -> (the ``n_fit_frames`` chosen rows of the prepared series, ascending, and the ``info``
    of ``Stac.select_frames``).  Every rank computes the selection itself: same bits.  A frame that carries a mark of any
    preparation stage (``series.marks``) is no candidate: the offsets are calibrated on observed keypoints only.  ``min_observed``
    (``stac.fit_frames_min_observed`` under ``stac.offset_mask: observed``, else None): the candidates are those of
    ``fit_frame_exclude`` instead, since the masked offset phase leaves a frame's filled keypoints out itself."""
    n, T = int(cfg.stac.n_fit_frames), series.kp_data.shape[0]
    if min_observed is None:
        exclude = np.zeros(T, bool)
        for mark in series.marks.values():
            exclude |= (np.asarray(mark).reshape(T, -1) != 0).any(axis=1)
        why = "carry no mark of a preparation stage"
    else:
        K = series.kp_data.shape[1] // 3
        exclude = fit_frame_exclude(series.marks["kp_gap"], series.marks.get("kp_swapped"), min_observed)
        why = (f"have at least {min_observed_count(min_observed, K)} of their {K} keypoints observed (stac.fit_frames_min_observed = "
               f"{min_observed:g}) and no swap repaired")
    n_cand = int(T - np.count_nonzero(exclude))
    if n_cand < n:
        raise ValueError(f"stac.fit_frames = {mode}: n_fit_frames = {n}, but only {n_cand} of the {T} frames {why}")
    rows, info = stac.select_frames(series.kp_data, n, mode, exclude=exclude)
    if min_observed is not None:
        info["min_observed"] = float(min_observed)
    if info["n_selected"] < n:
        raise ValueError(f"stac.fit_frames = {mode}: n_fit_frames = {n}, but the selection stopped after {info['n_selected']} frames: "
                         "every other usable frame equals one of them (or has a coordinate that is not finite)")
    return rows, info


def frames_path(fit_offsets_path) -> Path:
    """``fit.h5`` -> ``fit.h5.frames.json`` (of the name the fit file really has: ``io.resolve_output_path``)."""
    p = io.resolve_output_path(fit_offsets_path)
    return p.with_name(p.name + ".frames.json")


def _write_frames(fit_offsets_path, rows, info) -> Path:
    """What ``stac.fit_frames`` chose, as JSON next to the fit file: the mode, the rows of the series that are the rows of the fit
    file (ascending), the same in selection order, and ``radius2`` (``diverse``; the first is infinite: written as null)."""
    import json

    path = frames_path(fit_offsets_path)
    r2 = [None if not np.isfinite(v) else float(v) for v in info["radius2"]]
    out = {"mode": info["mode"], "indices": [int(i) for i in rows], "order": [int(i) for i in info["order"]], "radius2": r2}
    if "min_observed" in info:  # (stac.offset_mask: observed -- the fit_frames_min_observed that chose the candidates)
        out["min_observed"] = float(info["min_observed"])
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(f"fit_frames: wrote {path}", flush=True)
    return path


def offset_counts_path(fit_offsets_path) -> Path:
    """``fit.h5`` -> ``fit.h5.offsets.json`` (of the name the fit file really has: ``io.resolve_output_path``)."""
    p = io.resolve_output_path(fit_offsets_path)
    return p.with_name(p.name + ".offsets.json")


def _write_offset_counts(fit_offsets_path, kp_names, counts) -> Path:
    """What ``stac.offset_mask: observed`` fitted the offsets to, as JSON next to the fit file: the keypoint names, per keypoint the
    number of sampled frames of the last calibration iteration that observed it, the number of sampled frames, and the keypoints
    that none observed (their offsets follow the regularisation, or stay as they were where there is none)."""
    import json

    path = offset_counts_path(fit_offsets_path)
    n = [int(v) for v in counts["n"]]
    path.write_text(json.dumps({"kp_names": list(kp_names), "n": n, "n_sampled": int(counts["n_sampled"]),
                                "never_observed": [str(kp_names[k]) for k, v in enumerate(n) if v == 0]}, indent=1) + "\n")
    print(f"offset_mask: wrote {path}", flush=True)
    return path


def _run_ik(stac, series, fit_offsets_path, ik_only_path, pre, start):
    """``ik_only`` on the whole series with the offsets of the fit file, the host post-processing and the result file(s) -> what
    ``run_stac`` returns."""
    kp_data = series.kp_data
    cfg = pre.cfg  # the caller's, until the fit file is read back
    if kp_data.shape[0] % cfg.stac.n_frames_per_clip != 0:
        raise ValueError(
            f"n_frames_per_clip ({cfg.stac.n_frames_per_clip}) must divide evenly with the total number of mocap "
            f"frames({kp_data.shape[0]})")
    print("Running ik_only()")
    # the config stored with the fit replaces the caller's from here on, as in the reference (main.py:111): it decides
    # continuous / n_frames_per_clip / infer_qvels below and is what the ik_only file records (the Stac object
    # itself keeps the caller's config, also as in the reference)
    cfg, fit_data = io.load_stac_data(fit_offsets_path)
    rank, world_size = dist.world()
    F = int(cfg.stac.n_frames_per_clip)
    n_clips = kp_data.shape[0] // F
    # where the results go: resolved here (an "auto" becomes rank0 / none by output size; a continuous run always gathers) and
    # handed to ik_only as an argument -- the caller's config object is not touched
    mode = _ik_output_mode(stac.cfg, kp_data.shape[0], stac, continuous=bool(cfg.stac.continuous)) if world_size > 1 else "rank0"
    sharded = world_size > 1 and mode == "none"
    if sharded and cfg.stac.continuous:  # (explicit gather = none with a fit file whose config turned out continuous)
        raise ValueError(GATHER_NONE_CONTINUOUS)
    if sharded and pre.resample is not None:  # (gather = auto that resolved to none by the size of the output)
        raise ValueError(RESAMPLE_SHARDED)
    post = {"continuous": bool(cfg.stac.continuous), "n_frames_per_clip": F, "infer_qvels": bool(cfg.stac.infer_qvels)} if pre.post_gpu else None
    if pre.smooth is not None:  # (postprocess = gpu: _smooth_mode)
        _check_smooth_clip(pre.smooth, _smooth_clip_len(cfg, kp_data.shape[0]))
        post["smooth"] = pre.smooth
    if seam_options(cfg.stac) != (pre.seam_passes, pre.seam_report):  # the ik_only file records what this run did at its clip borders
        from .config import validate_config

        stored = cfg.to_dict()
        stored["stac"].update({"seam_passes": pre.seam_passes, "seam_report": "on" if pre.seam_report else "off"})
        cfg = validate_config(stored)
    extra = {"post": post} if pre.post_gpu else {}
    if pre.seam_passes != 1:
        extra["passes"] = pre.seam_passes
    if pre.ground["mode"] == "level" and sharded:  # (gather = auto that resolved to none by the size of the output)
        raise ValueError(GROUND_LEVEL_SHARDED)
    ik_data = stac.ik_only(kp_data, fit_data.offsets, gather=mode, **extra)
    if rank != 0 and not sharded and mode != "all":
        dist.barrier()  # this rank holds its own shard only: rank 0 post-processes and writes the gathered result
        if pre.resample is not None:
            dist.barrier()  # ... and the resampled one
        return fit_offsets_path, io.resolve_output_path(ik_only_path)
    if cfg.stac.continuous and post is None:
        ik_data = utils.handle_edge_effects(ik_data, F)
    print(f"Final qpos shape: {ik_data.qpos.shape}")
    if post is None and cfg.stac.infer_qvels and ik_data.qpos.shape[0]:  # main.py:118-133: per clip of n_frames_per_clip frames
        batched = ik_data.qpos.reshape((-1, F, ik_data.qpos.shape[-1]))
        qvels = [utils.compute_velocity_from_kinematics(c, dt=stac._timestep, freejoint=stac._freejoint) for c in batched]
        ik_data.qvel = np.stack(qvels).reshape(-1, qvels[0].shape[-1])
    lo, hi = dist.shard_range(n_clips) if sharded else (0, n_clips)
    # (rows of the input series, not passed through the cross-fade; a shard file carries the rows of its clips)
    series.attach(ik_data, lo * F, hi * F)
    ground = None
    if pre.ground["mode"] != "off" and (sharded or rank == 0) and np.asarray(ik_data.xpos).shape[0]:
        ground = _ground_stage(stac, ik_data, pre.ground)  # (level: ik_data is levelled from here on; resample inherits it)
        cfg = _ground_config(cfg, pre.ground, ground)
    if sharded:
        # every rank writes ITS clips under a shard name (never a partial result under the full-run name; its report is of these
        # clips, shard reports are not merged); rank 0 adds the manifest that io.load_stac_result() reads the run back through
        shard = _write_result(stac, cfg, ik_data, io.shard_path(ik_only_path, rank, world_size), pre.report, True)
        if pre.seam_report:  # (of this rank's clips, like its report)
            _write_seams(stac, ik_data, shard, F)
        if ground is not None:
            _write_ground(shard, ground)
        manifest = io.manifest_path(ik_only_path)
        if rank == 0:
            io.write_manifest(manifest, ik_only_path, world_size, n_clips, F)
        dist.barrier()
        print(f"Saved ik_only shard {shard} (clips {lo}:{hi}); manifest {manifest}. "
              f"Finished in {(time.time() - start) / 60:.2f} minutes")
        return fit_offsets_path, manifest
    ik_only_path = _write_result(stac, cfg, ik_data, ik_only_path, pre.report, rank == 0)
    if pre.seam_report and rank == 0:
        _write_seams(stac, ik_data, ik_only_path, F)
    if ground is not None:
        _write_ground(ik_only_path, ground)
    if pre.resample is not None:
        _write_resampled(stac, cfg, ik_data, ik_only_path, pre, rank == 0)
    print(f"Saved ik_only to {ik_only_path}. Finished in {(time.time() - start) / 60:.2f} minutes")
    return fit_offsets_path, ik_only_path


def seams_path(ik_only_path) -> Path:
    """``ik_only.h5`` -> ``ik_only.h5.seams.json`` (of the name the result file really has: ``io.resolve_output_path``)."""
    p = io.resolve_output_path(ik_only_path)
    return p.with_name(p.name + ".seams.json")


def _write_seams(stac, ik_data, ik_only_path, clip_len) -> Path:
    """``stac.seam_report: on``: the summary of ``Stac.seam_steps`` of the packaged ik_only result (clips of ``clip_len`` rows: a
    continuous run is stitched by now) as JSON next to the result file, which does not change."""
    import json

    path = seams_path(ik_only_path)
    if np.asarray(ik_data.qpos).shape[0] == 0:  # (a rank of a sharded run that owns no clip)
        return path
    summary = stac.seam_steps(ik_data, clip_len=clip_len)["summary"]
    path.write_text(json.dumps(summary, indent=1) + "\n")
    print(f"seam_report: {summary['n_seams']} seams, mean / max step across a clip border {summary['seam_mean']} / {summary['seam_max']}; "
          f"wrote {path}", flush=True)
    return path


GROUND_LEVEL_SHARDED = ("stac.ground = level takes the floor from the whole ik_only result on rank 0, but this run writes per-rank shards "
                        "(stac.gather resolves to none): use gather = rank0, or stac.ground = report")
GROUND_LEVEL_FIXED_ROOT = ("stac.ground = level moves the model along z through a free root joint that the fit places (root optimisation), "
                           "which this model does not have: use stac.ground = report")


def ground_path(ik_only_path) -> Path:
    """``ik_only.h5`` -> ``ik_only.h5.ground.json`` (of the name the result file really has: ``io.resolve_output_path``)."""
    p = io.resolve_output_path(ik_only_path)
    return p.with_name(p.name + ".ground.json")


def _ground_mode(cfg) -> dict:
    """``stac.ground``: "off" (default) | "report" | "level" -> the options of ``config.ground_options``.  ``ValueError`` for a bad
    value of any of the seven keys.  What needs the model is for ``_check_ground_model``."""
    return ground_options(cfg.stac)


def check_ground_level(mode: str, setup):
    """``level`` shifts the pose along z through the free joint's translation: refused for a model without one, and for one whose
    root the fit leaves where the model has it (a tethered animal: no ``ROOT_OPTIMIZATION_KEYPOINT``)."""
    if mode == "level" and not (setup.freejoint and setup.do_root_opt):
        raise ValueError(GROUND_LEVEL_FIXED_ROOT)


def _check_ground_model(opt, stac):
    """What ``stac.ground`` asks of the model, once it is known and before any work: a free root for ``level``, and geom and body
    names (``ground_geoms``, ``ground_track``) that the model has."""
    if opt["mode"] == "off":
        return
    check_ground_level(opt["mode"], stac.setup)
    stac.ground_table(opt["geoms"], opt["geom_groups"], opt["track"])


def _ground_stage(stac, ik_data, opt) -> dict:
    """``stac.ground``: the summary of ``Stac.ground_clearance`` of the packaged ik_only result.  ``level``: ``floor_z`` of that
    summary is subtracted in float32 from ``qpos[:, 2]`` and from the z of ``xpos``, ``marker_sites`` and ``kp_data`` of ``ik_data``
    (in place), and ``summary["level"]`` says per geom how many frames it spends below the new floor: a second call on the unshifted
    arrays with ``z_ref = floor_z``."""
    args = dict(geoms=opt["geoms"], track=opt["track"], permille=opt["permille"], contact=opt["contact"])
    summary = stac.ground_clearance(ik_data, z_ref=opt["z_ref"], **args)["summary"]
    summary["mode"] = opt["mode"]
    if opt["mode"] != "level":
        return summary
    if summary["floor_z"] is None:
        raise ValueError("stac.ground = level: no frame of the result has a finite lowest z, so there is no floor to subtract")
    floor = np.float32(summary["floor_z"])
    again = stac.ground_clearance(ik_data, z_ref=float(floor), **args)["summary"]
    summary["level"] = {"floor_z": float(floor), "geoms": [{"name": g["name"], "frames_below": g["frames_below"]} for g in again["geoms"]],
                        "unfitted_below": again["unfitted_below"]}
    for name, index in (("qpos", (slice(None), 2)), ("xpos", (Ellipsis, 2)), ("marker_sites", (Ellipsis, 2)), ("kp_data", (slice(None), slice(2, None, 3)))):
        a = np.array(getattr(ik_data, name), dtype=np.float32)
        a[index] = a[index] - floor
        setattr(ik_data, name, a)
    return summary


def _ground_config(cfg, opt, summary):
    """The config that the ik_only file stores: the ``stac.ground*`` keys of this run and, for ``level``, the floor it subtracted."""
    from .config import validate_config

    stored = cfg.to_dict()
    stored["stac"].update({"ground": opt["mode"], "ground_geoms": opt["geoms"], "ground_track": list(opt["track"]), "ground_z": opt["z_ref"],
                           "ground_permille": opt["permille"], "ground_contact": opt["contact"]})
    if opt["geom_groups"] is not None:
        stored["stac"]["ground_geom_groups"] = list(opt["geom_groups"])
    if opt["mode"] == "level":
        stored["stac"]["ground_floor_z"] = summary["level"]["floor_z"]
    else:
        stored["stac"].pop("ground_floor_z", None)
    return validate_config(stored)


def _write_ground(ik_only_path, summary) -> Path:
    """The summary of ``_ground_stage`` as JSON next to the result file, and one line of it to the log."""
    import json

    path = ground_path(ik_only_path)
    path.write_text(json.dumps(summary, indent=1) + "\n")
    print(f"ground: floor_z {summary['floor_z']}, {len(summary['unfitted_below'])} geoms outside the fit below z = {summary['z_ref']:g} in most frames"
          + (f"; levelled by {summary['level']['floor_z']}" if "level" in summary else "") + f"; wrote {path}", flush=True)
    return path


def resampled_path(ik_only_path, to_hz) -> Path:
    """``ik_only.h5`` and 50 -> ``ik_only.50hz.h5`` (29.97 -> ``ik_only.29.97hz.h5``): where ``stac.resample`` writes its file."""
    p = Path(ik_only_path)
    return p.with_name(f"{p.stem}.{to_hz:g}hz{p.suffix}")


def _write_resampled(stac, cfg, ik_data, ik_only_path, pre, writes: bool) -> Path:
    """``stac.resample``: the packaged ik_only result at ``stac.resample_hz`` as a second file next to the first, through the writer
    of every result file (and with its own report under ``stac.report: on``).  The config stored in it is the first file's with the
    five keys of the caller's and, where the run is not continuous, ``n_frames_per_clip`` set to the rows of a resampled clip, so that
    ``fit_report`` and ``smooth_result`` of that file cut the right clips."""
    from . import post as gpost
    from .config import validate_config

    opt = pre.resample
    path = resampled_path(ik_only_path, opt["to_hz"])
    if writes:
        stored = cfg.to_dict()
        stored["stac"].update({"resample": opt["kind"], "mocap_hz": opt["from_hz"], "resample_hz": opt["to_hz"], "resample_lobes": opt["lobes"],
                               "resample_beta": opt["beta"], "postprocess": "gpu"})
        if "reference_marker_order" in stored["stac"]:  # (the caller's decides the rows of this run, and the pre-flight refused a true one)
            stored["stac"]["reference_marker_order"] = False
        if not cfg.stac.continuous:
            stored["stac"]["n_frames_per_clip"] = gpost.resample_rows(int(cfg.stac.n_frames_per_clip), opt["up"], opt["down"])
        stored = validate_config(stored)
        # (the clips are those of the config stored with the ik_only file; the Stac object keeps the caller's)
        data = stac.resample_result(ik_data, opt["from_hz"], opt["to_hz"], lobes=opt["lobes"], beta=opt["beta"], cfg=cfg)
    path = _write_result(stac, stored if writes else cfg, data if writes else None, path, pre.report, writes)
    print(f"resample: saved the ik_only result at {opt['to_hz']:g} Hz to {path}", flush=True)
    return path


class _Preflight:
    """What ``run_stac`` reads from the caller's config and refuses before any work is done.  Several refusals depend on the config
    stored with the fit (it decides the clip length and ``continuous`` of the ik_only run): ``fit_cfg`` is the caller's when this run
    writes the fit, else it is read from the fit file, once, and only if a refusal asks for it."""

    def __init__(self, cfg, n_frames: int, fit_offsets_path, kp_names=None):
        self.cfg, self.n_frames, self.fit_offsets_path = cfg, int(n_frames), fit_offsets_path
        self.kp_names = kp_names  # (None: a caller that checks a config without a run; stac.repair_swaps then names no candidates)
        self._fit_cfg = None

    @property
    def fit_cfg(self):
        if self._fit_cfg is None:
            self._fit_cfg = self.cfg if not self.cfg.stac.skip_fit_offsets else io.load_stac_data(self.fit_offsets_path)[0]
        return self._fit_cfg

    def check_config(self):
        """What needs no model (bad values, hampel without fill_missing, smoothing without postprocess = gpu or with
        reference_marker_order, ...): refused before a ``Stac`` is built."""
        stac = self.cfg.stac
        self.reject_mode, self.reject_args = _reject_outliers_mode(self.cfg)
        self.pairwise_mode, self.pairwise_args = _reject_pairwise_mode(self.cfg)
        self.swaps_pairs, self.swaps_args = _repair_swaps_mode(self.cfg, self.kp_names)
        self.donors_mode, self.donors_triples = _fill_donors_mode(self.cfg)
        self.report = _report_mode(self.cfg)
        self.smooth = _smooth_mode(self.cfg)
        self.resample = _resample_mode(self.cfg)
        self.fit_frames = fit_frames_options(stac)
        self.offset_mask, self.min_observed = _offset_mask_mode(self.cfg)
        self.seam_passes, self.seam_report = seam_options(stac)
        self.ground = _ground_mode(self.cfg)
        if self.fit_frames != "first" and not stac.skip_fit_offsets:  # (first keeps the reference's slice, which takes what there is)
            n = int(stac.n_fit_frames)
            if n > self.n_frames:
                raise ValueError(f"stac.fit_frames = {self.fit_frames}: n_fit_frames = {n} exceeds the {self.n_frames} frames of the recording")
            if n < 1:
                raise ValueError(f"stac.fit_frames = {self.fit_frames}: n_fit_frames must be at least 1, not {n}")
        if stac.skip_ik_only:  # (checked all the same; there is no ik_only file to resample)
            self.resample = None
        self.marker_order = not stac.skip_ik_only and bool(stac.get("reference_marker_order", False))
        if self.report[0] and self.marker_order:
            F = int(self.fit_cfg.stac.n_frames_per_clip)
            if F > 1 and self.n_frames // max(F, 1) > 1:
                raise ValueError("stac.report = on cannot pair marker_sites with kp_data in the reference's frame-major row order "
                                 "(stac.reference_marker_order: true with more than one clip of more than one frame): the rows of "
                                 "marker_sites are then not the rows of kp_data")
        if self.smooth is not None and not stac.skip_ik_only:  # stac.smooth: a clip must hold a whole window
            _check_smooth_clip(self.smooth, _smooth_clip_len(self.fit_cfg, self.n_frames))

    def check_run(self, world_size: int):
        """What today follows the construction of the ``Stac``, in that order."""
        stac = self.cfg.stac
        if not stac.skip_ik_only and world_size > 1 and str(stac.get("gather", "auto") or "auto") == "none":
            # an EXPLICIT gather = none cannot serve a continuous run (cross-fades reach across shard borders)
            if self.fit_cfg.stac.continuous:
                raise ValueError(GATHER_NONE_CONTINUOUS)
            if self.resample is not None:
                raise ValueError(RESAMPLE_SHARDED)
            if self.ground["mode"] == "level":
                raise ValueError(GROUND_LEVEL_SHARDED)
        # stac.postprocess (engine extension, read from the caller's config like gather): "host" (default) = the numpy functions
        # of utils.py; "gpu" = ik_only stitches and infers qvel on the device (post.py) and the two host steps are skipped
        self.post_gpu = _postprocess_mode(self.cfg) == "gpu"
        if self.post_gpu and self.marker_order and self.fit_cfg.stac.continuous:
            raise ValueError(POSTPROCESS_GPU_MARKER_ORDER)
        self.fill_mode = _fill_missing_mode(self.cfg)


@dataclass
class _Series:
    """What ``_prepare_series`` leaves: the prepared ``kp_data`` [T, 3K] and ``marks``, result-field name (``io.OPTIONAL_FIELDS``) ->
    [T, K] array whose row i is about row i of the series, of the fields that this run produced alone."""

    kp_data: np.ndarray
    marks: dict = field(default_factory=dict)

    def attach(self, data, lo: int, hi: int):
        """The rows ``lo:hi`` of every mark become the field of that name of ``data`` (a ``StacData`` of those rows of the series)."""
        for name, mark in self.marks.items():
            setattr(data, name, mark[lo:hi])

    def attach_rows(self, data, rows):
        """The index form: ``data`` holds the rows ``rows`` of the series, in that order."""
        for name, mark in self.marks.items():
            setattr(data, name, mark[rows])


def _prepare_series(stac, cfg, kp_data, pre) -> _Series:
    """``stac.repair_swaps`` (on the raw series), then ``stac.reject_pairwise`` (its medians are those of the repaired series), then
    ``stac.reject_outliers``, then ``stac.fill_donors`` (what it fills is no longer missing; ``kp_gap`` is then ITS gap, the gap of the
    series before anything was filled), then ``stac.fill_missing`` over the WHOLE series, once, on the GPU (every rank itself: same bits) -> the
    prepared series and its marks: kp_swapped (1 for both keypoints of a repaired pair), kp_rejected_pairwise (the pairwise detector's
    share), kp_rejected (what either detector rejected) and kp_gap, each only with its stage on.  A missing run that crosses
    n_fit_frames or a clip border is so filled from its true neighbours, and both phases see the filled array.  A rejected keypoint is
    three NaN, which the fill closes like any missing one, so kp_gap > 0 there with no further code (and the pre-flight refuses a
    rejecter without the fill, so kp_rejected never comes without kp_gap)."""
    kp_gap = kp_rejected = kp_pairwise = kp_hampel = kp_swapped = None
    if pre.swaps_pairs:
        kp_data, swap_flag = stac.repair_swaps(kp_data, pre.swaps_pairs, **pre.swaps_args)
        kp_swapped = np.zeros((kp_data.shape[0], kp_data.shape[1] // 3), np.uint8)
        for s, (a, b) in enumerate(pre.swaps_pairs):
            kp_swapped[:, a] = kp_swapped[:, b] = swap_flag[:, s]
        n_fit = min(int(cfg.stac.n_fit_frames), kp_swapped.shape[0])
        if not cfg.stac.skip_fit_offsets and n_fit > 0:
            print(f"repair_swaps: {int(np.count_nonzero(swap_flag[:n_fit]))} (frame, pair)s of the {n_fit} fit frames were exchanged back")
    if pre.pairwise_mode != "off":
        kp_data, kp_pairwise = stac.reject_pairwise(kp_data, **pre.pairwise_args)
        kp_rejected = kp_pairwise
    if pre.reject_mode != "off":
        kp_data, kp_hampel = stac.reject_outliers(kp_data, **pre.reject_args)
        # (Hampel passes a keypoint that is missing already: the two detectors' sets are disjoint)
        kp_rejected = kp_hampel if kp_pairwise is None else kp_hampel | kp_pairwise
    donor_gap = None
    if pre.donors_mode != "off":  # (the pre-flight refuses it without the fill)
        from . import prep

        # the pairwise statistics of a stage of this run if one has them (reject_pairwise's over repair_swaps'), else of this series
        don = prep.donor_table(stac.pair_stats, kp_data.shape[1] // 3, pre.donors_triples) if pre.pairwise_mode != "off" or pre.swaps_pairs else None
        kp_data, donor_gap, src = stac.fill_donors(kp_data, don, pre.donors_triples)
        n_fit = min(int(cfg.stac.n_fit_frames), src.shape[0])
        if not cfg.stac.skip_fit_offsets and n_fit > 0:
            share = lambda sel: 100.0 * np.count_nonzero(sel) / src[:n_fit].size  # noqa: E731
            ranks = ", ".join(f"triple {d + 1}: {share(src[:n_fit] == d + 1):.3f} %" for d in range(pre.donors_triples))
            print(f"fill_donors: of the keypoints of the {n_fit} fit frames, filled by {ranks}; left to fill_missing: {share(src[:n_fit] == 255):.3f} %")
    if pre.fill_mode != "off":
        kp_data, kp_gap = stac.fill_missing(kp_data, pre.fill_mode)
        if donor_gap is not None:  # kp_gap is the gap of the series before anything was filled: donor-filled values are filled values
            kp_gap = donor_gap
        n_fit = min(int(cfg.stac.n_fit_frames), kp_gap.shape[0])
        if not cfg.stac.skip_fit_offsets and n_fit > 0:  # (the offset phase fits filled positions like observed ones: DESIGN.md §10)
            print(f"fill_missing: {100.0 * np.count_nonzero(kp_gap[:n_fit]) / kp_gap[:n_fit].size:.3f} % of the keypoints of the "
                  f"{n_fit} fit frames are filled values")
            if kp_pairwise is not None:
                print(f"reject_pairwise: {100.0 * np.count_nonzero(kp_pairwise[:n_fit]) / kp_pairwise[:n_fit].size:.3f} % of the "
                      f"keypoints of the {n_fit} fit frames were rejected by their pairwise distances (and are among the filled ones)")
            if kp_hampel is not None:
                print(f"reject_outliers: {100.0 * np.count_nonzero(kp_hampel[:n_fit]) / kp_hampel[:n_fit].size:.3f} % of the "
                      f"keypoints of the {n_fit} fit frames were rejected as outliers (and are among the filled ones)")
    marks = {"kp_swapped": kp_swapped, "kp_rejected_pairwise": kp_pairwise, "kp_rejected": kp_rejected, "kp_gap": kp_gap}
    return _Series(kp_data, {name: mark for name, mark in marks.items() if mark is not None})


def _write_result(stac, cfg, data, path, report, writes: bool) -> Path:
    """The tail of a phase: the rank that ``writes`` adds the report (``stac.report: on``) and saves ``data``; every rank gets the
    name the file really has, once it is there."""
    on, permille, worst = report
    if writes:
        if on:
            _write_report(stac, data, path, permille, worst)
        io.save_data_to_h5(config=cfg, file_path=path, **data.as_dict())
    path = io.resolve_output_path(path)
    dist.barrier()
    return path


def report_path(result_path) -> Path:
    """``fit.h5`` -> ``fit.h5.report.json`` (of the name the result file really has: ``io.resolve_output_path``)."""
    p = io.resolve_output_path(result_path)
    return p.with_name(p.name + ".report.json")


def _report_mode(cfg) -> tuple:
    """``stac.report``: "off" (default) | "on" -> (on, permille values of ``stac.report_quantiles``, ``stac.report_worst``).
    ``ValueError`` for a bad value of any of the three keys."""
    return report_options(cfg.stac)


def _write_report(stac, data, result_path, permille, worst) -> Path:
    """The report of a phase's final ``StacData``, computed on the device, as JSON next to the result file that is about to be
    written, and two lines of it to the log."""
    import json

    from . import report

    summary = stac.fit_report(data, permille, worst)
    path = report_path(result_path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(summary, indent=1) + "\n")
    for line in report.overall_lines(summary):
        print(line)
    print(f"report: wrote {path}", flush=True)
    return path


def _smooth_mode(cfg):
    """``stac.smooth``: "off" (default) | "savgol" | "gaussian" -> None, or the options of ``config.smooth_options`` as the
    ``post["smooth"]`` of ``Stac.ik_only`` takes them.  ``ValueError`` for a bad value of any of the four keys, and for smoothing
    without ``postprocess: gpu`` or with ``reference_marker_order: true``."""
    opt = smooth_options(cfg.stac)
    return None if opt["kind"] == "off" else opt


def _resample_mode(cfg):
    """``stac.resample``: "off" (default) | "kaiser" -> None, or the options of ``config.resample_options``.  ``ValueError`` for a
    bad value of any of the five keys, a missing rate, a ratio or window that the kernel does not take, and for resampling without
    ``postprocess: gpu`` or with ``reference_marker_order: true``."""
    opt = resample_options(cfg.stac)
    return None if opt["kind"] == "off" else opt


def _smooth_clip_len(fit_cfg, n_frames: int) -> int:
    """Rows that ``stac.smooth`` treats as one clip: ``n_frames_per_clip`` of the config stored with the fit, or, for a continuous
    run, everything (the stitched rows of ``n_frames // n_frames_per_clip`` windows)."""
    F = int(fit_cfg.stac.n_frames_per_clip)
    if not fit_cfg.stac.continuous:
        return F
    n_clips, ov = n_frames // max(F, 1), utils.CONTINUOUS_BATCH_OVERLAP
    return 0 if n_clips == 0 else F + ov + max(n_clips - 2, 0) * F + max(F - ov, 0)


def _check_smooth_clip(smooth, clip_len: int):
    W = 2 * smooth["half_window"] + 1
    if clip_len < W:
        raise ValueError(f"stac.smooth = {smooth['kind']} with smooth_window = {smooth['half_window']} needs clips of at least {W} "
                         f"frames (the window), but a clip of this run has {clip_len}")


def _postprocess_mode(cfg) -> str:
    """``stac.postprocess``: "host" (default) | "gpu"."""
    return postprocess_options(cfg.stac)


def _fill_missing_mode(cfg) -> str:
    """``stac.fill_missing``: "off" (default) | "linear" | "hold"."""
    return fill_missing_options(cfg.stac)


def _reject_outliers_mode(cfg) -> tuple:
    """``stac.reject_outliers``: "off" (default) | "hampel" -> (mode, keyword arguments of ``Stac.reject_outliers`` from
    ``stac.outlier_window`` / ``outlier_nsigma`` / ``outlier_min_dev``).  ``ValueError`` for a bad value of any of the four keys,
    and for ``hampel`` with ``fill_missing`` off: the solver cannot take the NaN of a rejected keypoint."""
    mode, h, n_sigma, min_dev = outlier_options(cfg.stac)
    if mode != "off" and _fill_missing_mode(cfg) == "off":
        raise ValueError("stac.reject_outliers = hampel turns outliers into missing keypoints (NaN), which the solver cannot take: "
                         "set stac.fill_missing to linear or hold as well")
    return mode, {"half_window": h, "n_sigma": n_sigma, "min_dev": min_dev}


def _reject_pairwise_mode(cfg) -> tuple:
    """``stac.reject_pairwise``: "off" (default) | "mad" -> (mode, keyword arguments of ``Stac.reject_pairwise`` from
    ``stac.pairwise_nsigma`` / ``pairwise_min_dev`` / ``pairwise_votes``).  ``ValueError`` for a bad value of any of the four keys,
    and for ``mad`` with ``fill_missing`` off: the solver cannot take the NaN of a rejected keypoint."""
    mode, n_sigma, min_dev, votes = pairwise_options(cfg.stac)
    if mode != "off" and _fill_missing_mode(cfg) == "off":
        raise ValueError(PAIRWISE_NEEDS_FILL)
    return mode, {"n_sigma": n_sigma, "min_dev": min_dev, "votes": votes}


def _fill_donors_mode(cfg) -> tuple:
    """``stac.fill_donors``: "off" (default) | "auto" -> (mode, ``stac.fill_donors_triples``).  ``ValueError`` for a bad value of
    either key, and for ``auto`` with ``fill_missing`` off: what no donor triple can fill stays NaN, which the solver cannot take."""
    mode, n_triples = donor_options(cfg.stac)
    if mode != "off" and _fill_missing_mode(cfg) == "off":
        raise ValueError(DONORS_NEED_FILL)
    return mode, n_triples


def _offset_mask_mode(cfg) -> tuple:
    """``stac.offset_mask``: "off" (default) | "observed" -> (mode, ``stac.fit_frames_min_observed``).  ``ValueError`` for a bad value
    of either key, for a ``fit_frames_min_observed`` other than 1.0 with the mask off, and for ``observed`` with ``fill_missing`` off:
    ``kp_gap``, the mark of that stage, is what says which values are observations."""
    mode, q = offset_mask_options(cfg.stac)
    if mode != "off" and _fill_missing_mode(cfg) == "off":
        raise ValueError(OFFSET_MASK_NEEDS_FILL)
    return mode, q


def _repair_swaps_mode(cfg, kp_names=None) -> tuple:
    """``stac.repair_swaps``: off (default) | lr | [[nameA, nameB], ...] -> (the candidates as index pairs into ``kp_names``, [] for
    off, keyword arguments of ``Stac.repair_swaps`` from ``stac.swaps_nsigma`` / ``swaps_min_dev`` / ``swaps_min_bad``).
    ``ValueError`` for a bad value of any of the four keys, for names that ``kp_names`` does not hold, for a keypoint in two pairs
    and for ``lr`` without a left / right pair among the names.  Without ``kp_names`` only the values are checked."""
    mode, n_sigma, min_dev, min_bad = swaps_options(cfg.stac)
    pairs = swaps_candidates(mode, kp_names) if kp_names is not None else []
    return pairs, {"n_sigma": n_sigma, "min_dev": min_dev, "min_bad": min_bad}


GATHER_AUTO_MAX_BYTES = 1 << 30  # above this much output a multi-GPU run keeps per-rank shard files ("auto")


def _ik_output_mode(cfg, n_frames: int, stac, continuous: bool = False) -> str:
    """``stac.gather`` for the ik_only outputs: "rank0" | "all" | "none" | "auto" (default).  "auto" gathers to rank 0
    while the packed outputs (qpos, xpos, xquat, marker_sites, kp_data; 2 728 B per rodent frame) stay below
    ``stac.gather_max_bytes`` (default 1 GiB) and writes per-rank shards above: a 1 M-frame run is 2.7 GB that a
    padded gather would stage on rank 0's GPU for nothing.  A continuous run (cross-fades across clip borders, done on the
    gathered result) always gathers under "auto", whatever its size."""
    mode = str(cfg.stac.get("gather", "auto") or "auto")
    if mode != "auto":
        return mode
    if continuous:
        return "rank0"
    t = stac.setup.tables
    per_frame = 4 * (t.nq + 7 * t.nbody + 6 * t.nsite)
    limit = int(cfg.stac.get("gather_max_bytes", GATHER_AUTO_MAX_BYTES) or GATHER_AUTO_MAX_BYTES)
    return "rank0" if n_frames * per_frame <= limit else "none"
