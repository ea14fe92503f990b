"""``Stac``: model set-up, ``fit_offsets`` / ``ik_only`` and output packing on the HIP engine.

Mirrors ``stac_mjx/stac.py`` (:91-658; ``render`` draws with the GPU ray caster of ``render.py``).  The
per-frame Python loops of the reference (``compute_stac.pose_optimization``) run inside one
``stac_q_phase`` kernel launch per phase; sequencing, warm starts, sampling and packing follow the
reference.
"""

from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from . import dist, prng, utils
from .config import (GATHER_NONE_CONTINUOUS, INT32_MAX, POSTPROCESS_GPU_MARKER_ORDER, SEAM_MAX_PASSES, checked_int, report_options, seam_options,
                     smooth_marker_order_refusal)
from .engine import Engine
from .fit_model import FitSetup, build_fit_setup
from .io import StacData
from .stac_core import ModelHandle, StacCore


class Stac:
    """Skeletal registration on one GPU (or one rank of a multi-GPU job)."""

    def __init__(self, xml_path, cfg, kp_names, *, setup: FitSetup | None = None, device=None, verbose: bool = True):
        self.cfg = cfg
        self._kp_names = list(kp_names)
        self._xml_path = Path(xml_path) if xml_path is not None else None
        self.verbose = verbose
        self.setup = setup if setup is not None else build_fit_setup(self._xml_path, cfg.model, self._kp_names)
        s = self.setup
        self._lb, self._ub, self._part_names = s.lb, s.ub, s.part_names
        self._indiv_parts = s.part_masks
        self._trunk_kps = s.trunk_kps
        self._root_kp_idx = s.root_kp_idx
        self._is_regularized = s.is_regularized
        self._body_names = s.tables.body_names
        self._freejoint, self._slidejoint, self._fixed = s.freejoint, s.slidejoint, s.fixed_root
        stac_cfg = cfg.stac
        # `stac.solver` is an engine extension of the config surface: "pg" (default) = the reference's projected
        # gradient, reproduced exactly; "lm" = optional Levenberg-Marquardt solver (faster, fits the markers at
        # least as well, but does not reproduce the reference's truncated iterates).
        self.engine = Engine(s.tables, s.lb, s.ub, tol=float(cfg.model.FTOL), maxiter=int(cfg.model.N_ITER_Q),
                             lanes_per_chain=int(stac_cfg.get("lanes_per_chain", 0) or 0), device=device,
                             solver=str(stac_cfg.get("solver", "pg") or "pg"),
                             lm_maxiter=int(stac_cfg.get("lm_maxiter", 20) or 20))
        self.stac_core_obj = StacCore(self.engine, float(cfg.model.FTOL), int(cfg.model.N_ITER_Q))
        self._offsets = torch.as_tensor(s.tables.site_pos.copy())
        self.timings = None  # bench.py --mode run: {} collects the phase times of ik_only (see _tick)
        self._t_last = 0.0
        self._timestep = s.tables.timestep
        self._renderer = None
        self.pair_stats = None  # the pairwise statistics of the last reject_pairwise / repair_swaps call (device tensors)
        self.offset_counts = None  # fit_offsets(valid=...): the observed counts of the last calibration iteration

    # -- helpers ------------------------------------------------------------------------------------
    def _log(self, *a):
        if self.verbose:
            print(*a, flush=True)

    def _model_handle(self):
        return ModelHandle(engine=self.engine, nq=self.setup.tables.nq, jnt_type=self.setup.tables.jnt_type,
                           site_pos=self.engine.get_site_pos())

    def _get_error_stats(self, errors):
        e = np.asarray(errors).reshape(-1)
        if e.size == 0:  # a rank of a sharded run that owns no clip
            return e, 0.0, 0.0
        return e, float(np.mean(e)), float(np.std(e))

    def _q_phase(self, kp, *, do_root_opt, q_init=None, want_outputs=True, out=None):
        s = self.setup
        return self.engine.q_phase(
            kp, part_masks=s.part_masks, trunk_kps=s.trunk_kps, root_kp_idx=max(s.root_kp_idx, 0),
            root_dims=s.root_dims, do_root_opt=do_root_opt, q_init=q_init, want_bodies=want_outputs,
            want_markers=want_outputs, out=out)

    def _series_to_device(self, kp_data, what):
        """The whole series ``kp_data`` [T, 3K] as a float32 tensor on the engine's device."""
        kp = np.asarray(kp_data, dtype=np.float32)
        if kp.ndim != 2 or kp.shape[1] != 3 * len(self._kp_names):
            raise ValueError(f"{what}: kp_data must be [frames, {3 * len(self._kp_names)}], got {kp.shape}")
        if not kp.flags.writeable:  # (torch does not wrap a read-only array)
            kp = kp.copy()
        return torch.as_tensor(kp).to(self.engine.device)

    def _log_flagged(self, out, flag, head, names, verb):
        """The tail of a preparation stage: one log line per column of ``flag`` [T, columns] that is not all zero
        ("<head>: <names[column]>: n of T frames <verb> (share)"), then ``(out, flag)`` as numpy arrays."""
        T = flag.shape[0]
        count = flag.sum(dim=0, dtype=torch.int64).cpu().numpy()
        for c in np.flatnonzero(count):
            self._log(f"{head}: {names[c]}: {int(count[c])} of {T} frames {verb} ({100.0 * int(count[c]) / T:.3f} %)")
        return out.cpu().numpy(), flag.cpu().numpy()

    # -- fill_missing (engine extension; DESIGN.md "Filling missing keypoints") ----------------------------------------
    def fill_missing(self, kp_data, mode=None):
        """Fills the missing keypoints (a NaN or infinite coordinate) of the whole series ``kp_data`` [T, 3K] along time on the
        GPU (``prep.fill_missing``) -> ``(filled [T, 3K] float32, gap [T, K] int32)`` as numpy arrays; ``gap`` is 0 where the
        keypoint was observed, else the length of the missing run.  ``mode``: "linear" | "hold" (None: ``stac.fill_missing`` of
        the config).  One log line per keypoint that had gaps.  A keypoint without a single valid frame cannot be filled: a
        ``ValueError`` that names every such keypoint."""
        from . import prep

        mode = str(self.cfg.stac.get("fill_missing", "off") or "off") if mode is None else mode
        prep.mode_code(mode)
        kp = self._series_to_device(kp_data, "fill_missing")
        filled, gap = prep.fill_missing(kp, mode)
        info = prep.summary(gap)
        if info["empty"]:
            raise ValueError("fill_missing: no valid frame at all for keypoint(s) "
                             + ", ".join(f"{self._kp_names[k]} (index {k})" for k in info["empty"]) + ": nothing to fill them from")
        for k in np.flatnonzero(info["missing"]):
            self._log(f"fill_missing ({mode}): {self._kp_names[k]}: {int(info['missing'][k])} of {kp.shape[0]} frames filled, "
                      f"longest run {int(info['longest'][k])}")
        return filled.cpu().numpy(), gap.cpu().numpy()

    # -- reject_outliers (engine extension; DESIGN.md "Rejecting keypoint outliers") ------------------------------------
    def reject_outliers(self, kp_data, half_window=5, n_sigma=3.0, min_dev=0.001):
        """The Hampel identifier over the whole series ``kp_data`` [T, 3K] on the GPU (``prep.reject_outliers``) ->
        ``(out [T, 3K] float32, flag [T, K] uint8)`` as numpy arrays: a keypoint with a coordinate further than
        ``n_sigma * 1.4826`` median absolute deviations, and than ``min_dev``, from the median of the frames
        ``t - half_window .. t + half_window`` of its track is three NaN in ``out`` and 1 in ``flag``; everything else is the
        input bit for bit.  One log line per keypoint that had rejections: the count and the share."""
        from . import prep

        prep.outlier_params(half_window, n_sigma, min_dev)
        kp = self._series_to_device(kp_data, "reject_outliers")
        out, flag = prep.reject_outliers(kp, half_window, n_sigma, min_dev)
        return self._log_flagged(out, flag, f"reject_outliers (hampel, window {half_window}, {n_sigma} sigma)", self._kp_names, "rejected")

    # -- reject_pairwise (engine extension; DESIGN.md "Rejecting keypoints by pairwise distances") -----------------------
    def reject_pairwise(self, kp_data, n_sigma=6.0, min_dev=0.002, votes=2):
        """The pairwise-distance detector over the whole series ``kp_data`` [T, 3K] on the GPU (``prep.reject_pairwise``) ->
        ``(out [T, 3K] float32, flag [T, K] uint8)`` as numpy arrays: a keypoint that is in at least ``votes`` pairs whose
        distance lies further than ``n_sigma * 1.4826`` median absolute deviations, and than ``min_dev``, from that pair's median
        over the series is three NaN in ``out`` and 1 in ``flag``; everything else is the input bit for bit.  No time window:
        the length of a run of wrong values does not matter.  One log line per keypoint that had rejections."""
        from . import prep

        prep.pairwise_params(n_sigma, min_dev, votes)
        kp = self._series_to_device(kp_data, "reject_pairwise")
        out, flag, self.pair_stats = prep.reject_pairwise(kp, n_sigma, min_dev, votes)  # (kept for fill_donors: device tensors)
        return self._log_flagged(out, flag, f"reject_pairwise (mad, {n_sigma} sigma, {votes} votes)", self._kp_names, "rejected")

    # -- repair_swaps (engine extension; DESIGN.md "Repairing keypoint swaps") -------------------------------------------
    def repair_swaps(self, kp_data, pairs=None, n_sigma=6.0, min_dev=0.002, min_bad=3):
        """Exchanges back keypoints that carry each other's label, over the whole series ``kp_data`` [T, 3K] on the GPU
        (``prep.repair_swaps``) -> ``(out [T, 3K] float32, flag [T, S] uint8)`` as numpy arrays: ``flag[t, s]`` is 1 where the two
        keypoints of candidate ``s`` were exchanged in frame ``t``; everything else is the input bit for bit and no NaN is made.
        ``pairs``: the candidates as pairs of keypoint indices or names (None: the left / right pairs that ``config.lr_pairs``
        finds in the keypoint names).  One log line per candidate that had swaps."""
        from . import prep
        from .config import lr_pairs, named_pairs

        prep.swaps_params(n_sigma, min_dev, min_bad)
        names = list(self._kp_names)
        if pairs is None:
            cand = lr_pairs(names)
        elif all(isinstance(v, str) for p in pairs for v in p):
            cand = named_pairs(pairs, names)
        else:
            cand = pairs
        cand = prep.swaps_pairs(cand, len(names))
        kp = self._series_to_device(kp_data, "repair_swaps")
        out, flag, self.pair_stats = prep.repair_swaps(kp, cand, n_sigma, min_dev, min_bad)  # (kept for fill_donors: device tensors)
        return self._log_flagged(out, flag, f"repair_swaps ({n_sigma} sigma, min_bad {min_bad})", [f"{names[a]} / {names[b]}" for a, b in cand],
                                 "exchanged")

    # -- fill_donors (engine extension; DESIGN.md "Filling gaps from donor keypoints") -------------------------------------
    def fill_donors(self, kp_data, don=None, n_triples=4):
        """Fills the missing keypoints of the whole series ``kp_data`` [T, 3K] from the local frame of three other keypoints that
        are still tracked, on the GPU (``prep.fill_donors``) -> ``(out [T, 3K] float32, gap [T, K] int32, src [T, K] uint8)`` as
        numpy arrays: ``gap`` is ``fill_missing``'s of the input, ``src`` is 0 where the keypoint was observed, d + 1 where donor
        triple d filled it and 255 where it stays missing (for ``fill_missing`` to close).  ``don``: the donor table [K, D, 3]
        (None: ``prep.donor_table`` with ``n_triples`` rows from the pairwise statistics of this series, by one
        ``prep.reject_pairwise`` call that rejects nothing).  One log line per keypoint that had donor fills."""
        from . import prep

        kp = self._series_to_device(kp_data, "fill_donors")
        if don is None:
            prep.donor_triples(n_triples)
            # (votes that no frame can reach: a keypoint is in at most K - 1 pairs)
            don = prep.donor_table(prep.reject_pairwise(kp, votes=INT32_MAX)[2], len(self._kp_names), n_triples) if kp.shape[0] else \
                np.full((len(self._kp_names), n_triples, 3), -1, np.int32)
        out, gap, src = prep.fill_donors(kp, don)
        out, _ = self._log_flagged(out, ((src > 0) & (src < 255)).to(torch.uint8), "fill_donors", self._kp_names, "filled from donors")
        return out, gap.cpu().numpy(), src.cpu().numpy()

    # -- select_frames (engine extension; DESIGN.md "Choosing calibration frames") ---------------------------------------
    def select_frames(self, kp_data, n, mode="diverse", exclude=None):
        """``n`` calibration frames of the whole series ``kp_data`` [T, 3K] -> ``(indices [n_selected] int64 ascending, info)``.
        ``mode``: "first" (the first ``n`` candidates), "strided" (``select.select_strided``: even steps through the candidates,
        on the host) or "diverse" (``select.select_diverse``: greedy farthest-point selection over the frames' pairwise keypoint
        distances, on the GPU).  ``exclude`` ([T], truthy = not a candidate; None: every frame is one).  ``info``: ``mode``,
        ``order`` (the indices in selection order), ``radius2`` (float32, ``diverse`` only: the squared descriptor distance of every
        pick to the picks before it, else empty) and ``n_selected`` (below ``n`` only where ``diverse`` stopped early).  Logs the
        covering radius and how the picks spread over the ten tenths of the recording."""
        from . import select

        if mode not in select.MODES:
            raise ValueError(f"select_frames: mode must be first, strided or diverse, not {mode!r}")
        kp = np.asarray(kp_data)
        if kp.ndim != 2 or kp.shape[1] != 3 * len(self._kp_names):
            raise ValueError(f"select_frames: kp_data must be [frames, {3 * len(self._kp_names)}], got {kp.shape}")
        T = int(kp.shape[0])
        n = checked_int(n, "select_frames: n", ValueError, 1)
        cand = None
        if exclude is not None:
            ex = np.asarray(exclude)
            if ex.shape != (T,):
                raise ValueError(f"select_frames: exclude must be [{T}], one entry per frame, got {ex.shape}")
            cand = ex == 0
        radius2 = np.zeros(0, np.float32)
        if mode == "diverse":
            sel, r2, n_sel = select.select_diverse(self._series_to_device(kp, "select_frames"), n, cand)
            order, radius2 = sel.cpu().numpy()[:n_sel], r2.cpu().numpy()[:n_sel]
        elif mode == "strided":
            order = select.select_strided(T, n, cand)
        else:
            frames = np.arange(T, dtype=np.int64) if cand is None else np.flatnonzero(cand).astype(np.int64)
            if frames.size < n:
                raise ValueError(f"select_frames: {n} frames wanted, but only {frames.size} of the {T} frames are candidates")
            order = frames[:n]
        order = np.asarray(order, dtype=np.int64)
        tenths = np.bincount(np.minimum(order * 10 // max(T, 1), 9), minlength=10) if order.size else np.zeros(10, np.int64)
        cover = f", covering radius {float(np.sqrt(radius2[-1])):.6g} (descriptor units)" if radius2.size > 1 else ""
        self._log(f"select_frames ({mode}): {order.size} of {T} frames{cover}; picks per tenth of the recording: "
                  + " ".join(str(int(c)) for c in tenths))
        return np.sort(order), {"mode": mode, "order": order, "radius2": radius2, "n_selected": int(order.size)}

    # -- fit_report (engine extension; DESIGN.md "Fit report") -----------------------------------------------------------
    def fit_report(self, data, permille=None, worst=None) -> dict:
        """The marker error of a result, on the GPU (``report.fit_errors``), as the summary of ``report.summarize``: per keypoint
        the number of observed frames, the rms, the quantiles and the maximum of the distance between the fitted marker and the
        keypoint, over all keypoints the same, and the frames of largest summed squared error.  ``data``: a ``StacData`` or the
        path of a result file (a ``*.manifest.json`` reads a sharded run); its ``kp_gap``, when it has one, keeps filled
        keypoints out of every statistic.  ``permille`` / ``worst``: None = ``stac.report_quantiles`` / ``stac.report_worst``
        of the config.  One log line per keypoint."""
        from . import io, report

        _, cfg_perm, cfg_worst = report_options(self.cfg.stac)
        permille = report.check_permille(cfg_perm if permille is None else permille)
        worst = cfg_worst if worst is None else worst
        if not isinstance(data, StacData):
            data = io.load_stac_result(data)[1]
        markers = np.asarray(data.marker_sites, dtype=np.float32)
        kp = np.asarray(data.kp_data, dtype=np.float32)
        if markers.ndim != 3 or markers.shape[2] != 3 or kp.ndim != 2 or kp.shape != (markers.shape[0], 3 * markers.shape[1]):
            raise ValueError(f"fit_report: marker_sites {markers.shape} and kp_data {kp.shape} are not [frames, K, 3] and [frames, 3K]")
        gap = np.asarray(data.kp_gap)
        dev = self.engine.device
        to_dev = lambda a: torch.as_tensor(np.array(a)).to(dev)  # noqa: E731  (a copy: torch does not wrap a read-only array)
        res = report.fit_errors(to_dev(markers), to_dev(kp), to_dev(gap.astype(np.int32)) if gap.size else None, permille)
        summary = report.summarize(res, list(data.kp_names), worst=worst, permille=permille)
        for line in report.table_lines(summary):
            self._log(line)
        return summary

    # -- smooth_result (engine extension; DESIGN.md "Smoothing fitted poses") ----------------------------------------------
    def smooth_result(self, data, kind, half_window=3, order=None, sigma=None) -> StacData:
        """Smooths a stored ``ik_only`` result again without refitting, on the GPU (``post.smooth``): the counterpart of
        ``fit_report(path)``.  ``data``: the path of a result file (a ``*.manifest.json`` reads a sharded run), whose stored config
        decides the clips -- a continuous run is one clip, else clips of its ``n_frames_per_clip`` rows -- or a ``StacData``, with
        this object's config.  It starts from ``qpos_raw`` when the result has one, else from ``qpos``, and returns a ``StacData``
        whose ``qpos_raw`` is that start, whose ``qpos`` is its smoothed version (``kind`` / ``half_window`` / ``order`` /
        ``sigma`` as ``stac.smooth`` and its keys), whose ``xpos`` / ``xquat`` / ``marker_sites`` are the kinematics of that
        under the stored ``offsets`` and whose ``qvel`` is inferred again when the result had one; every other field passes.
        The engine's offsets are left as they were."""
        from . import io
        from . import post as gpost

        taps = gpost.smooth_taps(kind, half_window, order=order, sigma=sigma)
        cfg = self.cfg
        if not isinstance(data, StacData):
            cfg, data = io.load_stac_result(data)
        raw = np.asarray(data.qpos_raw if np.asarray(data.qpos_raw).size else data.qpos, dtype=np.float32)
        nq, K = self.setup.tables.nq, self.setup.tables.nsite
        if raw.ndim != 2 or raw.shape[1] != nq:
            raise ValueError(f"smooth_result: qpos must be [frames, {nq}], got {raw.shape}")
        F = int(cfg.stac.n_frames_per_clip)
        clip_len = raw.shape[0] if bool(cfg.stac.continuous) else F
        if clip_len < taps.shape[0]:
            raise ValueError(f"smooth_result: clips of {clip_len} frames are shorter than the window of {taps.shape[0]} frames")
        eng = self.engine
        keep = eng.get_site_pos()
        eng.set_site_pos(torch.as_tensor(np.array(data.offsets, dtype=np.float32)).reshape(K, 3))
        try:
            out = self._smooth_gpu(torch.as_tensor(np.array(raw)).to(eng.device), clip_len, taps)
            if np.asarray(data.qvel).size:
                out["qvel"] = gpost.infer_qvel(out["qpos"], F, self._timestep, self._freejoint)
            host = {k: v.cpu().numpy() for k, v in out.items()}
        finally:
            eng.set_site_pos(keep)
        from dataclasses import replace

        return replace(data, qpos_raw=raw, **host)

    # -- resample_result (engine extension; DESIGN.md "Resampling fitted poses") ---------------------------------------------
    def resample_result(self, data, from_hz, to_hz, lobes=10, beta=5.0, *, cfg=None) -> StacData:
        """A stored ``ik_only`` result at another frame rate, on the GPU (``post.resample``): the sibling of ``smooth_result``.
        ``data``: the path of a result file (a ``*.manifest.json`` reads a sharded run), whose stored config decides the clips -- a
        continuous run is one clip, else clips of its ``n_frames_per_clip`` rows -- or a ``StacData``, with ``cfg`` (None: this
        object's config).  Every clip of L rows becomes one of ``post.resample_rows(L, U, D)`` rows (U / D = ``to_hz / from_hz``): ``qpos`` is
        resampled with this model's quaternion columns and the engine's bounds, ``kp_data`` with the same filter as plain columns;
        ``xpos`` / ``xquat`` / ``marker_sites`` are the kinematics of the new ``qpos`` under the stored ``offsets``; ``qvel`` is
        inferred again when the result had one, with the real step ``1 / to_hz`` (the source file's was the model's ``timestep``);
        every per-frame mark (``kp_gap``, ``kp_rejected``, ...) is that of the nearest input row
        (``post.resample_source_rows``); ``qpos_raw`` is empty, its rows no longer correspond.  A NaN spreads over the outputs
        whose window holds it, and the first and last row of a clip are held beyond its ends, not extrapolated.
        The engine's offsets are left as they were."""
        from dataclasses import replace

        from . import io
        from . import post as gpost

        U, D = gpost.resample_ratio(from_hz, to_hz)
        taps = gpost.resample_taps(U, D, lobes=lobes, beta=beta)
        cfg = self.cfg if cfg is None else cfg
        if not isinstance(data, StacData):
            cfg, data = io.load_stac_result(data)
        qpos = np.asarray(data.qpos, dtype=np.float32)
        kp = np.asarray(data.kp_data, dtype=np.float32)
        nq, K = self.setup.tables.nq, self.setup.tables.nsite
        if qpos.ndim != 2 or qpos.shape[1] != nq:
            raise ValueError(f"resample_result: qpos must be [frames, {nq}], got {qpos.shape}")
        N = qpos.shape[0]
        if kp.ndim != 2 or kp.shape[0] != N:
            raise ValueError(f"resample_result: kp_data {kp.shape} does not have the {N} rows of qpos")
        L = N if bool(cfg.stac.continuous) else int(cfg.stac.n_frames_per_clip)
        if N == 0 or L < 1 or N % L != 0:
            raise ValueError(f"resample_result: cannot cut {N} rows into clips of {L} frames")
        Lo = gpost.resample_rows(L, U, D)
        eng = self.engine
        to_dev = lambda a: torch.as_tensor(np.array(a)).to(eng.device)  # noqa: E731  (a copy: torch does not wrap a read-only array)
        keep = eng.get_site_pos()
        eng.set_site_pos(torch.as_tensor(np.array(data.offsets, dtype=np.float32)).reshape(K, 3))
        try:
            taps_dev = to_dev(taps)
            q = gpost.resample(to_dev(qpos), L, U, D, taps_dev, self._quat_cols(), lb=eng.lb, ub=eng.ub)
            fk = eng.fk(q, want=("xpos", "xquat", "site_xpos"))
            out = {"qpos": q, "xpos": fk["xpos"], "xquat": fk["xquat"], "marker_sites": fk["site_xpos"],
                   "kp_data": gpost.resample(to_dev(kp), L, U, D, taps_dev)}
            if np.asarray(data.qvel).size:
                out["qvel"] = gpost.infer_qvel(q, Lo, 1.0 / float(to_hz), self._freejoint)
            host = {k: v.cpu().numpy() for k, v in out.items()}
        finally:
            eng.set_site_pos(keep)
        src = (np.arange(N // L, dtype=np.int64)[:, None] * L + gpost.resample_source_rows(L, U, D)[None, :]).reshape(-1)
        for name, _ in io.OPTIONAL_FIELDS:
            mark = np.asarray(getattr(data, name))
            if name != "qpos_raw" and mark.size:
                host[name] = mark[src]
        self._log(f"resample_result: {from_hz} -> {to_hz} Hz ({U} / {D}, {taps.shape[1]} taps): {N // L} clip(s) of {L} rows -> {Lo} rows each")
        return replace(data, qpos_raw=np.array([]), **host)

    # -- fit_offsets (stac.py:253-354) ------------------------------------------------------------------
    def fit_offsets(self, kp_data, time_indices=None, valid=None) -> StacData:
        """Alternate pose and offset optimisation.

        Default (the reference, ``stac.py:298-341``): ONE warm-started chain over all frames, carried across the
        calibration iterations -- a serial computation, run on this rank's GPU (replicas only).

        ``stac.fit_frames_per_clip: F`` (engine extension, not the reference's sequencing): the fit frames are cut
        into clips of F frames; every clip is its own chain (root-optimised in the first pass, carried across the
        iterations), the clips are sharded over the ranks and the offset phase all-reduces its 3K + 2 partial sums.

        ``time_indices`` (optional) overrides the PRNGKey(0) frame sample of the offset phase.

        ``valid`` (optional, bool [T, K]; engine extension, DESIGN.md "Offsets from observed keypoints"): which keypoint values
        are observations.  The offset phase of every calibration iteration then sums over the observed keypoints of the sampled
        rows only (``Engine.m_partial_masked`` / ``m_finish_masked``; under ``fit_frames_per_clip`` the all-reduce carries their
        4K + 2 partial sums), logs the keypoints that no sampled row observed, and leaves the counts of the last iteration in
        ``self.offset_counts`` (``n`` [K] and ``n_sampled``).  The pose phase sees ``kp_data`` as it is, filled values included.
        """
        cfgm = self.cfg.model
        eng = self.engine
        fpc = int(self.cfg.stac.get("fit_frames_per_clip", 0) or 0)
        kp_np = np.asarray(kp_data, dtype=np.float32)
        valid_np = None
        if valid is not None:
            valid_np = np.asarray(valid)
            if valid_np.dtype != np.bool_ or valid_np.shape != (kp_np.shape[0], len(self._kp_names)):
                raise ValueError(f"fit_offsets: valid must be a bool array [{kp_np.shape[0]}, {len(self._kp_names)}], one entry per frame "
                                 f"and keypoint, got {valid_np.dtype} {valid_np.shape}")
        if fpc > 0:
            kp_np = utils.batch_kp_data(kp_np, fpc, continuous=False)  # [C, F, 3K]; a ragged tail is dropped
            if kp_np.shape[0] == 0:
                raise ValueError(f"fit_frames_per_clip = {fpc} exceeds the {len(kp_data)} fit frames")
            if valid_np is not None:  # (the rows that batch_kp_data kept, cut the same way)
                valid_np = valid_np[: kp_np.shape[0] * fpc].reshape(kp_np.shape[0], fpc, -1)
        else:
            kp_np = kp_np[None]
            valid_np = None if valid_np is None else valid_np[None]
        n_clips, n_per = kp_np.shape[0], kp_np.shape[1]
        n = n_clips * n_per
        lo, hi = dist.shard_range(n_clips) if fpc > 0 else (0, 1)
        kp = torch.as_tensor(kp_np[lo:hi]).to(eng.device)
        valid_dev = None if valid_np is None else torch.as_tensor(np.ascontiguousarray(valid_np[lo:hi])).to(eng.device).reshape(-1, valid_np.shape[-1])
        self.offset_counts = None
        self._offsets = eng.get_site_pos().clone()
        do_root = self.setup.do_root_opt
        if self._root_kp_idx == -1:
            self._log("ROOT_OPTIMIZATION_KEYPOINT not specified, skipping Root Optimization.")
        elif self._fixed:
            self._log("ROOT_OPTIMIZATION_KEYPOINT specified but model has fixed root, skipping Root Optimization")
        n_sample = int(cfgm.N_SAMPLE_FRAMES)
        if time_indices is None:
            time_indices = prng.sample_time_indices(n, n_sample, seed=0)
        tix = np.asarray(time_indices, dtype=np.int64)
        mine = tix[(tix >= lo * n_per) & (tix < hi * n_per)] - lo * n_per  # sampled frames that live on this rank
        idx = torch.as_tensor(mine, dtype=torch.long, device=eng.device)
        is_reg = torch.as_tensor(self._is_regularized).to(eng.device)
        carry = None
        res = None
        for n_iter in range(int(cfgm.N_ITERS) + 1):
            final = n_iter == int(cfgm.N_ITERS)
            self._log("Final pose optimization" if final else f"Calibration iteration: {n_iter + 1}/{cfgm.N_ITERS}")
            # root optimisation happens once, before the first pose pass (stac.py:277-296); the warm start is
            # carried across iterations and into the final pass (stac.py:300-301,331-332)
            res = self._q_phase(kp, do_root_opt=(do_root and n_iter == 0), q_init=carry, want_outputs=final)
            carry = res["carry_qpos"]
            _, mean, std = self._get_error_stats(res["frame_error"].cpu().numpy())
            self._log(f"Mean: {mean}\nStandard deviation: {std}")
            if final:
                break
            # offset phase (compute_stac.py:107-167): regularised toward the PREVIOUS iterate (stac.py:317-328)
            nq = self.setup.tables.nq
            kp_s, q_s = kp.reshape(-1, kp.shape[-1])[idx], res["qpos"].reshape(-1, nq)[idx]
            if valid_dev is None:
                partial = eng.m_partial(kp_s, q_s)
            else:  # observed keypoints only: the kinematics of the sampled poses, then the masked sums
                xpos_s, xquat_s = eng.fk_bodies(q_s)
                partial = eng.m_partial_masked(kp_s, xpos_s, xquat_s, valid_dev[idx])
            if fpc > 0:
                partial = dist.all_reduce_partial(partial)  # the one data-path collective: 3K + 2 floats (4K + 2 with valid)
            if valid_dev is None:
                new_off, err = eng.m_finish(partial, self._offsets, is_reg, float(cfgm.M_REG_COEF))
            else:
                new_off, err, n_obs = eng.m_finish_masked(partial, self._offsets, is_reg, float(cfgm.M_REG_COEF))
                self.offset_counts = {"n": n_obs.cpu().numpy(), "n_sampled": int(tix.size)}
                never = [self._kp_names[k] for k in np.flatnonzero(self.offset_counts["n"] == 0)]
                self._log(f"offset phase on observed keypoints: {len(never)} of {len(self._kp_names)} keypoints were observed in none of the "
                          f"{tix.size} sampled frames" + (": " + ", ".join(never) + " (their offsets follow the regularisation alone)" if never else ""))
            self._log(f"Final residual error of {float(err)}")
            eng.set_site_pos(new_off)
            self._offsets = new_off
        if fpc > 0 and dist.is_dist():
            res, kp_np = self._gather(res, kp_np, n_clips, lo, hi)
        return self._package_data(res, kp_np.reshape(kp_np.shape[0] * n_per, kp_np.shape[-1]), batched=fpc > 0)

    # -- ik_only (stac.py:356-454) --------------------------------------------------------------------------
    def ik_only(self, kp_data, offsets, gather=None, *, post=None, passes=None) -> StacData:
        """Inverse kinematics with fixed offsets; clips are independent chains, sharded over ranks.  ``gather`` (multi-GPU
        result placement: "rank0" | "all" | "none") overrides ``stac.gather`` for this call (run_stac resolves "auto").

        ``passes`` (``stac.seam_passes``, engine extension, 1 .. 8; None: the config's, default 1 = every clip starts cold): the
        clips behind the first are solved ``passes - 1`` times more, each warm-started from the pose that the clip in front of it
        ended in (``_seam_passes``); every output is the last pass's.

        ``post`` (``stac.postprocess: gpu``, engine extension): ``{"continuous", "n_frames_per_clip", "infer_qvels"}`` as the fit
        file's config decided them.  The cross-fade stitch of ``utils.handle_edge_effects`` and the ``qvel`` of
        ``utils.compute_velocity_from_kinematics`` then run on the device (``post.py``), wherever the full tensors are, only
        the stitched arrays cross to the host and the returned ``StacData`` carries ``qvel``.  None: nothing of that.
        An optional ``post["smooth"]`` (``stac.smooth``: ``{"kind", "half_window", "order", "sigma"}``) smooths ``qpos`` per clip
        between the two; the ``StacData`` then carries ``qpos_raw`` and the kinematics of the smoothed pose."""
        eng = self.engine
        passes = seam_options(self.cfg.stac)[0] if passes is None else checked_int(passes, "ik_only: passes", ValueError, 1, SEAM_MAX_PASSES)
        if post is not None:
            post = self._check_post(post, gather)
        tick = self._tick
        tick(None)
        batched = utils.batch_kp_data(np.asarray(kp_data, dtype=np.float32), int(self.cfg.stac.n_frames_per_clip),
                                      continuous=bool(self.cfg.stac.continuous))
        eng.set_site_pos(torch.as_tensor(np.asarray(offsets, dtype=np.float32)).reshape(-1, 3))
        n_clips = batched.shape[0]
        lo, hi = dist.shard_range(n_clips)
        kp = torch.as_tensor(batched[lo:hi]).to(eng.device)
        tick("batch_and_h2d_s")
        if self._root_kp_idx == -1:
            self._log("Missing or invalid ROOT_OPTIMIZATION_KEYPOINT, skipping root_optimization()")
        res = self._q_phase(kp, do_root_opt=self.setup.do_root_opt)
        tick("q_phase_and_fk_kernels_s")
        if passes > 1:
            self._seam_passes(res, kp, n_clips, lo, passes)
            tick("seam_passes_s")
        if dist.is_dist():
            res, batched = self._gather(res, batched, n_clips, lo, hi, mode=gather)
            tick("gather_s")
        _, mean, std = self._get_error_stats(res["frame_error"].cpu().numpy())
        self._log(f"Mean: {mean}\nStandard deviation: {std}")
        self._offsets = eng.get_site_pos()
        extra = None
        if post is not None and not (dist.is_dist() and self._gather_mode(gather) == "rank0" and dist.world()[0] != 0):
            # (a rank that kept only its shard of a rank0 gather has nothing to post-process: rank 0 does it)
            extra = self._postprocess_gpu(res, batched if dist.is_dist() else kp, post)
            tick("postprocess_s")
        data = self._package_data(res, batched, batched=True, post=extra)
        tick("d2h_and_packing_s")
        return data

    def _seam_passes(self, res, kp, n_clips, lo, passes):
        """``stac.seam_passes``: pass p = 2 .. ``passes`` solves every clip but clip 0 again through ``Engine.q_phase``, without root
        optimisation, from the pose that the clip in front of it ended in under pass p - 1: row F - 1 of that clip's ``qpos`` (F =
        ``n_frames_per_clip``; the window of a continuous run has F + 10 rows and row F - 1 is still the frame in front of the next
        window's first).  The warm starts are a copy taken before the launch, and the launch writes into the slices of ``res`` (the
        outputs of pass 1, this rank's clips ``lo ..``) behind clip 0, which keeps its pass-1 result.  Multi-GPU: the clip in front of
        a rank's first one lives on an earlier rank, ``dist.exchange_seam_rows`` brings its row (one all-gather per pass).  With one
        clip there is nothing to do."""
        if n_clips <= 1:
            self._log(f"seam_passes = {passes}: the run is one clip, there is no clip border to warm-start across")
            return
        nq, F = self.setup.tables.nq, int(self.cfg.stac.n_frames_per_clip)
        if not 1 <= F <= kp.shape[1]:
            raise ValueError(f"seam_passes: n_frames_per_clip = {F}, but the clips have {kp.shape[1]} rows")
        n_local = int(kp.shape[0])
        start = 1 if lo == 0 else 0  # (clip 0 is never solved again)
        names = ("qpos", "frame_error", "counters", "carry_qpos", "xpos", "xquat", "marker_sites")
        scalar = None
        if self.verbose:
            from .seam import scalar_columns

            scalar = torch.as_tensor(scalar_columns(nq, self._quat_cols(), 3 if self._freejoint else 0), device=self.engine.device)

        def seam_mean():  # of this rank's own clip borders, over the hinge and slide columns
            if scalar is None or n_local < 2 or scalar.numel() == 0:
                return float("nan")
            q = res["qpos"]
            return float((q[1:, 0][:, scalar] - q[:-1, F - 1][:, scalar]).abs().amax(dim=1).mean())

        for p in range(2, passes + 1):
            before = seam_mean()
            last = res["qpos"][:, F - 1, :]  # [n_local, nq]: the pose every clip of this rank ended in
            rows = [last[:-1]] if n_local else []
            if dist.is_dist():
                incoming = dist.exchange_seam_rows(last[-1] if n_local else None, nq, self.engine.device)
                if start == 0 and n_local:
                    if incoming is None:
                        raise RuntimeError(f"seam_passes: no earlier rank holds the clip in front of clip {lo}")
                    rows.insert(0, incoming.reshape(1, nq))
            if n_local - start < 1:
                continue  # (a rank without a clip behind clip 0 only takes part in the exchange)
            q_init = torch.cat(rows, dim=0).clone() if start == 0 else last[:-1].clone()
            out = {k: res[k][start:] for k in names if res.get(k) is not None}
            self._q_phase(kp[start:], do_root_opt=False, q_init=q_init, out=out)
            self._log(f"seam_passes: pass {p} of {passes}: {n_local - start} clips warm-started; mean seam jump {before:.4f} -> "
                      f"{seam_mean():.4f} rad over this rank's {max(n_local - 1, 0)} borders")

    # -- seam_steps (engine extension; DESIGN.md "Warm-started clips and pose steps") --------------------------------------
    def seam_steps(self, data, clip_len=None) -> dict:
        """The pose steps of a result, on the GPU (``seam.seam_steps``): per row how far the pose moved since the row before it --
        ``step_joint`` (the largest hinge or slide step, rad or m), ``step_col`` (its column), ``step_rot`` (1 - |<a, b>| of the
        quaternions) and ``step_lin2`` (the squared step of the free joint's translation) as numpy arrays -- per column the largest
        step within the clips and across their borders (``col_max_in`` / ``col_max_seam``), and ``summary`` (``seam.summarize``:
        per seam, seam mean / max, the p50 / p99 within the clips, and the marker error of the first frames of the clips against
        the whole run's).  ``data``: a ``StacData``, with this object's config, or the path of a result file (a ``*.manifest.json``
        reads a sharded run), whose stored config decides the clips: ``n_frames_per_clip`` rows, also for a continuous run once it
        is stitched (an unstitched one has windows of ``n_frames_per_clip + 10`` rows).  ``clip_len`` overrides it."""
        from . import io, seam

        cfg = self.cfg
        if not isinstance(data, StacData):
            cfg, data = io.load_stac_result(data)
        qpos = np.asarray(data.qpos, dtype=np.float32)
        nq = self.setup.tables.nq
        if qpos.ndim != 2 or qpos.shape[1] != nq or qpos.shape[0] < 1:
            raise ValueError(f"seam_steps: qpos must be [frames, {nq}] with at least one frame, got {qpos.shape}")
        N, F, ov = qpos.shape[0], int(cfg.stac.n_frames_per_clip), utils.CONTINUOUS_BATCH_OVERLAP
        if clip_len is None:
            clip_len = F + ov if bool(cfg.stac.continuous) and N % F != 0 and N % (F + ov) == 0 else F
        clip_len = checked_int(clip_len, "seam_steps: clip_len", ValueError, 1)
        if N % clip_len != 0:
            raise ValueError(f"seam_steps: cannot cut {N} rows into clips of {clip_len} frames")
        res = seam.seam_steps(torch.as_tensor(np.array(qpos)).to(self.engine.device), clip_len, self._quat_cols(), 3 if self._freejoint else 0)
        markers, kp = np.asarray(data.marker_sites), np.asarray(data.kp_data)
        paired = markers.ndim == 3 and markers.shape[0] == N and kp.ndim == 2 and kp.shape == (N, 3 * markers.shape[1])
        summary = seam.summarize(res, clip_len, data.names_qpos, markers if paired else None, kp if paired else None)
        w = summary["within"]
        self._log(f"seam_steps: {summary['n_seams']} seams of {N} rows (clips of {clip_len}): seam mean / max {summary['seam_mean']} / "
                  f"{summary['seam_max']}; within clips p50 / p99 / max {w['p50']} / {w['p99']} / {w['max']}")
        out = {k: v.cpu().numpy() for k, v in res.items()}
        out["summary"] = summary
        return out

    # -- ground_clearance (engine extension; DESIGN.md "Ground clearance") ------------------------------------------------------
    def ground_table(self, geoms="fitted", geom_groups=None, track=()):
        """``ground.ground_table`` of this model: the scene is compiled as ``render`` compiles it (the same ``SCALE_FACTOR``), once per
        choice of ``geoms`` / ``geom_groups`` / ``track``.  ``ValueError`` for unknown names and for a ``Stac`` without an MJCF file."""
        from . import ground

        key = (geoms if isinstance(geoms, str) else tuple(geoms), None if geom_groups is None else tuple(int(g) for g in geom_groups), tuple(track))
        tables = getattr(self, "_ground_tables", None)
        if tables is None:
            tables = self._ground_tables = {}
        if key not in tables:
            if getattr(self, "_ground_scene", None) is None:
                if self._xml_path is None:
                    raise ValueError("Stac.ground_clearance needs the model's MJCF file: this Stac was built from `setup=` without an xml_path")
                from .mjcf import compile_render_scene

                self._ground_scene = compile_render_scene(self._xml_path, scale=float(self.cfg.model.SCALE_FACTOR), log=self._log)
            tables[key] = ground.ground_table(self._ground_scene, self.setup.tables, geoms, geom_groups, track)
        return tables[key]

    def ground_clearance(self, data, geoms=None, track=None, z_ref=None, permille=None, contact=None) -> dict:
        """How far the fitted body is from the floor, on the GPU (``ground.ground_clearance``): per frame ``low_z``, the lowest world z
        of the included geoms, and ``low_geom``, the table index of the geom that has it; ``track_z`` [N, S], the lowest z of the geoms
        of each tracked body; per geom ``geom_min`` and ``geom_below`` (the frames it spends below ``z_ref``), as numpy arrays;
        ``names`` (the geoms of the table) and ``summary`` (``ground.summarize``: ``floor_z``, the ``permille`` quantile of ``low_z``;
        its minimum, median and maximum; every geom; the geoms that are not included and lie below ``z_ref`` in most frames; per track
        the share of frames within ``contact`` of the floor).  ``data``: a ``StacData`` or the path of a result file (a
        ``*.manifest.json`` reads a sharded run).  Arguments left None come from ``stac.ground_*`` of this object's config."""
        from . import ground, io
        from .config import ground_options

        opt = ground_options(self.cfg.stac)
        geoms = opt["geoms"] if geoms is None else geoms
        track = opt["track"] if track is None else list(track)
        z_ref = opt["z_ref"] if z_ref is None else float(z_ref)
        permille = opt["permille"] if permille is None else checked_int(permille, "ground_clearance: permille", ValueError, 1, 1000)
        contact = opt["contact"] if contact is None else float(contact)
        if not isinstance(data, StacData):
            _, data = io.load_stac_result(data)
        nb = self.setup.tables.nbody
        xpos, xquat = np.asarray(data.xpos, dtype=np.float32), np.asarray(data.xquat, dtype=np.float32)
        if xpos.ndim != 3 or xpos.shape[1:] != (nb, 3) or xquat.shape != (xpos.shape[0], nb, 4) or xpos.shape[0] < 1:
            raise ValueError(f"ground_clearance: xpos / xquat must be [frames, {nb}, 3 / 4] with at least one frame, got {xpos.shape} / {xquat.shape}")
        table = self.ground_table(geoms, opt["geom_groups"], track)
        dev = self.engine.device
        res = ground.ground_clearance(torch.as_tensor(np.array(xpos)).to(dev), torch.as_tensor(np.array(xquat)).to(dev), table, z_ref)
        summary = ground.summarize(res, table, z_ref, permille, contact)
        lz = summary["low_z"]
        self._log(f"ground_clearance: {summary['n_frames']} frames, {summary['n_included']} of {summary['n_geoms']} geoms included: floor_z "
                  f"{summary['floor_z']} (permille {permille}); low_z min / median / max {lz['min']} / {lz['median']} / {lz['max']}; "
                  f"{len(summary['unfitted_below'])} geoms that are not included lie below z = {z_ref:g} in most frames")
        out = {k: v.cpu().numpy() for k, v in res.items()}
        out["names"] = list(table.names)
        out["summary"] = summary
        return out

    def _check_post(self, post, gather):
        """The ``post`` argument of ik_only, checked before any work is done."""
        out = {"continuous": bool(post["continuous"]), "n_frames_per_clip": int(post["n_frames_per_clip"]),
               "infer_qvels": bool(post["infer_qvels"])}
        if out["n_frames_per_clip"] < 1:
            raise ValueError(f"post: n_frames_per_clip = {out['n_frames_per_clip']}")
        if out["continuous"] and bool(self.cfg.stac.get("reference_marker_order", False)):
            raise ValueError(POSTPROCESS_GPU_MARKER_ORDER)
        if out["continuous"] and dist.world()[1] > 1 and self._gather_mode(gather) == "none":
            raise ValueError(GATHER_NONE_CONTINUOUS)
        if post.get("smooth"):
            from . import post as gpost

            sm = dict(post["smooth"])
            if bool(self.cfg.stac.get("reference_marker_order", False)):
                raise ValueError(smooth_marker_order_refusal(sm["kind"]))
            # (every bad kind / half_window / order / sigma is a ValueError of smooth_taps)
            out["smooth"] = {"kind": sm["kind"], "half_window": int(sm["half_window"]),
                             "taps": gpost.smooth_taps(sm["kind"], sm["half_window"], order=sm.get("order"), sigma=sm.get("sigma"))}
            if not out["continuous"] and out["n_frames_per_clip"] < 2 * out["smooth"]["half_window"] + 1:
                raise ValueError(f"stac.smooth: clips of {out['n_frames_per_clip']} frames are shorter than the window of "
                                 f"{2 * out['smooth']['half_window'] + 1} frames")
        return out

    def _quat_cols(self):
        """First columns of the quaternion blocks of a qpos row: the free joint's (its address + 3) and every ball joint's."""
        from .mjcf import JNT_BALL, JNT_FREE

        t = self.setup.tables
        jt, adr = np.asarray(t.jnt_type), np.asarray(t.jnt_qposadr)
        return [int(a) + 3 for a in adr[jt == JNT_FREE]] + [int(a) for a in adr[jt == JNT_BALL]]

    def _smooth_gpu(self, qpos, clip_len, taps):
        """``post.smooth`` of a flat device ``qpos`` with this model's quaternion columns and the engine's bounds, and the
        kinematics of the result under the offsets the engine holds -> {qpos, xpos, xquat, marker_sites} (device)."""
        from . import post as gpost

        q = gpost.smooth(qpos, clip_len, taps, self._quat_cols(), lb=self.engine.lb, ub=self.engine.ub)
        fk = self.engine.fk(q, want=("xpos", "xquat", "site_xpos"))
        return {"qpos": q, "xpos": fk["xpos"], "xquat": fk["xquat"], "marker_sites": fk["site_xpos"]}

    def _postprocess_gpu(self, res, kp_clips, post):
        """Stitch (continuous) and qvel (infer_qvels) of the flattened outputs on the device -> {name: device tensor}."""
        from . import post as gpost

        F, ov = post["n_frames_per_clip"], utils.CONTINUOUS_BATCH_OVERLAP
        nq, nb, K = self.setup.tables.nq, self.setup.tables.nbody, self.setup.tables.nsite
        kp_dev = torch.as_tensor(kp_clips).to(device=self.engine.device, dtype=torch.float32)
        out = {"qpos": res["qpos"].reshape(-1, nq), "xpos": res["xpos"].reshape(-1, nb, 3), "xquat": res["xquat"].reshape(-1, nb, 4),
               "marker_sites": res["marker_sites"].reshape(-1, K, 3), "kp_data": kp_dev.reshape(-1, kp_dev.shape[-1])}
        if post["continuous"]:
            for name, a in out.items():  # the flat rows as windows of F + 10, as handle_edge_effects reshapes them
                if a.shape[0] % (F + ov) != 0:
                    raise ValueError(f"cannot reshape {a.shape[0]} rows of {name} into windows of {F + ov} frames")
                out[name] = gpost.stitch(a.reshape((-1, F + ov) + tuple(a.shape[1:])), F, ov)
        if post.get("smooth") and out["qpos"].shape[0]:
            # stac.smooth: the fitted pose stays as qpos_raw; qpos, and the kinematics that go with it, are the smoothed one's.  A
            # continuous run is one clip (the stitched rows), else clips are the F rows they were solved as: no window crosses a border
            out["qpos_raw"] = out["qpos"]
            out.update(self._smooth_gpu(out["qpos"], out["qpos"].shape[0] if post["continuous"] else F, post["smooth"]["taps"]))
        if post["infer_qvels"] and out["qpos"].shape[0]:
            out["qvel"] = gpost.infer_qvel(out["qpos"], F, self._timestep, self._freejoint)
        return out

    def _tick(self, name):
        """Phase clock of ik_only for `bench.py --mode run` (``self.timings = {}`` switches it on; it synchronises the device
        at every phase boundary, so it is off by default)."""
        if self.timings is None:
            return
        import time

        torch.cuda.synchronize(self.engine.device)
        now = time.perf_counter()
        if name is not None:
            self.timings[name] = self.timings.get(name, 0.0) + now - self._t_last
        self._t_last = now

    def _gather_mode(self, mode=None) -> str:
        mode = str(mode or self.cfg.stac.get("gather", "rank0") or "rank0")
        if mode == "auto":  # run_stac resolves "auto" by output size before it calls ik_only; direct callers get rank0
            mode = "rank0"
        if mode not in ("rank0", "all", "none"):
            raise ValueError(f"stac.gather must be auto, rank0, all or none, not {mode!r}")
        return mode

    def _gather(self, res, kp_clips, n_clips, lo, hi, mode=None):
        """Multi-GPU result placement, ``stac.gather`` (engine extension): "rank0" (default) -- rank 0 packages every
        clip, the other ranks keep (and return) their own shard; "all" -- every rank gets every clip (small runs,
        tests); "none" -- every rank keeps its shard.  Returns (results, the keypoint clips that go with them)."""
        mode = self._gather_mode(mode)
        tensors = {k: v for k, v in res.items() if isinstance(v, torch.Tensor)}
        if mode == "all":
            return {k: dist.all_gather_clips(v, n_clips) for k, v in tensors.items()}, kp_clips
        if mode == "rank0":
            full = {k: dist.gather_clips(v, n_clips, dst=0) for k, v in tensors.items()}
            if dist.world()[0] == 0:
                return full, kp_clips
        return tensors, kp_clips[lo:hi]

    # -- packing (stac.py:456-503) ---------------------------------------------------------------------------
    def _package_data(self, res, kp_data, batched=False, post=None) -> StacData:
        """Clip-major flatten of every field.

        The reference flattens ``marker_sites`` frame-major when C > 1 and F > 1 (``stac.py:486``: a C-order
        reshape of the (F, C, K, 3) stack, while qpos / xpos / xquat / kp_data come out clip-major -- SURVEY.md
        A5-7, a reference bug).  Default here: all fields clip-major, row i of every field is the same frame.
        ``stac.reference_marker_order: true`` reproduces the reference's row order of ``marker_sites`` exactly
        (row j = frame j // C of clip j % C) for consumers that undo it themselves."""
        nq, nb, K = self.setup.tables.nq, self.setup.tables.nbody, self.setup.tables.nsite
        if post is not None:  # stac.postprocess = gpu: the arrays are stitched and flat already (_postprocess_gpu)
            host = {k: v.cpu().numpy() for k, v in post.items()}
        else:
            host = {"qpos": res["qpos"].reshape(-1, nq).cpu().numpy(), "xpos": res["xpos"].reshape(-1, nb, 3).cpu().numpy(),
                    "xquat": res["xquat"].reshape(-1, nb, 4).cpu().numpy(),
                    "kp_data": np.asarray(kp_data).reshape(-1, np.asarray(kp_data).shape[-1])}
        marker_order = batched and bool(self.cfg.stac.get("reference_marker_order", False))
        if post is None or marker_order:  # (with post never a continuous run: _check_post)
            ms = res["marker_sites"]
            if marker_order and ms.dim() == 4:
                ms = ms.transpose(0, 1)  # (C, F, K, 3) -> (F, C, K, 3), flattened in C order like stac.py:486
            host["marker_sites"] = ms.reshape(-1, K, 3).cpu().numpy()
        return StacData(offsets=np.asarray(torch.as_tensor(self._offsets).cpu()).reshape(K, 3), names_qpos=self._part_names,
                        names_xpos=self._body_names, kp_names=self._kp_names, **host)

    # -- render (stac.py:505-658) -------------------------------------------------------------------------------
    def _get_renderer(self, geom_groups=None):
        key = None if geom_groups is None else tuple(int(g) for g in geom_groups)
        if self._renderer is not None and getattr(self, "_renderer_groups", None) != key:
            self._renderer.close()
            self._renderer = None
        if self._renderer is None:
            if self._xml_path is None:
                raise ValueError("Stac.render needs the model's MJCF file: this Stac was built from `setup=` without an xml_path")
            from .mjcf import compile_render_scene
            from .render import Renderer

            cfgm = self.cfg.model
            pairs = dict(cfgm.KEYPOINT_MODEL_PAIRS)
            colours = dict(cfgm.KEYPOINT_COLOR_PAIRS)
            rgba = [[float(c) for c in v.split()] if isinstance(v, str) else [float(c) for c in v] for v in (colours[k] for k in pairs)]
            scene = compile_render_scene(self._xml_path, scale=float(cfgm.SCALE_FACTOR), log=self._log)
            self._renderer = Renderer(self.engine, scene, list(pairs), list(pairs.values()), rgba,
                                      marker_size=float(cfgm.get("MARKER_SIZE", 0.005) if hasattr(cfgm, "get") else cfgm.MARKER_SIZE),
                                      geom_groups=key)
            self._renderer_groups = key
        return self._renderer

    def render(self, qposes, kp_data, offsets, n_frames, save_path, start_frame=0, camera=0, height=1200, width=1920,
               show_marker_error=False, *, geom_groups=None, encoder="pil", return_frames=True):
        """Render fitted results as a video (the reference's signature and checks, ``stac.py:569-658``); returns the list of
        H x W x 3 uint8 frames.  ``camera``: index, name, or -1 (free camera).  ``geom_groups``: the geom groups to draw
        (None = the reference's rule, groups 0 and 2).  The engine's state is left as it was.

        ``encoder``: "pil" (default: frames go to the host and are encoded there) or "gpu" (``.avi`` only: the frames are
        JPEG-encoded on the device, ``stac_mjx_amd.jpeg``, and only the compressed stream crosses to the host).
        ``return_frames=False`` returns ``[]``; with the GPU encoder the raw frames then never leave the device."""
        if encoder not in ("pil", "gpu"):
            raise ValueError(f"unknown encoder {encoder!r}: 'pil' or 'gpu'")
        if encoder == "gpu" and Path(save_path).suffix.lower() != ".avi":
            raise ValueError(f"encoder='gpu' writes MJPEG .avi only (imageio needs raw frames): got {save_path}")
        qposes, kp_data = np.asarray(qposes), np.asarray(kp_data)
        if qposes.shape[0] != kp_data.shape[0]:
            raise ValueError(
                f"Length of qposes ({qposes.shape[0]}) is not equal to the length of kp_data({kp_data.shape[0]})")
        if start_frame < 0 or start_frame > kp_data.shape[0]:
            raise ValueError(
                f"start_frame ({start_frame}) must be non-negative and less than the length of kp_data ({kp_data.shape[0]})")
        if start_frame + n_frames > kp_data.shape[0]:
            raise ValueError(
                f"start_frame + n_frames ({start_frame} + {n_frames}) must be less than the length of given qposes and kp_data ({kp_data.shape[0]})")
        r = self._get_renderer(geom_groups)
        r.camera_index(camera)
        from .video import write_video

        sl = slice(start_frame, start_frame + n_frames)
        t = self.setup.tables
        if encoder == "gpu":
            from .video import write_avi

            out = r.render(qposes[sl], kp_data[sl], offsets, qpos0=t.qpos0, parent=t.body_parentid, camera=camera, width=width,
                           height=height, show_marker_error=show_marker_error, want_jpeg=True, want_rgb=bool(return_frames))
            write_avi(save_path, None, fps=float(self.cfg.model.RENDER_FPS), jpegs=out["jpeg"], size=(width, height))
            return list(out["rgb"].numpy()) if return_frames else []
        out = r.render(qposes[sl], kp_data[sl], offsets, qpos0=t.qpos0, parent=t.body_parentid, camera=camera, width=width,
                       height=height, show_marker_error=show_marker_error)
        frames = list(out["rgb"].numpy())
        write_video(save_path, frames, fps=float(self.cfg.model.RENDER_FPS), log=self._log)
        return frames if return_frames else []
