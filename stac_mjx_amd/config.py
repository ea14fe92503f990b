"""Config loading that keeps the reference's ``configs/*.yaml`` surface without Hydra/OmegaConf.

The reference composes ``configs/config.yaml`` (a Hydra ``defaults:`` list selecting one file of
the ``stac/`` group and one of the ``model/`` group) and merges the result into the structured
schema ``Config(model: ModelConfig, stac: StacConfig)`` (``stac_mjx/config.py:11-88``).  This
module does the same with PyYAML: ``defaults`` list, ``group=name`` / dotted ``a.b=value``
overrides, schema check, attribute access.
"""

from __future__ import annotations

import math
from pathlib import Path
from typing import Any, Iterable

import yaml

# Required keys (reference: stac_mjx/config.py:11-62).  MARKER_SIZE has a default there (:36).
_MODEL_REQUIRED = (
    "MJCF_PATH", "FTOL", "ROOT_FTOL", "LIMB_FTOL", "N_ITERS", "N_ITER_Q", "KP_NAMES",
    "KEYPOINT_MODEL_PAIRS", "KEYPOINT_INITIAL_OFFSETS", "ROOT_OPTIMIZATION_KEYPOINT",
    "TRUNK_OPTIMIZATION_KEYPOINTS", "INDIVIDUAL_PART_OPTIMIZATION", "KEYPOINT_COLOR_PAIRS",
    "SCALE_FACTOR", "MOCAP_SCALE_FACTOR", "SITES_TO_REGULARIZE", "RENDER_FPS", "N_SAMPLE_FRAMES",
    "M_REG_COEF",
)  # fmt: skip
_MODEL_DEFAULTS = {"MARKER_SIZE": 0.005}
_STAC_REQUIRED = (
    "fit_offsets_path", "ik_only_path", "data_path", "n_fit_frames", "skip_fit_offsets",
    "skip_ik_only", "infer_qvels", "n_frames_per_clip", "mujoco", "continuous",
)  # fmt: skip
_STAC_OPTIONAL = ("num_clips",)
_MUJOCO_REQUIRED = ("solver", "iterations", "ls_iterations")
# Engine extensions (not in the reference schema); all optional.  (lm_maxiter: accepted steps per solve of solver = lm, default 20
# -- 40 until round 3; gather: auto | rank0 | all | none, resolved per run by main.run_stac, the caller's config is never modified;
# postprocess: host (default) | gpu -- where the cross-fade stitch and qvel of a run happen, read from the caller's config;
# fill_missing: off (default) | linear | hold -- missing keypoints are filled along time before the fit, read from the caller's config;
# reject_outliers: off (default) | hampel, with outlier_window (half-width, 1 .. 16, default 5), outlier_nsigma (default 3.0) and
# outlier_min_dev (default 0.001, units of kp_data) -- finite but wrong keypoints become missing ones in front of fill_missing;
# reject_pairwise: off (default) | mad, with pairwise_nsigma (default 6.0), pairwise_min_dev (default 0.002, units of kp_data) and
# pairwise_votes (default 2) -- keypoints that leave the distributions of their distances to the other keypoints over the whole series
# become missing ones, in front of reject_outliers and fill_missing;
# repair_swaps: off (default) | lr | [[nameA, nameB], ...], with swaps_nsigma (default 6.0), swaps_min_dev (default 0.002, units of
# kp_data) and swaps_min_bad (default 3) -- two keypoints of a candidate pair that carry each other's label in a frame are exchanged
# back, in front of everything else; it makes no NaN and needs no fill_missing;
# fill_donors: off (default) | auto, with fill_donors_triples (donor triples per keypoint, 1 .. 8, default 4) -- a missing keypoint is
# carried through its gap by the local frame of three rigid partners that are still tracked, after the rejecters and directly in front
# of fill_missing, which closes what is left;
# report: off (default) | on, with report_quantiles (1 .. 8 permille values, default [500, 900, 990]) and report_worst (frames listed,
# default 10) -- a <result file>.report.json next to every result file, read from the caller's config;
# smooth: off (default) | savgol | gaussian, with smooth_window (half-width H, 1 .. 16, default 3: windows of 2 H + 1 frames),
# smooth_order (savgol: the polynomial order, 0 <= order < 2 H + 1, default 2) and smooth_sigma (gaussian: frames, > 0, default H / 2)
# -- the qpos of an ik_only run is low-pass filtered per clip on the GPU between the stitch and qvel, the file gains qpos_raw and its
# xpos / xquat / marker_sites are those of the smoothed pose; needs postprocess = gpu, read from the caller's config;
# resample: off (default) | kaiser, with mocap_hz (the rate of the recording), resample_hz (the rate wanted), resample_lobes (zero
# crossings of the sinc on each side, 1 .. 16, default 10) and resample_beta (the Kaiser window's, >= 0, default 5.0) -- the ik_only
# result is resampled per clip on the GPU into a second file next to the first, which does not change; needs postprocess = gpu, read
# from the caller's config;
# fit_frames: first (default) | strided | diverse -- which n_fit_frames rows of the prepared series calibrate the offsets: the first
# ones (the reference), every (candidates / n)-th candidate, or the frames whose pairwise keypoint distances differ most (greedy
# farthest-point selection on the GPU); strided and diverse pass over every frame that a preparation stage marked, hand the rows
# to fit_offsets in ascending time order and write <fit file>.frames.json next to the fit file, read from the caller's config;
# offset_mask: off (default) | observed -- the offset phase of fit_offsets sums over the keypoints that were observed (kp_gap == 0)
# and leaves filled values out, the pose phase still sees the filled series; needs fill_missing; writes <fit file>.offsets.json with
# the observed count of every keypoint; with it fit_frames_min_observed (q in (0, 1], default 1.0 = today's rule) lets strided and
# diverse take a frame of which at least ceil(q K) keypoints are observed; read from the caller's config;
# seam_passes: 1 (default) .. 8 -- ik_only solves the clips behind the first again, P - 1 times, each warm-started from the pose
# that the clip in front of it ended in, without root optimisation; seam_report: off (default) | on -- a <ik file>.seams.json with
# the pose steps across and within the clips, measured on the GPU; both read from the caller's config;
# ground: off (default) | report | level -- the ground clearance of the ik_only result, measured on the GPU: report writes
# <ik file>.ground.json (per frame the lowest geom, per geom its lowest z and the frames it spends under ground_z, the floor of the
# recording as the ground_permille quantile of the per-frame lowest z, per ground_track body the share of frames within
# ground_contact of it); level (free-root models) also subtracts that floor from the z of the packaged result; ground_geoms: fitted
# (default: the geoms of the bodies the fit can move) | all | a list of geom or body names; ground_geom_groups: the geom groups that
# enter (default all); ground_floor_z: written by a level run into the stored config, the floor it subtracted; read from the
# caller's config)
_STAC_EXTENSIONS = ("solver", "lanes_per_chain", "device", "time_indices", "fit_frames_per_clip", "reference_marker_order", "gather", "gather_max_bytes", "lm_maxiter", "postprocess", "fill_missing",
                    "reject_outliers", "outlier_window", "outlier_nsigma", "outlier_min_dev", "report", "report_quantiles", "report_worst",
                    "smooth", "smooth_window", "smooth_order", "smooth_sigma",
                    "reject_pairwise", "pairwise_nsigma", "pairwise_min_dev", "pairwise_votes",
                    "repair_swaps", "swaps_nsigma", "swaps_min_dev", "swaps_min_bad",
                    "fill_donors", "fill_donors_triples",
                    "resample", "mocap_hz", "resample_hz", "resample_lobes", "resample_beta",
                    "fit_frames", "offset_mask", "fit_frames_min_observed",
                    "seam_passes", "seam_report",
                    "ground", "ground_geoms", "ground_geom_groups", "ground_track", "ground_z", "ground_permille", "ground_contact", "ground_floor_z")
_MODEL_EXTENSIONS = ("KP_NAMES_LABEL3D_PATH",)


class ConfigError(ValueError):
    pass


INT32_MAX = 2**31 - 1  # what a count that crosses the C ABI as int32_t holds


def checked_number(v, name, exc, positive: bool = False) -> float:
    """``v`` as a float if it is a finite number (no bool) >= 0, or > 0 with ``positive``; else ``exc`` with "<name> must be ...".
    The one value check of the ``*_options`` below (name: ``stac.<key>``, ConfigError) and of ``prep.*_params`` (name:
    ``<function>: <parameter>``, ValueError)."""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0 or (positive and not v > 0):
        raise exc(f"{name} must be a finite number {'> 0' if positive else '>= 0'}, not {v!r}")
    return float(v)


def checked_int(v, name, exc, lo: int, hi=None, text=None) -> int:
    """``v`` if it is an integer (no bool) in ``lo .. hi`` (``hi`` None: no upper bound); else ``exc`` with "<name> must be <text>":
    ``text`` is "an integer in lo .. hi" or "an integer >= lo" unless given."""
    if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
        text = text or (f"an integer >= {lo}" if hi is None else f"an integer in {lo} .. {hi}")
        raise exc(f"{name} must be {text}, not {v!r}")
    return v


def _sigma_options(stac, defaults, prefix) -> list:
    """``stac.<prefix>_nsigma`` and ``stac.<prefix>_min_dev`` (absent: their defaults) as floats."""
    return [checked_number(stac.get(key, defaults[key]), f"stac.{key}", ConfigError) for key in (prefix + "_nsigma", prefix + "_min_dev")]


def _switch(stac, key):
    """``stac[key]`` of a key whose first value is ``off`` (absent: off).  YAML 1.1 reads a bare ``off`` / ``on`` as a boolean: False is
    off, and True is on for ``report``, the one key that has an ``on``.  A key without a value (None) is off, except ``fill_missing``."""
    v = stac.get(key, "off")
    if v is False or (v is None and key != "fill_missing"):
        return "off"
    return "on" if v is True and key == "report" else v


def postprocess_options(stac) -> str:
    """``stac.postprocess`` out of a ``stac`` mapping -> "host" (default) | "gpu"; ``ConfigError`` for anything else."""
    mode = stac.get("postprocess", "host")
    if mode not in ("host", "gpu"):
        raise ConfigError(f"stac.postprocess must be host or gpu, not {mode!r}")
    return mode


def fill_missing_options(stac) -> str:
    """``stac.fill_missing`` out of a ``stac`` mapping -> "off" (default) | "linear" | "hold"; ``ConfigError`` for anything else."""
    mode = _switch(stac, "fill_missing")
    if not isinstance(mode, str) or mode not in ("off", "linear", "hold"):
        raise ConfigError(f"stac.fill_missing must be off, linear or hold, not {mode!r}")
    return mode


OUTLIER_DEFAULTS = {"outlier_window": 5, "outlier_nsigma": 3.0, "outlier_min_dev": 0.001}
OUTLIER_MAX_WINDOW = 16  # csrc/stac_outlier.hpp: kOutlierMaxHalf


def outlier_options(stac) -> tuple:
    """``stac.reject_outliers`` and its three parameters out of a ``stac`` mapping -> (mode, half_window, n_sigma, min_dev), absent
    keys at their defaults.  ``ConfigError`` for anything else than off | hampel, a half-width that is not an integer in 1 .. 16,
    or an ``outlier_nsigma`` / ``outlier_min_dev`` that is not a finite number >= 0."""
    mode = _switch(stac, "reject_outliers")
    if not isinstance(mode, str) or mode not in ("off", "hampel"):
        raise ConfigError(f"stac.reject_outliers must be off or hampel, not {mode!r}")
    h = checked_int(stac.get("outlier_window", OUTLIER_DEFAULTS["outlier_window"]), "stac.outlier_window (the half-width in frames)",
                    ConfigError, 1, OUTLIER_MAX_WINDOW)
    n_sigma, min_dev = _sigma_options(stac, OUTLIER_DEFAULTS, "outlier")
    return mode, h, n_sigma, min_dev


PAIRWISE_DEFAULTS = {"pairwise_nsigma": 6.0, "pairwise_min_dev": 0.002, "pairwise_votes": 2}
# the one text of run_stac's pre-flight and of main._reject_pairwise_mode
PAIRWISE_NEEDS_FILL = ("stac.reject_pairwise = mad turns the keypoints it rejects into missing ones (NaN), which the solver cannot take: "
                       "set stac.fill_missing to linear or hold as well")


def pairwise_options(stac) -> tuple:
    """``stac.reject_pairwise`` and its three parameters out of a ``stac`` mapping -> (mode, n_sigma, min_dev, votes), absent keys
    at their defaults.  ``ConfigError`` for anything else than off | mad (a bare YAML ``off`` arrives as False), a
    ``pairwise_nsigma`` / ``pairwise_min_dev`` (units of kp_data) that is not a finite number >= 0, or a ``pairwise_votes`` that
    is not an integer >= 1."""
    mode = _switch(stac, "reject_pairwise")
    if not isinstance(mode, str) or mode not in ("off", "mad"):
        raise ConfigError(f"stac.reject_pairwise must be off or mad, not {mode!r}")
    n_sigma, min_dev = _sigma_options(stac, PAIRWISE_DEFAULTS, "pairwise")
    votes = checked_int(stac.get("pairwise_votes", PAIRWISE_DEFAULTS["pairwise_votes"]), "stac.pairwise_votes", ConfigError, 1, INT32_MAX,
                        "an integer >= 1")
    return mode, n_sigma, min_dev, votes


SWAPS_DEFAULTS = {"swaps_nsigma": 6.0, "swaps_min_dev": 0.002, "swaps_min_bad": 3}


def lr_pairs(kp_names) -> list:
    """The left / right keypoint pairs of a list of names as ``(index of the L name, index of the R name)``.  The partner of a name
    is the name with a trailing ``L`` replaced by ``R`` if that name exists (the rodent's ``AnkleL``, the mouse's ``Knee_L`` and
    ``Lisfranc_L``), otherwise the name with a leading ``L`` replaced by ``R`` if that exists (the fly's ``L1A``).  In the order of
    the sorted names of the L side; a keypoint is in at most one pair (the first that claims it)."""
    names = [str(n) for n in kp_names]
    where = {n: i for i, n in reversed(list(enumerate(names)))}  # (a repeated name: its first index)
    out, used = [], set()
    for n in sorted(where):
        partner = None
        if n.endswith("L") and n[:-1] + "R" in where:
            partner = n[:-1] + "R"
        elif n.startswith("L") and "R" + n[1:] in where:
            partner = "R" + n[1:]
        if partner is None or n in used or partner in used:
            continue
        used.update((n, partner))
        out.append((where[n], where[partner]))
    return out


def named_pairs(pairs, kp_names) -> list:
    """``[[nameA, nameB], ...]`` -> ``[(index of A, index of B), ...]``.  ``ConfigError`` for a name that ``kp_names`` does not hold,
    a pair of one name, or a keypoint in two pairs."""
    names = [str(n) for n in kp_names]
    out, used = [], set()
    for a, b in pairs:
        for n in (a, b):
            if n not in names:
                raise ConfigError(f"stac.repair_swaps names the keypoint {n!r}, which is not among the keypoints {names}")
        if a == b:
            raise ConfigError(f"stac.repair_swaps: the pair [{a}, {b}] names one keypoint twice")
        for n in (a, b):
            if n in used:
                raise ConfigError(f"stac.repair_swaps: the keypoint {n!r} is in two pairs")
        used.update((a, b))
        out.append((names.index(a), names.index(b)))
    return out


def swaps_options(stac) -> tuple:
    """``stac.repair_swaps`` and its three parameters out of a ``stac`` mapping -> (mode, n_sigma, min_dev, min_bad), absent keys at
    their defaults; mode is "off" (default; a bare YAML ``off`` arrives as False), "lr" (the left / right pairs of the keypoint
    names: ``lr_pairs``) or a list of ``[nameA, nameB]`` pairs.  ``ConfigError`` for anything else, a ``swaps_nsigma`` /
    ``swaps_min_dev`` (units of kp_data) that is not a finite number >= 0, or a ``swaps_min_bad`` that is not an integer >= 1.
    Whether the names exist is for ``swaps_candidates``, which knows the keypoints."""
    mode = _switch(stac, "repair_swaps")
    if isinstance(mode, (list, tuple)):
        if not mode:
            raise ConfigError("stac.repair_swaps: an empty list of pairs repairs nothing: say off")
        pairs = []
        for p in mode:
            if not isinstance(p, (list, tuple)) or len(p) != 2 or not all(isinstance(n, str) and n for n in p):
                raise ConfigError(f"stac.repair_swaps: a candidate is a pair [nameA, nameB] of keypoint names, not {p!r}")
            pairs.append((p[0], p[1]))
        mode = pairs
    elif not isinstance(mode, str) or mode not in ("off", "lr"):
        raise ConfigError(f"stac.repair_swaps must be off, lr or a list of [nameA, nameB] pairs, not {mode!r}")
    n_sigma, min_dev = _sigma_options(stac, SWAPS_DEFAULTS, "swaps")
    min_bad = checked_int(stac.get("swaps_min_bad", SWAPS_DEFAULTS["swaps_min_bad"]), "stac.swaps_min_bad", ConfigError, 1, INT32_MAX,
                          "an integer >= 1")
    return mode, n_sigma, min_dev, min_bad


def swaps_candidates(mode, kp_names) -> list:
    """The candidates of a run as index pairs from the mode of ``swaps_options`` and the run's keypoint names: [] for off.
    ``ConfigError`` for unknown names, a keypoint in two pairs, or ``lr`` with names that hold no left / right pair."""
    if mode == "off":
        return []
    if mode == "lr":
        pairs = lr_pairs(kp_names)
        if not pairs:
            raise ConfigError(f"stac.repair_swaps = lr finds no left / right pair among the keypoints {[str(n) for n in kp_names]}: "
                              "name the pairs as [[nameA, nameB], ...]")
        return pairs
    return named_pairs(mode, kp_names)


DONOR_DEFAULTS = {"fill_donors_triples": 4}
DONOR_MAX_TRIPLES = 8  # csrc/stac_donor.hpp: kDonorMaxTriples
# the one text of run_stac's pre-flight and of main._fill_donors_mode
DONORS_NEED_FILL = ("stac.fill_donors = auto leaves missing what no donor triple can fill (NaN), which the solver cannot take: "
                    "set stac.fill_missing to linear or hold as well")


def donor_options(stac) -> tuple:
    """``stac.fill_donors`` and its parameter out of a ``stac`` mapping -> (mode, n_triples), absent keys at their defaults.
    ``ConfigError`` for anything else than off | auto (a bare YAML ``off`` arrives as False) or a ``fill_donors_triples`` that is not
    an integer in 1 .. 8."""
    mode = _switch(stac, "fill_donors")
    if not isinstance(mode, str) or mode not in ("off", "auto"):
        raise ConfigError(f"stac.fill_donors must be off or auto, not {mode!r}")
    n_triples = checked_int(stac.get("fill_donors_triples", DONOR_DEFAULTS["fill_donors_triples"]), "stac.fill_donors_triples", ConfigError,
                            1, DONOR_MAX_TRIPLES)
    return mode, n_triples


FIT_FRAMES_MODES = ("first", "strided", "diverse")


def fit_frames_options(stac) -> str:
    """``stac.fit_frames`` out of a ``stac`` mapping -> "first" (default, also for a key without a value) | "strided" | "diverse";
    ``ConfigError`` for anything else."""
    mode = stac.get("fit_frames", "first")
    mode = "first" if mode is None else mode
    if not isinstance(mode, str) or mode not in FIT_FRAMES_MODES:
        raise ConfigError(f"stac.fit_frames must be first, strided or diverse, not {mode!r}")
    return mode


OFFSET_MASK_DEFAULTS = {"fit_frames_min_observed": 1.0}
# the one text of run_stac's pre-flight and of main._offset_mask_mode
OFFSET_MASK_NEEDS_FILL = ("stac.offset_mask = observed reads which keypoint values are observations from kp_gap, the mark of "
                          "stac.fill_missing: set stac.fill_missing to linear or hold as well")


def offset_mask_options(stac) -> tuple:
    """``stac.offset_mask`` and ``stac.fit_frames_min_observed`` out of a ``stac`` mapping -> (mode, q), absent keys at their defaults.
    ``ConfigError`` for anything else than off | observed (a bare YAML ``off`` arrives as False), for a q that is not a number in
    (0, 1], and for a q other than 1.0 with the mask off: only the masked offset phase can take a frame with filled keypoints."""
    mode = _switch(stac, "offset_mask")
    if not isinstance(mode, str) or mode not in ("off", "observed"):
        raise ConfigError(f"stac.offset_mask must be off or observed, not {mode!r}")
    q = stac.get("fit_frames_min_observed", OFFSET_MASK_DEFAULTS["fit_frames_min_observed"])
    q = OFFSET_MASK_DEFAULTS["fit_frames_min_observed"] if q is None else q
    if isinstance(q, bool) or not isinstance(q, (int, float)) or not math.isfinite(q) or not 0 < q <= 1:
        raise ConfigError(f"stac.fit_frames_min_observed must be a number in (0, 1], not {q!r}")
    if mode == "off" and float(q) != 1.0:
        raise ConfigError(f"stac.fit_frames_min_observed = {q!r} is honoured only with stac.offset_mask = observed: without the mask the "
                          "offset phase fits filled keypoints like observed ones, so it must stay 1.0")
    return mode, float(q)


SEAM_MAX_PASSES = 8


def seam_options(stac) -> tuple:
    """``stac.seam_passes`` and ``stac.seam_report`` out of a ``stac`` mapping -> (passes, report on), absent keys (and keys without
    a value) at their defaults 1 and off.  ``ConfigError`` for passes that are not an integer in 1 .. 8 and for anything else than
    off | on (or the bool that a bare YAML off / on arrives as)."""
    p = stac.get("seam_passes", 1)
    p = checked_int(1 if p is None else p, "stac.seam_passes", ConfigError, 1, SEAM_MAX_PASSES)
    mode = stac.get("seam_report", "off")
    mode = "off" if mode is None or mode is False else ("on" if mode is True else mode)
    if not isinstance(mode, str) or mode not in ("off", "on"):
        raise ConfigError(f"stac.seam_report must be off or on, not {mode!r}")
    return p, mode == "on"


GROUND_MODES = ("off", "report", "level")
GROUND_DEFAULTS = {"ground_geoms": "fitted", "ground_track": (), "ground_z": 0.0, "ground_permille": 50, "ground_contact": 0.002}
GROUND_MAX_TRACK = 32  # csrc/ground/stac_ground.hpp: kGroundMaxSlots


def _name_list(v, name) -> list:
    if not isinstance(v, (list, tuple)) or not all(isinstance(n, str) and n for n in v):
        raise ConfigError(f"{name} must be a list of names, not {v!r}")
    return [str(n) for n in v]


def ground_options(stac) -> dict:
    """``stac.ground`` and its six parameters out of a ``stac`` mapping -> ``{"mode", "geoms", "geom_groups", "track", "z_ref",
    "permille", "contact"}``, absent keys (and keys without a value) at their defaults.  ``ConfigError`` for anything else than off |
    report | level (a bare YAML ``off`` arrives as False), ``ground_geoms`` that is not fitted, all or a non-empty list of names,
    ``ground_geom_groups`` that is not a list of integers >= 0, ``ground_track`` that is not a list of at most 32 distinct names, a
    ``ground_z`` that is not a finite number, a ``ground_permille`` outside 1 .. 1000 and a ``ground_contact`` that is not a finite
    number >= 0, and a ``ground_floor_z`` (the floor that a ``level`` run records in the config its result file stores; it is written,
    never read) that is not a finite number or comes without ``level``.  Whether the names exist is for ``ground.ground_table``, which knows the model."""
    mode = _switch(stac, "ground")
    if not isinstance(mode, str) or mode not in GROUND_MODES:
        raise ConfigError(f"stac.ground must be off, report or level, not {mode!r}")
    get = lambda key: GROUND_DEFAULTS[key] if stac.get(key) is None else stac.get(key)  # noqa: E731
    geoms = get("ground_geoms")
    if not (isinstance(geoms, str) and geoms in ("fitted", "all")):
        if isinstance(geoms, str) or not geoms:
            raise ConfigError(f"stac.ground_geoms must be fitted, all or a list of geom or body names, not {geoms!r}")
        geoms = _name_list(geoms, "stac.ground_geoms")
    groups = stac.get("ground_geom_groups")
    if groups is not None:
        if not isinstance(groups, (list, tuple)) or not groups or any(isinstance(g, bool) or not isinstance(g, int) or g < 0 for g in groups):
            raise ConfigError(f"stac.ground_geom_groups must be a list of geom groups (integers >= 0), not {groups!r}")
        groups = [int(g) for g in groups]
    track = _name_list(get("ground_track"), "stac.ground_track")
    if len(track) > GROUND_MAX_TRACK or len(set(track)) != len(track):
        raise ConfigError(f"stac.ground_track must be a list of at most {GROUND_MAX_TRACK} distinct body names, not {track!r}")
    z = get("ground_z")
    if isinstance(z, bool) or not isinstance(z, (int, float)) or not math.isfinite(z):
        raise ConfigError(f"stac.ground_z must be a finite number, not {z!r}")
    permille = checked_int(get("ground_permille"), "stac.ground_permille", ConfigError, 1, 1000)
    contact = checked_number(get("ground_contact"), "stac.ground_contact", ConfigError)
    floor = stac.get("ground_floor_z")  # (written by a level run into the config that its result file stores; never read back)
    if floor is not None:
        if isinstance(floor, bool) or not isinstance(floor, (int, float)) or not math.isfinite(floor):
            raise ConfigError(f"stac.ground_floor_z must be a finite number, not {floor!r}")
        if mode != "level":
            raise ConfigError(f"stac.ground_floor_z = {floor!r} is what a run with stac.ground = level records in its result file: it goes with level only")
    return {"mode": mode, "geoms": geoms, "geom_groups": groups, "track": track, "z_ref": float(z), "permille": permille, "contact": contact}


REPORT_DEFAULTS = {"report_quantiles": (500, 900, 990), "report_worst": 10}
REPORT_MAX_QUANTILES = 8  # csrc/stac_report.hpp: kReportMaxQuant


def report_options(stac) -> tuple:
    """``stac.report`` and its two parameters out of a ``stac`` mapping -> (on, permille values, worst), absent keys at their
    defaults.  ``ConfigError`` for anything else than off | on (or the bool that a bare YAML off / on arrives as), for
    ``report_quantiles`` that is not a list of 1 .. 8 integers in 0 .. 1000, or a ``report_worst`` that is not an integer >= 0."""
    mode = _switch(stac, "report")
    if not isinstance(mode, str) or mode not in ("off", "on"):
        raise ConfigError(f"stac.report must be off or on, not {mode!r}")
    q = stac.get("report_quantiles", REPORT_DEFAULTS["report_quantiles"])
    if not isinstance(q, (list, tuple)) or not 1 <= len(q) <= REPORT_MAX_QUANTILES:
        raise ConfigError(f"stac.report_quantiles must be a list of 1 .. {REPORT_MAX_QUANTILES} permille values, not {q!r}")
    for v in q:
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 1000:
            raise ConfigError(f"stac.report_quantiles holds permille values, integers in 0 .. 1000, not {v!r}")
    w = checked_int(stac.get("report_worst", REPORT_DEFAULTS["report_worst"]), "stac.report_worst", ConfigError, 0)
    return mode == "on", tuple(q), w


SMOOTH_DEFAULTS = {"smooth_window": 3, "smooth_order": 2}
SMOOTH_MAX_WINDOW = 16  # csrc/stac_smooth.hpp: kSmoothMaxHalf


def smooth_options(stac) -> dict:
    """``stac.smooth`` and its parameters out of a ``stac`` mapping -> ``{"kind", "half_window", "order", "sigma"}``, absent keys
    at their defaults (``order`` is None for gaussian, ``sigma`` for savgol; both for off).  ``ConfigError`` for anything else
    than off | savgol | gaussian (a bare YAML ``off`` arrives as False), a half-width that is not an integer in 1 .. 16, an order
    outside 0 .. 2 H, a sigma that is not a finite number > 0, and for smoothing without ``postprocess: gpu`` (there is no host
    path) or with ``reference_marker_order: true`` (the rows of marker_sites must be the rows of qpos)."""
    kind = _switch(stac, "smooth")
    if not isinstance(kind, str) or kind not in ("off", "savgol", "gaussian"):
        raise ConfigError(f"stac.smooth must be off, savgol or gaussian, not {kind!r}")
    h = checked_int(stac.get("smooth_window", SMOOTH_DEFAULTS["smooth_window"]), "stac.smooth_window (the half-width in frames)",
                    ConfigError, 1, SMOOTH_MAX_WINDOW)
    # (the order is held to the window for savgol only: gaussian does not read it)
    order = checked_int(stac.get("smooth_order", SMOOTH_DEFAULTS["smooth_order"]), "stac.smooth_order", ConfigError, 0,
                        2 * h if kind == "savgol" else None, f"an integer with 0 <= order < {2 * h + 1} (the window)")
    sigma = checked_number(stac.get("smooth_sigma", h / 2.0), "stac.smooth_sigma (in frames)", ConfigError, positive=True)
    if kind != "off":
        if stac.get("postprocess", "host") != "gpu":
            raise ConfigError(f"stac.smooth = {kind} runs on the device only (there is no host path for smoothing): set stac.postprocess to gpu as well")
        if bool(stac.get("reference_marker_order", False)):
            raise ConfigError(smooth_marker_order_refusal(kind))
    return {"kind": kind, "half_window": h, "order": order if kind == "savgol" else None, "sigma": sigma if kind == "gaussian" else None}


RESAMPLE_DEFAULTS = {"resample_lobes": 10, "resample_beta": 5.0}
RESAMPLE_MAX_LOBES = 16  # post.RESAMPLE_MAX_LOBES
RESAMPLE_MAX_UP, RESAMPLE_MAX_DOWN, RESAMPLE_MAX_WIN = 32, 64, 256  # csrc/stac_resample.hpp: kResampleMaxUp, kResampleMaxDown, kResampleMaxWin
# the one text of run_stac's pre-flight for a run whose ik_only output is sharded
RESAMPLE_SHARDED = ("stac.resample = kaiser resamples the whole ik_only result on rank 0, but this run writes per-rank shards "
                    "(stac.gather resolves to none): use gather = rank0, or call Stac.resample_result on the manifest afterwards")


def resample_ratio(from_hz, to_hz, exc=ConfigError, names=("stac.mocap_hz", "stac.resample_hz")) -> tuple:
    """``to_hz / from_hz`` in lowest terms -> (U, D), read through the decimal text of the two numbers so that 29.97 is exact.
    ``exc`` for a rate that is not a finite number > 0 and for U > 32 or D > 64."""
    from fractions import Fraction

    for name, v in zip(names, (from_hz, to_hz)):
        checked_number(v, name, exc, positive=True)
    ratio = Fraction(str(to_hz)) / Fraction(str(from_hz))
    if ratio.numerator > RESAMPLE_MAX_UP or ratio.denominator > RESAMPLE_MAX_DOWN:
        raise exc(f"{names[1]} / {names[0].split(': ')[-1]} = {to_hz!r} / {from_hz!r} is {ratio.numerator} / {ratio.denominator} in lowest terms; "
                  f"up to {RESAMPLE_MAX_UP} / {RESAMPLE_MAX_DOWN} can be resampled")
    return ratio.numerator, ratio.denominator


def resample_window(U, D, lobes) -> int:
    """Taps W of an output of the Kaiser table for U / D with ``lobes`` (post.resample_taps)."""
    return 2 * ((lobes * max(U, D)) // U + 1)


def resample_options(stac) -> dict:
    """``stac.resample`` and its parameters out of a ``stac`` mapping -> ``{"kind", "from_hz", "to_hz", "up", "down", "lobes",
    "beta"}``, absent keys at their defaults (the rates and the ratio are None for off).  ``ConfigError`` for anything else than
    off | kaiser (a bare YAML ``off`` arrives as False), ``resample_lobes`` that is not an integer in 1 .. 16, a
    ``resample_beta`` that is not a finite number >= 0, a rate (when given) that is not a finite number > 0, and with kaiser for a
    missing rate, a ratio beyond 32 / 64, a window of more than 256 taps, and for resampling without ``postprocess: gpu`` (there
    is no host path) or with ``reference_marker_order: true`` (the rows of marker_sites must be the rows of qpos)."""
    kind = _switch(stac, "resample")
    if not isinstance(kind, str) or kind not in ("off", "kaiser"):
        raise ConfigError(f"stac.resample must be off or kaiser, not {kind!r}")
    lobes = checked_int(stac.get("resample_lobes", RESAMPLE_DEFAULTS["resample_lobes"]), "stac.resample_lobes", ConfigError, 1, RESAMPLE_MAX_LOBES)
    beta = checked_number(stac.get("resample_beta", RESAMPLE_DEFAULTS["resample_beta"]), "stac.resample_beta", ConfigError)
    rates = {}
    for key in ("mocap_hz", "resample_hz"):
        rates[key] = stac.get(key)
        if rates[key] is not None:
            checked_number(rates[key], f"stac.{key}", ConfigError, positive=True)
    up = down = None
    if kind != "off":
        for key in ("mocap_hz", "resample_hz"):
            if rates[key] is None:
                raise ConfigError(f"stac.resample = {kind} needs stac.{key}: the rate of the recording (mocap_hz) and the rate wanted (resample_hz)")
        up, down = resample_ratio(rates["mocap_hz"], rates["resample_hz"])
        if resample_window(up, down, lobes) > RESAMPLE_MAX_WIN:
            raise ConfigError(f"stac.resample_lobes = {lobes} at {up} / {down} needs {resample_window(up, down, lobes)} taps per output, "
                              f"at most {RESAMPLE_MAX_WIN}: fewer lobes")
        if stac.get("postprocess", "host") != "gpu":
            raise ConfigError(f"stac.resample = {kind} runs on the device only (there is no host path for resampling): set stac.postprocess to gpu as well")
        if bool(stac.get("reference_marker_order", False)):
            raise ConfigError(f"stac.resample = {kind} recomputes marker_sites from the resampled qpos row by row, which the reference's "
                              "frame-major row order of marker_sites (stac.reference_marker_order: true) cannot hold")
    return {"kind": kind, "from_hz": rates["mocap_hz"], "to_hz": rates["resample_hz"], "up": up, "down": down, "lobes": lobes, "beta": beta}


# Refusals that both run_stac (before any work) and Stac.ik_only (for its direct callers) raise: one text each
GATHER_NONE_CONTINUOUS = ("stac.gather = none writes per-rank shards, but stac.continuous cross-fades neighbouring "
                          "clips across shard borders: use gather = rank0 (or all, or auto) for continuous runs")
POSTPROCESS_GPU_MARKER_ORDER = ("stac.postprocess = gpu cannot cross-fade marker_sites in the reference's frame-major row order "
                                "(stac.reference_marker_order: true): only postprocess = host reproduces fading across it")


def smooth_marker_order_refusal(kind) -> str:
    return (f"stac.smooth = {kind} recomputes marker_sites from the smoothed qpos row by row, which the reference's "
            "frame-major row order of marker_sites (stac.reference_marker_order: true) cannot hold")


class ConfigNode(dict):
    """dict with attribute access and OmegaConf-like ``get``/``in`` behaviour."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def to_dict(self) -> dict:
        def conv(v):
            if isinstance(v, ConfigNode):
                return {k: conv(x) for k, x in v.items()}
            if isinstance(v, list):
                return [conv(x) for x in v]
            return v

        return conv(self)

    def to_yaml(self) -> str:
        return yaml.safe_dump(self.to_dict(), sort_keys=False)


def _wrap(v: Any) -> Any:
    if isinstance(v, dict):
        return ConfigNode({k: _wrap(x) for k, x in v.items()})
    if isinstance(v, list):
        return [_wrap(x) for x in v]
    return v


def _load_yaml(path: Path) -> dict:
    with open(path, "r") as fh:
        return yaml.safe_load(fh) or {}


def _parse_scalar(text: str) -> Any:
    try:
        return yaml.safe_load(text)
    except yaml.YAMLError:
        return text


def compose_config(
    config_path: Path | str,
    config_name: str = "config",
    overrides: Iterable[str] | None = None,
) -> ConfigNode:
    """Compose ``<config_path>/<config_name>.yaml`` like ``stac_mjx.config.compose_config`` (config.py:73-88)."""
    config_dir = Path(config_path).resolve()
    top_path = config_dir / f"{config_name}.yaml"
    if not top_path.exists():
        raise ConfigError(f"config file not found: {top_path}")
    top = _load_yaml(top_path)
    overrides = list(overrides or [])

    group_choice: dict[str, str] = {}
    for item in top.pop("defaults", []) or []:
        if isinstance(item, dict):
            for g, name in item.items():
                group_choice[str(g)] = str(name)
        elif item != "_self_":
            raise ConfigError(f"unsupported defaults entry: {item!r}")
    dotted: list[tuple[str, Any]] = []
    for ov in overrides:
        if ov.startswith("hydra/") or ov.startswith("hydra."):
            continue  # hydra logging switches the reference adds (config.py:80)
        if "=" not in ov:
            raise ConfigError(f"override must be key=value: {ov!r}")
        key, val = ov.split("=", 1)
        key = key.lstrip("+")
        if "." not in key and key in ("stac", "model"):
            group_choice[key] = val
        else:
            dotted.append((key, _parse_scalar(val)))

    cfg: dict[str, Any] = {}
    for group, name in group_choice.items():
        gpath = config_dir / group / f"{name}.yaml"
        if not gpath.exists():
            raise ConfigError(f"config group file not found: {gpath}")
        cfg[group] = _load_yaml(gpath)
    for k, v in top.items():  # _self_ comes last in the reference's defaults lists
        if isinstance(v, dict) and isinstance(cfg.get(k), dict):
            cfg[k].update(v)
        else:
            cfg[k] = v
    for key, val in dotted:
        node = cfg
        parts = key.split(".")
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        node[parts[-1]] = val
    return validate_config(cfg)


def validate_config(cfg: dict) -> ConfigNode:
    """Schema check equivalent to the OmegaConf structured merge (config.py:86-88)."""
    if "model" not in cfg or "stac" not in cfg:
        raise ConfigError("config must define both 'model' and 'stac' groups")
    model = dict(_MODEL_DEFAULTS)
    model.update(cfg["model"])
    stac = dict(cfg["stac"])
    missing = [k for k in _MODEL_REQUIRED if k not in model]
    # the reference tolerates absent optional model keys only where it probes with `in`/get
    # (ROOT_OPTIMIZATION_KEYPOINT, INDIVIDUAL_PART_OPTIMIZATION, SITES_TO_REGULARIZE: stac.py:122,174,229)
    soft = {"ROOT_OPTIMIZATION_KEYPOINT", "INDIVIDUAL_PART_OPTIMIZATION", "SITES_TO_REGULARIZE",
            "KEYPOINT_COLOR_PAIRS", "RENDER_FPS", "ROOT_FTOL", "LIMB_FTOL", "KP_NAMES"}  # fmt: skip
    hard_missing = [k for k in missing if k not in soft]
    if hard_missing:
        raise ConfigError(f"model config is missing keys: {hard_missing}")
    unknown = [k for k in model if k not in _MODEL_REQUIRED and k not in _MODEL_DEFAULTS and k not in _MODEL_EXTENSIONS]
    if unknown:
        raise ConfigError(f"model config has keys outside the schema: {unknown}")
    missing = [k for k in _STAC_REQUIRED if k not in stac]
    if missing:
        raise ConfigError(f"stac config is missing keys: {missing}")
    unknown = [k for k in stac if k not in _STAC_REQUIRED and k not in _STAC_OPTIONAL and k not in _STAC_EXTENSIONS]
    if unknown:
        raise ConfigError(f"stac config has keys outside the schema: {unknown}")
    missing = [k for k in _MUJOCO_REQUIRED if k not in stac["mujoco"]]
    if missing:
        raise ConfigError(f"stac.mujoco config is missing keys: {missing}")
    # light type coercion like OmegaConf's structured merge
    for k in ("FTOL", "SCALE_FACTOR", "MOCAP_SCALE_FACTOR", "M_REG_COEF", "MARKER_SIZE"):
        model[k] = float(model[k])
    for k in ("N_ITERS", "N_ITER_Q", "N_SAMPLE_FRAMES"):
        model[k] = int(model[k])
    for k in ("n_fit_frames", "n_frames_per_clip"):
        stac[k] = int(stac[k])
    for k in ("skip_fit_offsets", "skip_ik_only", "infer_qvels", "continuous"):
        if not isinstance(stac[k], bool):
            raise ConfigError(f"stac.{k} must be a bool")
    postprocess_options(stac)
    for key, options in (("fill_missing", fill_missing_options), ("reject_outliers", outlier_options), ("report", report_options),
                         ("smooth", smooth_options), ("reject_pairwise", pairwise_options), ("repair_swaps", swaps_options),
                         ("fill_donors", donor_options), ("resample", resample_options), ("offset_mask", offset_mask_options)):
        if isinstance(stac.get(key), bool):  # the file that is written with a result says off / on, not the boolean
            stac[key] = _switch(stac, key)
        options(stac)
    fit_frames_options(stac)
    if isinstance(stac.get("seam_report"), bool):  # (as above: the stored file says off / on)
        stac["seam_report"] = "on" if stac["seam_report"] else "off"
    seam_options(stac)
    if isinstance(stac.get("ground"), bool):
        stac["ground"] = _switch(stac, "ground")
    ground_options(stac)
    return _wrap({"model": model, "stac": stac})


def load_configs(config_dir: Path | str, config_name: str = "config") -> ConfigNode:
    """Same signature as ``stac_mjx.main.load_configs`` (main.py:18-30)."""
    return compose_config(config_dir, config_name=config_name)
