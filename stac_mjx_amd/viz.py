"""``viz_stac``: render a result file (``stac_mjx/viz.py:10-61``) with the GPU renderer of ``Stac.render``."""

from __future__ import annotations

from pathlib import Path

import numpy as np

from . import io


def viz_stac(data_path, n_frames: int, save_path, start_frame: int = 0, camera=0, height: int = 1200, width: int = 1920,
             base_path: Path | None = None, show_marker_error: bool = False, *, geom_groups=None, encoder=None,
             return_frames=None, show_filled: bool = False):
    """Render forward kinematics from STAC output data; returns (config, list of rendered RGB frames).  ``geom_groups``: the
    geom groups to draw (None = the reference's rule, groups 0 and 2).  ``encoder`` ("pil" / "gpu") and ``return_frames``:
    see ``Stac.render``; None = its defaults.

    A file written with ``stac.fill_missing`` carries ``kp_gap``: keypoints that were filled (``kp_gap > 0``) go to the renderer as
    NaN unless ``show_filled=True``, so by the render rule they draw neither their sphere nor their error segment -- a filled
    value is not shown as an observation.  (A host-side mask; a file without ``kp_gap`` renders as before.)"""
    from .stac import Stac

    cfg, d = io.load_stac_data(data_path)
    if base_path is None:
        base_path = Path.cwd()
    xml_path = Path(base_path) / cfg.model.MJCF_PATH
    stac = Stac(xml_path, cfg, d.kp_names)
    kw = {} if geom_groups is None else {"geom_groups": geom_groups}
    if encoder is not None:
        kw["encoder"] = encoder
    if return_frames is not None:
        kw["return_frames"] = return_frames
    gap = getattr(d, "kp_gap", None)  # (absent or empty: the file's kp_data goes to the renderer as it is)
    kp_data = d.kp_data if show_filled or gap is None else mask_filled(d.kp_data, gap)
    return cfg, stac.render(d.qpos, kp_data, d.offsets, n_frames, save_path, start_frame, camera, height, width,
                            show_marker_error, **kw)


def mask_filled(kp_data, kp_gap):
    """``kp_data`` [T, 3K] with the three coordinates of every filled keypoint (``kp_gap`` [T, K] > 0) set to NaN; ``kp_data`` itself
    when ``kp_gap`` is empty.  The rows must correspond (they do in every file ``run_stac`` writes)."""
    gap = np.asarray(kp_gap)
    if gap.size == 0 or not np.any(gap > 0):
        return kp_data
    kp_data = np.asarray(kp_data)
    if gap.ndim != 2 or kp_data.shape != (gap.shape[0], 3 * gap.shape[1]):
        raise ValueError(f"kp_gap {gap.shape} does not match kp_data {kp_data.shape}")
    out = np.array(kp_data, dtype=kp_data.dtype, copy=True)
    out.reshape(gap.shape[0], gap.shape[1], 3)[gap > 0] = np.nan
    return out
