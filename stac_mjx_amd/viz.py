"""``viz_stac``: render a result file (``stac_mjx/viz.py:10-61``) with the GPU renderer of ``Stac.render``."""

from __future__ import annotations

from pathlib import Path

from . import io


def viz_stac(data_path, n_frames: int, save_path, start_frame: int = 0, camera=0, height: int = 1200, width: int = 1920,
             base_path: Path | None = None, show_marker_error: bool = False, *, geom_groups=None, encoder=None,
             return_frames=None):
    """Render forward kinematics from STAC output data; returns (config, list of rendered RGB frames).  ``geom_groups``: the
    geom groups to draw (None = the reference's rule, groups 0 and 2).  ``encoder`` ("pil" / "gpu") and ``return_frames``:
    see ``Stac.render``; None = its defaults."""
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
    return cfg, stac.render(d.qpos, d.kp_data, d.offsets, n_frames, save_path, start_frame, camera, height, width,
                            show_marker_error, **kw)
