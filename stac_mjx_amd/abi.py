"""The C ABI of ``libstac_hip.so`` (``include/stac_hip.h``) as ctypes sees it: the five structures, ONE table of the 39
prototypes in the header's order, ``declare`` that applies the table to a loaded library (``engine.load_library`` does, to whatever
it loads), and the few helpers every caller of the library shares.  ``tests/test_host.py`` holds the table against the header and
the structures against the compiler.
"""

from __future__ import annotations

import ctypes as C

import torch

_i32p = C.POINTER(C.c_int32)
_f32p = C.POINTER(C.c_float)
_u8p = C.POINTER(C.c_uint8)


class StacModelTables(C.Structure):
    _fields_ = [
        ("nbody", C.c_int32), ("njnt", C.c_int32), ("nq", C.c_int32), ("nsite", C.c_int32),
        ("body_parentid", _i32p), ("body_pos", _f32p), ("body_quat", _f32p),
        ("body_jntadr", _i32p), ("body_jntnum", _i32p),
        ("jnt_type", _i32p), ("jnt_qposadr", _i32p), ("jnt_bodyid", _i32p),
        ("jnt_pos", _f32p), ("jnt_axis", _f32p), ("qpos0", _f32p),
        ("site_bodyid", _i32p), ("site_pos", _f32p), ("lb", _f32p), ("ub", _f32p),
    ]  # fmt: skip


class StacQParams(C.Structure):
    _fields_ = [("tol", C.c_float), ("maxiter", C.c_int32), ("maxls", C.c_int32), ("lanes_per_chain", C.c_int32),
                ("solver", C.c_int32), ("lm_lambda0", C.c_float)]


class StacRenderTables(C.Structure):
    _fields_ = [
        ("nprim", C.c_int32), ("prim_type", _i32p), ("prim_body", _i32p), ("prim_flags", _i32p),
        ("prim_size", _f32p), ("prim_pos", _f32p), ("prim_quat", _f32p), ("prim_rgba", _f32p), ("prim_rgb2", _f32p),
        ("prim_texrepeat", _f32p), ("nkp", C.c_int32), ("kp_rgba", _f32p),
        ("marker_rgba", C.c_float * 4), ("segment_rgba", C.c_float * 4), ("marker_radius", C.c_float),
        ("segment_radius", C.c_float), ("nlight", C.c_int32), ("light_dir", _f32p), ("light_diffuse", _f32p),
        ("head_ambient", C.c_float * 3), ("head_diffuse", C.c_float * 3), ("alpha", C.c_float), ("background", C.c_float * 3),
    ]  # fmt: skip


class StacRenderMeshes(C.Structure):
    _fields_ = [
        ("nmesh", C.c_int32), ("node_offset", _i32p), ("tri_offset", _i32p), ("node_box", _f32p), ("node_link", _i32p),
        ("tri_vertex", _f32p), ("prim_mesh", _i32p),
    ]  # fmt: skip


class StacReportParams(C.Structure):
    _fields_ = [("markers", C.c_void_p), ("kp", C.c_void_p), ("gap", C.c_void_p), ("n_frames", C.c_int64), ("n_kp", C.c_int32),
                ("n_quant", C.c_int32), ("permille", _i32p), ("sqerr", C.c_void_p), ("frame_sse", C.c_void_p),
                ("frame_n", C.c_void_p), ("count", C.c_void_p), ("sum", C.c_void_p), ("max", C.c_void_p), ("argmax", C.c_void_p),
                ("hist", C.c_void_p), ("quant", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("stream", C.c_void_p)]


# the ctypes structures by the name of their typedef in the header
STRUCTS = {"stac_model_tables": StacModelTables, "stac_q_params": StacQParams, "stac_render_tables": StacRenderTables,
           "stac_render_meshes": StacRenderMeshes, "stac_report_params": StacReportParams}

vp, i32, i64, f32, f64, P = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double, C.POINTER
# every function include/stac_hip.h declares: name -> (restype, argtypes); None is the restype of a void function
PROTOTYPES = {
    "stac_last_error": (C.c_char_p, []),
    "stac_last_error_code": (i32, []),
    "stac_abi_version": (i32, []),
    "stac_device_count": (i32, []),
    "stac_model_create": (vp, [P(StacModelTables)]),
    "stac_model_destroy": (None, [vp]),
    "stac_model_info": (i32, [vp, _i32p]),
    "stac_set_site_pos": (i32, [vp, vp, vp]),
    "stac_get_site_pos": (i32, [vp, vp, vp]),
    "stac_fk": (i32, [vp, vp, i32, vp, vp, vp, vp, vp]),
    "stac_q_solve": (i32, [vp, P(StacQParams), vp, vp, _u8p, _u8p, _f32p, _f32p, i32, vp, vp, vp, vp]),
    "stac_q_phase": (i32, [vp, P(StacQParams), vp, vp, _u8p, _u8p, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "stac_m_phase_workspace_floats": (i64, [vp, i32]),
    "stac_m_phase_partial": (i32, [vp, vp, vp, i32, vp, vp, vp]),
    "stac_m_phase_finish": (i32, [vp, vp, vp, vp, f32, vp, vp, vp]),
    "stac_render_scene_create": (vp, [vp, P(StacRenderTables)]),
    "stac_render_scene_destroy": (None, [vp]),
    "stac_render_scene_create_with_meshes": (vp, [vp, P(StacRenderTables), P(StacRenderMeshes)]),
    "stac_render": (i32, [vp, i32, vp, vp, vp, vp, i32, vp, f32, i32, i32, vp, vp, vp, vp]),
    "stac_jpeg_header": (i64, [i32, i32, i32, i32, vp, i64]),
    "stac_jpeg_workspace_bytes": (i64, [i64, i32, i32, i32]),
    "stac_jpeg_encode": (i32, [i64, i32, i32, i32, i32, vp, vp, i64, vp, vp, i64, vp]),
    "stac_post_stitch_rows": (i64, [i64, i32, i32]),
    "stac_post_stitch": (i32, [vp, i64, i32, i32, i32, P(f64), vp, i64, vp]),
    "stac_post_qvel": (i32, [vp, i64, i32, i32, f64, i32, f64, vp, vp]),
    "stac_post_smooth": (i32, [vp, i64, i32, i32, i32, _f32p, _i32p, i32, vp, vp, vp, vp]),
    "stac_post_resample_rows": (i64, [i64, i32, i32]),
    # the tap table of stac_post_resample is DEVICE memory, its quat_cols are HOST memory: an int32 pointer, not a device address
    "stac_post_resample": (i32, [vp, i64, i32, i64, i32, i32, i32, vp, _i32p, i32, vp, vp, vp, i64, vp]),
    "stac_prep_fill_workspace": (i64, [i64, i32]),
    "stac_prep_fill": (i32, [vp, i64, i32, i32, vp, vp, vp, i64, vp]),
    "stac_prep_reject": (i32, [vp, i64, i32, i32, f64, f64, vp, vp, vp]),
    "stac_prep_pairwise_workspace": (i64, [i64, i32]),
    "stac_prep_pairwise": (i32, [vp, i64, i32, f64, f64, i32, vp, vp, vp, vp, vp, vp, i64, vp]),
    "stac_prep_swaps_workspace": (i64, [i64, i32]),
    # the candidate table of stac_prep_swaps is HOST memory: an int32 pointer, not a device address
    "stac_prep_swaps": (i32, [vp, i64, i32, _i32p, i32, f64, f64, i32, vp, vp, vp, vp, vp, vp, i64, vp]),
    "stac_prep_donor_workspace": (i64, [i64, i32]),
    # the donor table of stac_prep_donor is DEVICE memory
    "stac_prep_donor": (i32, [vp, i64, i32, vp, i32, vp, vp, vp, vp, i64, vp]),
    "stac_report_workspace": (i64, [i64, i32, i32]),
    "stac_report_errors": (i32, [P(StacReportParams)]),
}  # fmt: skip
ABI_SYMBOLS = tuple(PROTOTYPES)
# every function csrc/select/stac_select.h declares (libstac_select.so, the companion library of stac.fit_frames), in its order
SELECT_PROTOTYPES = {
    "stac_select_last_error": (C.c_char_p, []),
    "stac_select_last_error_code": (i32, []),
    "stac_select_workspace": (i64, [i64, i32]),
    "stac_select_diverse": (i32, [vp, i64, i32, vp, i64, vp, vp, vp, vp, i64, vp]),
}
# every function csrc/mmask/stac_mmask.h declares (libstac_mmask.so, the companion library of stac.offset_mask), in its order
MMASK_PROTOTYPES = {
    "stac_mmask_last_error": (C.c_char_p, []),
    "stac_mmask_last_error_code": (i32, []),
    "stac_mmask_workspace": (i64, [i64, i32]),
    "stac_mmask_partial": (i32, [vp, vp, vp, i32, vp, vp, i64, i32, vp, i64, vp, vp]),
    "stac_mmask_finish": (i32, [vp, i32, vp, vp, f32, vp, vp, vp, vp]),
}
# every function csrc/seam/stac_seam.h declares (libstac_seam.so, the companion library of stac.seam_report), in its order; the
# quat_cols of stac_seam_steps are HOST memory: an int32 pointer, not a device address
SEAM_PROTOTYPES = {
    "stac_seam_last_error": (C.c_char_p, []),
    "stac_seam_last_error_code": (i32, []),
    "stac_seam_steps": (i32, [vp, i64, i32, i64, _i32p, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
}
# every function csrc/ground/stac_ground.h declares (libstac_ground.so, the companion library of stac.ground), in its order; the
# geom_meta_host of stac_ground_clearance is HOST memory: an int32 pointer, not a device address
GROUND_PROTOTYPES = {
    "stac_ground_last_error": (C.c_char_p, []),
    "stac_ground_last_error_code": (i32, []),
    "stac_ground_clearance": (i32, [vp, vp, i64, i32, _i32p, vp, vp, i32, vp, i32, i32, f32, vp, vp, vp, vp, vp, vp]),
}


class StacHipError(RuntimeError):
    pass


def declare(lib, prototypes=None):
    """Declares ``restype`` and ``argtypes`` of every function of the table (``prototypes`` None: ``PROTOTYPES``) on ``lib``
    (idempotent) -> ``lib``."""
    for name, (restype, argtypes) in (PROTOTYPES if prototypes is None else prototypes).items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def last_error(lib) -> str:
    return lib.stac_last_error().decode("utf-8", "replace")


def hip_error(lib, what, rc) -> StacHipError:
    """The exception for status ``rc`` of the call ``what`` (None: no prefix), with the library's last error text."""
    return StacHipError(f"{what + ': ' if what else ''}libstac_hip error {rc}: {last_error(lib)}")


def check(lib, what, rc):
    """``rc`` of an entry point, a status or a size: negative is an error (include/stac_hip.h), anything else is returned."""
    if rc < 0:
        raise hip_error(lib, what, rc)
    return rc


def _ptr(t: torch.Tensor | None):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream_ptr(device):
    """The current stream of ``device`` as the ``void *stream`` of an entry point."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def device_tensor(x, message: str, dtype=torch.float32) -> torch.Tensor:
    """A CUDA tensor as a contiguous one of ``dtype``; anything else is a ``ValueError`` with ``message``."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError(message)
    return x.to(dtype=dtype).contiguous()
