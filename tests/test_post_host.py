"""Post-processing on the GPU, the parts that need no GPU: argument checks of the three entry points (they happen before the
device is touched), the ``stac.postprocess`` config key, and a CPU build of the kernels' arithmetic (csrc/stac_post.hpp) against
``utils.handle_edge_effects`` / ``utils.compute_velocity_from_kinematics`` on the cases of tests/test_gpu_post.py."""

import ctypes as C

import numpy as np
import pytest

import post_cases as pc
import host_scaffold as hs


@pytest.fixture(scope="module")
def lib():
    return hs.loaded_library()


def test_stitch_rows_formula(lib):
    for Cn, F in pc.STITCH_CF:
        assert lib.stac_post_stitch_rows(Cn, F, pc.OV) == pc.stitch_rows(Cn, F)
        if Cn >= 2 and F >= pc.OV:
            assert lib.stac_post_stitch_rows(Cn, F, pc.OV) == Cn * F
    assert lib.stac_post_stitch_rows(0, 5, 10) == 0
    assert lib.stac_post_stitch_rows(4, 7, 1) == 4 * 7 and lib.stac_post_stitch_rows(3, 40, 32) == 3 * 40
    for bad in ((3, 0, 10), (3, 5, 0), (3, 5, 33), (-1, 5, 10)):
        hs.invalid(lib, lib.stac_post_stitch_rows(*bad))


def test_stitch_argument_errors_need_no_device(lib):
    """Every pointer below is a fake non-NULL address: a call that got past its checks would fault, not return."""
    m = (C.c_double * 32)(*([0.5] * 32))
    src, dst = C.c_void_p(0x1000), C.c_void_p(0x2000)
    R = pc.stitch_rows(3, 12)
    call = lambda src=src, Cn=3, F=12, ov=10, D=7, m=m, dst=dst, rows=R: lib.stac_post_stitch(src, Cn, F, ov, D, m, dst, rows, None)
    hs.invalid(lib, call(F=0))
    hs.invalid(lib, call(ov=0, rows=3 * 12))
    hs.invalid(lib, call(ov=33, rows=3 * 12))
    hs.invalid(lib, call(D=0))
    hs.invalid(lib, call(Cn=-1))
    assert "36" in hs.invalid(lib, call(rows=R + 1))  # the message names the row count it expected
    hs.invalid(lib, call(src=None))
    hs.invalid(lib, call(dst=None))
    hs.invalid(lib, call(m=None))
    assert call(Cn=0, rows=0, src=None, dst=None, m=None) == 0  # nothing to do
    hs.invalid(lib, call(Cn=0, rows=1))


def test_qvel_argument_errors_need_no_device(lib):
    q, v = C.c_void_p(0x1000), C.c_void_p(0x2000)
    call = lambda q=q, N=12, nq=74, F=4, dt=0.02, fj=1, mx=20.0, v=v: lib.stac_post_qvel(q, N, nq, F, dt, fj, mx, v, None)
    hs.invalid(lib, call(F=0))
    assert "13" in hs.invalid(lib, call(N=13))  # N % F != 0
    hs.invalid(lib, call(nq=6))           # a free joint needs 7
    hs.invalid(lib, call(nq=0, fj=0))
    hs.invalid(lib, call(dt=0.0))
    hs.invalid(lib, call(N=-4))
    hs.invalid(lib, call(q=None))
    hs.invalid(lib, call(v=None))
    assert call(N=0, q=None, v=None) == 0  # nothing to do
    assert call(N=0, nq=6, fj=0, q=None, v=None) == 0


def test_python_wrappers_refuse_host_tensors():
    import torch

    from stac_mjx_amd import post

    with pytest.raises(ValueError):
        post.stitch(torch.zeros(2, 14, 3), 4)
    with pytest.raises(ValueError):
        post.infer_qvel(torch.zeros(8, 7), 4, 0.02, True)
    x = np.linspace(0.0, 1.0, 10)
    np.testing.assert_array_equal(post.crossfade_mask(10), 0.5 * (1.0 + np.tanh(10.0 * (x - 0.5) / 2.0)))


def test_config_postprocess_key(rodent_cfg):
    from stac_mjx_amd.config import ConfigError, validate_config
    from stac_mjx_amd.main import _postprocess_mode

    def cfg(**over):
        stac = dict(fit_offsets_path="fit.h5", ik_only_path="ik.h5", data_path="d.mat", continuous=False, n_fit_frames=4,
                    skip_fit_offsets=False, skip_ik_only=False, infer_qvels=False, n_frames_per_clip=2,
                    mujoco=dict(solver="newton", iterations=1, ls_iterations=4))
        stac.update(over)
        return validate_config({"model": dict(rodent_cfg), "stac": stac})

    assert _postprocess_mode(cfg()) == "host"
    assert _postprocess_mode(cfg(postprocess="host")) == "host" and _postprocess_mode(cfg(postprocess="gpu")) == "gpu"
    for bad in ("cpu", "GPU", True, 1, ""):
        with pytest.raises(ConfigError):
            cfg(postprocess=bad)


# ---- a CPU build of the kernels' per-element functions ---------------------------------------------------------------------------
_DRIVER = r"""
#include "stac_post.hpp"
using namespace stac;
extern "C" void host_stitch(const float *src, int64_t C, int32_t F, int32_t ov, int32_t D, const double *m, float *dst, int64_t R) {
    const int64_t W = (int64_t)F + ov;
    for (int64_t r = 0; r < R; ++r) {
        int64_t c;
        int32_t t;
        const bool fade = post_stitch_source(r, C, F, ov, &c, &t);
        const float *a = src + (c * W + t) * D;
        const float *b = src + ((c + 1) * W + (t - F)) * D;
        for (int32_t j = 0; j < D; ++j) dst[r * D + j] = fade ? post_fade(a[j], b[j], m[t - F]) : a[j];
    }
}
extern "C" int64_t host_stitch_rows(int64_t C, int32_t F, int32_t ov) { return post_stitch_rows(C, F, ov); }
extern "C" void host_qvel(const float *qpos, int64_t N, int32_t nq, int32_t F, int32_t freejoint, double dt, double max_qvel, float *qvel) {
    const int32_t nv = nq - (freejoint ? 1 : 0);
    for (int64_t r = 0; r < N; ++r)
        for (int32_t j = 0; j < nv; ++j)
            qvel[r * nv + j] = post_qvel_elem(qpos + r * nq, qpos + post_qvel_next(r, F) * nq, j, freejoint, (float)dt, (float)max_qvel);
}
"""


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    h = hs.build_cpu_library(tmp_path_factory, "post", _DRIVER)
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    h.host_stitch.argtypes = [fp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, dp, fp, C.c_int64]
    h.host_stitch.restype = None
    h.host_stitch_rows.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    h.host_stitch_rows.restype = C.c_int64
    h.host_qvel.argtypes = [fp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, fp]
    h.host_qvel.restype = None
    return h


def _cpu_stitch(h, x, F):
    from stac_mjx_amd.post import crossfade_mask

    Cn, D = x.shape[0], int(np.prod(x.shape[2:]))
    R = int(h.host_stitch_rows(Cn, F, pc.OV))
    m = np.ascontiguousarray(crossfade_mask(pc.OV))
    out = np.full((R,) + x.shape[2:], -12345.0, np.float32)
    h.host_stitch(hs.fp(x), Cn, F, pc.OV, D, m.ctypes.data_as(C.POINTER(C.c_double)), hs.fp(out), R)
    return out


@pytest.mark.parametrize("trailing", pc.STITCH_TRAILING, ids=str)
def test_cpu_build_stitch_equals_handle_edge_effects(hostlib, trailing):
    for Cn, F in pc.STITCH_CF:
        x = pc.stitch_input(Cn, F, trailing)
        want = pc.host_stitch(x, F)
        assert want.shape[0] == pc.stitch_rows(Cn, F)
        np.testing.assert_array_equal(_cpu_stitch(hostlib, x, F), want, err_msg=f"C={Cn} F={F}")


def test_cpu_build_stitch_many_rows(hostlib):
    Cn, F, trailing = pc.STITCH_BIG
    x = pc.stitch_input(Cn, F, trailing)
    np.testing.assert_array_equal(_cpu_stitch(hostlib, x, F), pc.host_stitch(x, F))


@pytest.mark.parametrize("freejoint,nq", pc.QVEL_NQ)
@pytest.mark.parametrize("dt", pc.QVEL_DT, ids=lambda d: f"dt{d:.4g}")
def test_cpu_build_qvel_equals_compute_velocity_from_kinematics(hostlib, freejoint, nq, dt):
    differ = total = 0
    for F, Cn in pc.QVEL_FC:
        q = pc.qvel_input(F, Cn, nq, freejoint, dt)
        if freejoint:
            pc.assert_host_gyro_is_meaningful(q, F)
        want = pc.host_qvel(q, F, dt, freejoint)
        got = np.full_like(want, -12345.0)
        hostlib.host_qvel(hs.fp(q), q.shape[0], nq, F, int(freejoint), dt, pc.MAX_QVEL, hs.fp(got))
        a, b = pc.check_qvel(got, want, freejoint, label=f"F={F} C={Cn} nq={nq} dt={dt:.4g}")
        differ, total = differ + a, total + b
        if freejoint and F >= 7:
            # the cases hold what they are meant to: both branches of the gyro, an unclipped gyro above max_qvel, clipped joints
            gy = want[:, 3:6]
            assert np.any(np.all(gy == 0, axis=1)[np.arange(len(gy)) % F != F - 1]) and np.any(gy != 0)
            if dt < 1.0:
                assert np.nanmax(np.abs(gy)) > pc.MAX_QVEL
        if nq - (7 if freejoint else 0) > 0 and F >= 7:
            j = want[:, 6:] if freejoint else want
            assert np.any(j == pc.MAX_QVEL) and np.any(j == -pc.MAX_QVEL)
    print(f"nq={nq} dt={dt:.4g}: {differ} of {total} gyro values differ from the host's in the last bits")
