"""Smoothing fitted poses (stac.smooth), the parts that need no GPU: the config keys and their refusals, the tap table against
scipy, the numpy restatement of the rule (tests/smooth_cases.py) against ``scipy.signal.savgol_filter`` and its properties, a CPU
build of the kernel's arithmetic (csrc/stac_smooth.hpp) against the restatement with tolerance 0, the argument checks of the
entry point (they happen before the device is touched) and the ``qpos_raw`` field of the result files."""

import ctypes as C

import numpy as np
import pytest

import smooth_cases as sc
import host_scaffold as hs

SAVGOL_CASES = [(1, 0), (1, 2), (2, 2), (3, 2), (3, 3), (5, 3), (16, 2), (16, 4)]


# ---- configuration ------------------------------------------------------------------------------------------------------------
def test_config_smooth_keys(rodent_cfg):
    from stac_mjx_amd.config import ConfigError, smooth_options
    from stac_mjx_amd.main import _smooth_mode

    assert smooth_options(hs.stage_cfg(rodent_cfg).stac) == {"kind": "off", "half_window": 3, "order": None, "sigma": None}
    assert _smooth_mode(hs.stage_cfg(rodent_cfg)) is None
    cfg = hs.stage_cfg(rodent_cfg, smooth=False)  # a bare `off` in YAML 1.1 is the boolean
    assert cfg.stac.smooth == "off" and _smooth_mode(cfg) is None
    assert _smooth_mode(hs.stage_cfg(rodent_cfg, smooth="off", postprocess="host", reference_marker_order=True)) is None  # off asks for nothing
    assert _smooth_mode(hs.stage_cfg(rodent_cfg, smooth="savgol", postprocess="gpu")) == {"kind": "savgol", "half_window": 3, "order": 2, "sigma": None}
    assert _smooth_mode(hs.stage_cfg(rodent_cfg, smooth="gaussian", postprocess="gpu", smooth_window=4)) == \
        {"kind": "gaussian", "half_window": 4, "order": None, "sigma": 2.0}
    assert _smooth_mode(hs.stage_cfg(rodent_cfg, smooth="gaussian", postprocess="gpu", smooth_sigma=1))["sigma"] == 1.0
    assert _smooth_mode(hs.stage_cfg(rodent_cfg, smooth="savgol", postprocess="gpu", smooth_window=16, smooth_order=32))["order"] == 32
    assert _smooth_mode(hs.stage_cfg(rodent_cfg, smooth="savgol", postprocess="gpu", smooth_window=1, smooth_order=0))["order"] == 0
    for bad in (dict(smooth="on"), dict(smooth=True), dict(smooth="SAVGOL"), dict(smooth=1),
                dict(smooth_window=0), dict(smooth_window=17), dict(smooth_window=3.0), dict(smooth_window=True),
                dict(smooth_order=-1), dict(smooth_order=1.0), dict(smooth_order=True),
                dict(smooth="savgol", postprocess="gpu", smooth_window=3, smooth_order=7),
                dict(smooth_sigma=0), dict(smooth_sigma=-1.0), dict(smooth_sigma=float("inf")), dict(smooth_sigma=float("nan")),
                dict(smooth_sigma="1"), dict(smooth_sigma=True)):
        with pytest.raises(ConfigError):
            hs.stage_cfg(rodent_cfg, **bad)
    # the two refused combinations, before any work is done (ValueError, like hampel without fill_missing)
    for kind in ("savgol", "gaussian"):
        with pytest.raises(ValueError, match="postprocess"):
            hs.stage_cfg(rodent_cfg, smooth=kind)
        with pytest.raises(ValueError, match="postprocess"):
            hs.stage_cfg(rodent_cfg, smooth=kind, postprocess="host")
        with pytest.raises(ValueError, match="reference_marker_order"):
            hs.stage_cfg(rodent_cfg, smooth=kind, postprocess="gpu", reference_marker_order=True)


def test_config_yaml_boolean_and_overrides(reference_dir):
    from stac_mjx_amd.config import ConfigError, compose_config

    base = reference_dir / "configs"
    assert compose_config(base, overrides=["stac.smooth=off"]).stac.smooth == "off"  # YAML parses the bare word to False
    cfg = compose_config(base, overrides=["stac.smooth=savgol", "stac.postprocess=gpu", "stac.smooth_window=5", "stac.smooth_order=3"])
    assert (cfg.stac.smooth, cfg.stac.smooth_window, cfg.stac.smooth_order) == ("savgol", 5, 3)
    with pytest.raises(ConfigError):
        compose_config(base, overrides=["stac.smooth=savgol"])


def test_run_stac_refuses_clips_shorter_than_the_window_before_any_work(rodent_cfg, tmp_path):
    """The lengths are known from the config alone: no Stac is built (there is no GPU here) and nothing is written."""
    from stac_mjx_amd.main import run_stac

    kp = np.zeros((24, 69), np.float32)
    names = list(rodent_cfg["KEYPOINT_MODEL_PAIRS"].keys())
    cfg = hs.stage_cfg(rodent_cfg, smooth="savgol", postprocess="gpu", smooth_window=3, n_frames_per_clip=6)
    with pytest.raises(ValueError, match=r"(?s)7.*6|6.*7"):  # names the window and the clip
        run_stac(cfg, kp, names, base_path=tmp_path)
    # continuous: the clip is the stitched run (24 rows of 2 windows of 12 + 10), shorter than a window of 33
    cfg = hs.stage_cfg(rodent_cfg, smooth="gaussian", postprocess="gpu", smooth_window=16, n_frames_per_clip=12, continuous=True)
    with pytest.raises(ValueError, match=r"(?s)33.*24|24.*33"):
        run_stac(cfg, kp, names, base_path=tmp_path)
    assert not list(tmp_path.iterdir())


# ---- the tap table --------------------------------------------------------------------------------------------------------------
def test_taps_shape_rounding_and_refusals():
    from stac_mjx_amd import post

    for H in range(1, 17):
        W = 2 * H + 1
        for kind, kw in (("savgol", {}), ("savgol", {"order": 0}), ("gaussian", {}), ("gaussian", {"sigma": 0.7})):
            t = post.smooth_taps(kind, H, **kw)
            assert t.shape == (W, W) and t.dtype == np.float32 and t.flags.c_contiguous and np.all(np.isfinite(t))
    j = np.arange(7, dtype=np.float64)
    A = np.vander(j - 3, 3)
    np.testing.assert_allclose(post._smooth_taps64("savgol", 3, None, None), A @ np.linalg.pinv(A), rtol=0, atol=1e-14)  # the default order is 2
    np.testing.assert_array_equal(post.smooth_taps("savgol", 3), post.smooth_taps("savgol", 3, order=2))
    g = np.exp(-((j[None] - j[:, None]) ** 2) / (2 * 1.5 ** 2))
    np.testing.assert_array_equal(post.smooth_taps("gaussian", 3), (g / g.sum(axis=1, keepdims=True)).astype(np.float32))  # sigma = H / 2
    for bad in (("savgol", 0), ("savgol", 17), ("savgol", 2.0), ("boxcar", 3), ("savgol", True)):
        with pytest.raises(ValueError):
            post.smooth_taps(*bad)
    for kw in (dict(order=7), dict(order=-1), dict(order=1.5), dict(sigma=1.0)):
        with pytest.raises(ValueError):
            post.smooth_taps("savgol", 3, **kw)
    for kw in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(order=2)):
        with pytest.raises(ValueError):
            post.smooth_taps("gaussian", 3, **kw)


def test_taps_against_scipy():
    signal = pytest.importorskip("scipy.signal")
    from stac_mjx_amd import post

    # Orders 0 .. 3: there scipy's own coefficients are within 1e-12 of exact rational arithmetic (test_taps_against_exact_
    # arithmetic's reference); at H = 16 they are 1.06e-12 off at order 4, 1.8e-10 at order 6 and 1.8e-6 at order 10, so from
    # order 4 on the exact reference takes over.
    for H in range(1, 17):
        W = 2 * H + 1
        for order in range(0, min(3, W - 1) + 1):
            t64 = post._smooth_taps64("savgol", H, order, None)
            np.testing.assert_allclose(t64[H], signal.savgol_coeffs(W, order)[::-1], rtol=0, atol=1e-12, err_msg=f"H={H} order={order}")
            for p in (0, W - 1):  # an edge row evaluates the same polynomial at the edge position
                np.testing.assert_allclose(t64[p], signal.savgol_coeffs(W, order, pos=p, use="dot"), rtol=0, atol=1e-9)
            np.testing.assert_array_equal(post.smooth_taps("savgol", H, order=order), t64.astype(np.float32))
        for sigma in (None, 0.5, 3.0):
            t64 = post._smooth_taps64("gaussian", H, None, sigma)
            np.testing.assert_allclose(t64.sum(axis=1), 1.0, rtol=0, atol=4e-16 * W)
            np.testing.assert_allclose(post.smooth_taps("gaussian", H, sigma=sigma).astype(np.float64).sum(axis=1), 1.0, rtol=0, atol=W * 2.0 ** -24)
            assert np.all(np.argmax(t64, axis=1) == np.arange(W)) and np.all(t64 >= 0)


def _exact_projector(H, order):
    """A (A^T A)^-1 A^T of A = vander(j - H, order + 1) in rational arithmetic, rounded to float64 at the end."""
    from fractions import Fraction

    W, n = 2 * H + 1, order + 1
    A = [[Fraction(j - H) ** k for k in range(order, -1, -1)] for j in range(W)]
    aug = [[sum(A[r][a] * A[r][b] for r in range(W)) for b in range(n)] + [Fraction(int(a == k)) for k in range(n)] for a in range(n)]
    for c in range(n):  # Gauss-Jordan; A^T A is positive definite, so no pivot is 0
        pv = aug[c][c]
        aug[c] = [v / pv for v in aug[c]]
        for r in range(n):
            if r != c and aug[r][c] != 0:
                f = aug[r][c]
                aug[r] = [v - f * w for v, w in zip(aug[r], aug[c])]
    inv = [row[n:] for row in aug]
    B = [[sum(A[i][a] * inv[a][b] for a in range(n)) for b in range(n)] for i in range(W)]
    return np.array([[float(sum(B[i][b] * A[j][b] for b in range(n))) for j in range(W)] for i in range(W)])


@pytest.mark.parametrize("H,order", SAVGOL_CASES + [(8, 6), (16, 10), (4, 8), (16, 32)])
def test_taps_against_exact_arithmetic(H, order):
    """The whole table, edge rows included, to the 1e-12 that the interior row is held to against scipy -- also at the orders at
    which a float64 pseudo-inverse of the Vandermonde matrix fails (order 2 H: the projector is the identity)."""
    from stac_mjx_amd import post

    np.testing.assert_allclose(post._smooth_taps64("savgol", H, order, None), _exact_projector(H, order), rtol=0, atol=1e-12)


# ---- the restatement against scipy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,order", SAVGOL_CASES)
def test_restatement_within_the_derived_bound_of_scipy_savgol_filter(H, order):
    """Each scalar output is W products and W - 1 sums of float32 with taps rounded once: its distance from the exact sum is at
    most (W + 2) 2^-24 sum_j |taps[p][j]| |x[s + j]| (first order; measured worst ratio 0.41)."""
    signal = pytest.importorskip("scipy.signal")
    from stac_mjx_amd import post

    W = 2 * H + 1
    taps = post.smooth_taps("savgol", H, order=order)
    worst = 0.0
    for L in (W, W + 1, 2 * W, 100):
        rng = np.random.default_rng([H, order, L])
        x = (np.cumsum(rng.standard_normal((L, 6)), axis=0) + 3.0 * rng.standard_normal(6)).astype(np.float32)
        got = sc.restate(x, L, taps, []).astype(np.float64)
        want = signal.savgol_filter(x.astype(np.float64), W, order, axis=0, mode="interp")
        t = np.arange(L)
        s = np.clip(t - H, 0, L - W)
        p = t - s
        mag = sum(np.abs(taps[p, j].astype(np.float64))[:, None] * np.abs(x[s + j].astype(np.float64)) for j in range(W))
        bound = (W + 2) * 2.0 ** -24 * mag
        ratio = float((np.abs(got - want) / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"H={H} order={order} L={L}: {ratio:.3g} of the bound"
    print(f"savgol H={H} order={order}: worst error {worst:.3g} of the bound")


# ---- properties of the restatement -------------------------------------------------------------------------------------------
def _case(name, H, L, clips, kind="savgol", seed=0, specials=False):
    from stac_mjx_amd import post

    nq, cols = sc.LAYOUTS[name]
    taps = post.smooth_taps(kind, H)
    return sc.make_input(L, clips, nq, cols, H, seed=seed, specials=specials), taps, nq, cols


@pytest.mark.parametrize("kind", ["savgol", "gaussian"])
def test_restatement_sign_invariance(kind):
    """Negating input quaternions changes every output by exactly the sign of its own centre frame."""
    for name, H, L, clips in (("free8", 2, 11, 2), ("tail_ball13", 5, 23, 1), ("ball4", 1, 9, 3)):
        x, taps, nq, cols = _case(name, H, L, clips, kind)
        ref = sc.restate(x, L, taps, cols)
        rng = np.random.default_rng([5, H, L])
        flipped, sign = x.copy(), np.ones((x.shape[0], nq), np.float32)
        for col in cols:
            rows = rng.random(x.shape[0]) < 0.5
            flipped[rows, col:col + 4] *= np.float32(-1.0)
            sign[rows, col:col + 4] = -1.0
        assert np.any(sign < 0)
        sc.assert_same_bits(sc.restate(flipped, L, taps, cols), ref * sign, label=f"{name} {kind}")


@pytest.mark.parametrize("kind", ["savgol", "gaussian"])
def test_restatement_unit_norm(kind):
    """n carries the roundings of four products and three sums under a square root (at most 2 u relative, u = 2^-24) and the
    root's own; each component one division's: the norm of the output is within 4 u = 2 ulp of 1."""
    for name, H, L, clips in (("free7", 3, 40, 2), ("tail_ball13", 16, 70, 1), ("rodent74", 1, 30, 1)):
        x, taps, nq, cols = _case(name, H, L, clips, kind)
        out = sc.restate(x, L, taps, cols).astype(np.float64)
        for col in cols:
            n = np.sqrt((out[:, col:col + 4] ** 2).sum(axis=1))
            assert np.abs(n - 1.0).max() <= 2.0 * np.spacing(np.float32(1.0)), (name, np.abs(n - 1.0).max())


def test_restatement_clip_independence():
    x, taps, nq, cols = _case("tail_ball13", 2, 9, 4, specials=True)
    ref = sc.restate(x, 9, taps, cols)
    other = x.copy()
    other[18:27] = sc.make_input(9, 1, nq, cols, 2, seed=9)  # clip 2 becomes another clip
    out = sc.restate(other, 9, taps, cols)
    keep = np.r_[0:18, 27:36]
    sc.assert_same_bits(out[keep], ref[keep], label="the other clips")
    assert np.any(out[18:27] != ref[18:27])
    sc.assert_same_bits(out[18:27], sc.restate(other[18:27], 9, taps, cols), label="a clip alone")  # and a clip is smoothed as if it were alone


def test_restatement_clamp_and_nan():
    from stac_mjx_amd import post

    taps = post.smooth_taps("savgol", 3, order=3)
    rng = np.random.default_rng(3)
    ub = np.float32(0.25)
    x = np.minimum(ub, ub - 0.2 + 0.3 * rng.random((60, 2))).astype(np.float32)  # a hinge that rides its limit
    free = sc.restate(x, 60, taps, [])
    assert free.max() > ub  # the polynomial overshoots
    lb_, ub_ = np.full(2, -np.inf, np.float32), np.full(2, ub, np.float32)
    out = sc.restate(x, 60, taps, [], lb_, ub_)
    assert out.max() == ub and np.all(out <= ub)
    sc.assert_same_bits(out, np.minimum(free, ub))
    x[30, 0] = np.nan  # a NaN passes the clamp, and reaches exactly the frames whose windows hold it
    out = sc.restate(x, 60, taps, [], lb_, ub_)
    np.testing.assert_array_equal(np.flatnonzero(np.isnan(out[:, 0])), np.arange(27, 34))
    assert not np.isnan(out[:, 1]).any()


# ---- a CPU build of the kernel's per-element functions --------------------------------------------------------------------------
_DRIVER = r"""
#include "stac_smooth.hpp"
using namespace stac;
extern "C" void host_smooth(const float *qpos, int64_t N, int32_t nq, int32_t L, int32_t H, const float *taps, const int32_t *quat_cols,
                            int32_t n_quat, const float *lb, const float *ub, float *out) {
    const int32_t W = 2 * H + 1;
    for (int64_t r = 0; r < N; ++r) {
        const int64_t c = r / L;
        const int32_t t = (int32_t)(r - c * L), s = smooth_window_start(t, L, H);
        const float *row = taps + (t - s) * W, *win = qpos + (c * L + s) * nq;
        for (int32_t j = 0; j < nq; ++j) {
            float v = smooth_scalar(row, win + j, nq, W);
            if (lb) v = smooth_clamp(v, lb[j], ub[j]);
            out[r * nq + j] = v;
        }
        for (int32_t b = 0; b < n_quat; ++b) smooth_quat(row, win + quat_cols[b], nq, W, qpos + r * nq + quat_cols[b], out + r * nq + quat_cols[b]);
    }
}
extern "C" int32_t host_tile_frames(int32_t nq, int32_t H) { return smooth_tile_frames(nq, H); }
extern "C" int32_t host_max_quat() { return kSmoothMaxQuat; }
"""


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    h = hs.build_cpu_library(tmp_path_factory, "smooth", _DRIVER)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    h.host_smooth.argtypes = [fp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, fp, ip, C.c_int32, fp, fp, fp]
    h.host_smooth.restype = None
    h.host_tile_frames.argtypes = [C.c_int32, C.c_int32]
    h.host_tile_frames.restype = C.c_int32
    h.host_max_quat.restype = C.c_int32
    return h


def _cpu_smooth(h, x, L, taps, cols, lb=None, ub=None):
    out = np.full_like(x, -12345.0)
    qc = np.ascontiguousarray(cols, dtype=np.int32)
    h.host_smooth(hs.fp(x), x.shape[0], x.shape[1], L, taps.shape[0] // 2, hs.fp(taps), qc.ctypes.data_as(C.POINTER(C.c_int32)), len(cols),
                  hs.fp(lb), hs.fp(ub), hs.fp(out))
    return out


def test_tile_frames_of_header_and_python_agree(hostlib):
    from stac_mjx_amd import post

    assert hostlib.host_max_quat() == post.SMOOTH_MAX_QUAT >= max(len(cols) for _, cols in sc.LAYOUTS.values())
    for H in range(1, 17):
        for nq in list(range(1, 600)) + [4093, 4094, 20000]:
            T = post.smooth_tile_frames(nq, H)
            assert T == hostlib.host_tile_frames(nq, H), (nq, H)
            W = 2 * H + 1
            assert T == 0 or (1 <= T <= post.SMOOTH_MAX_TILE and W * W + 2 * nq + (T + 2 * H) * nq <= post.SMOOTH_LDS_FLOATS)
    # the models of tests/golden/: what DESIGN.md states
    assert [post.smooth_tile_frames(74, H) for H in (3, 16)] == [128, 128]
    assert [post.smooth_tile_frames(230, H) for H in (3, 16)] == [63, 32]
    assert post.smooth_tile_frames(437, 16) == 1 and post.smooth_tile_frames(438, 16) == 0
    assert post.smooth_tile_frames(3275, 1) == 1 and post.smooth_tile_frames(3276, 1) == 0


@pytest.mark.parametrize("name", list(sc.LAYOUTS))
@pytest.mark.parametrize("H", sc.HALF_WINDOWS)
def test_cpu_build_equals_restatement(hostlib, name, H):
    from stac_mjx_amd import post

    nq, cols = sc.LAYOUTS[name]
    T = post.smooth_tile_frames(nq, H)
    for i, L in enumerate(sc.clip_lengths(T, H)):
        clips, bounded, kind = (1, 3)[i & 1], bool(i & 2), ("savgol", "gaussian")[(i >> 2) & 1]
        taps = post.smooth_taps(kind, H)
        x = sc.make_input(L, clips, nq, cols, H)
        lb, ub = sc.make_bounds(nq, cols) if bounded else (None, None)
        want = sc.restate(x, L, taps, cols, lb, ub)
        sc.assert_same_bits(_cpu_smooth(hostlib, x, L, taps, cols, lb, ub), want, label=f"{name} H={H} L={L} clips={clips} {kind}")
        if cols and clips == 3:  # the cases hold what they are meant to: the n > 0 branch passed the centre block on
            np.testing.assert_array_equal(want[L:2 * L, cols[0]:cols[0] + 4], 0.0)
        if bounded and nq >= 74:
            assert np.any(want == ub) and np.any(want == lb)  # ... and the clamp acted on both sides


# ---- the entry point's argument checks (before the device is touched) -------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return hs.loaded_library()


def test_smooth_argument_errors_need_no_device(lib):
    """Every device pointer below is a fake non-NULL address: a call that got past its checks would fault, not return."""
    taps = np.zeros(33 * 33, np.float32)
    tp = taps.ctypes.data_as(C.POINTER(C.c_float))
    q, out, lb, ub = C.c_void_p(0x100000), C.c_void_p(0x900000), C.c_void_p(0x10000), C.c_void_p(0x20000)

    def call(q=q, N=40, nq=13, L=10, H=3, taps=tp, cols=(3, 9), lb=lb, ub=ub, out=out):
        qc = (C.c_int32 * max(len(cols), 1))(*cols) if cols is not None else None
        return lib.stac_post_smooth(q, N, nq, L, H, taps, qc, len(cols) if cols is not None else 1, lb, ub, out, None)

    hs.invalid(lib, call(H=0))
    assert "17" in hs.invalid(lib, call(H=17, L=40))
    msg = hs.invalid(lib, call(L=5, N=40))  # clip_len < W: names both numbers
    assert "5" in msg and "7" in msg
    assert "41" in hs.invalid(lib, call(N=41))  # N % clip_len != 0
    hs.invalid(lib, call(N=-10))
    hs.invalid(lib, call(nq=0, cols=()))
    assert "overlap" in hs.invalid(lib, call(cols=(3, 6)))
    assert "overlap" in hs.invalid(lib, call(cols=(9, 3, 9)))
    assert "leaves" in hs.invalid(lib, call(cols=(3, 10)))  # 10 + 4 > 13
    hs.invalid(lib, call(cols=(-1,)))
    assert "64" in hs.invalid(lib, call(nq=400, cols=tuple(range(0, 260, 4))))  # 65 blocks
    assert call(N=0, nq=400, cols=tuple(range(0, 256, 4)), q=None, out=None) == 0  # 64 are fine (and N == 0: nothing to do)
    hs.invalid(lib, call(cols=None))
    hs.invalid(lib, call(nq=450, H=16, L=40))  # no room for a window in LDS
    hs.invalid(lib, call(taps=None))
    hs.invalid(lib, call(lb=None))
    hs.invalid(lib, call(ub=None))
    hs.invalid(lib, call(q=None))
    hs.invalid(lib, call(out=None))
    hs.invalid(lib, call(q=C.c_void_p(0x100002)))
    assert "overlap" in hs.invalid(lib, call(out=q))  # in place
    assert "overlap" in hs.invalid(lib, call(out=C.c_void_p(0x100000 + 40 * 13 * 4 - 4)))
    assert "overlap" in hs.invalid(lib, call(lb=C.c_void_p(0x900000 + 64)))
    assert call(N=0, q=None, out=None) == 0 and call(N=0, lb=None, ub=None, cols=(), q=None, out=None) == 0


def test_python_wrapper_refuses_before_the_library(lib):
    import torch

    from stac_mjx_amd import post

    taps = post.smooth_taps("savgol", 3)
    with pytest.raises(ValueError, match="CUDA"):
        post.smooth(torch.zeros(14, 8), 7, taps, [3])
    with pytest.raises(ValueError, match="CUDA"):
        post.smooth(np.zeros((14, 8), np.float32), 7, taps, [3])


# ---- qpos_raw in the result files -------------------------------------------------------------------------------------------------
def test_qpos_raw_round_trip(tmp_path, rodent_cfg):
    for suffix in hs.result_suffixes():
        _qpos_raw_round_trip(tmp_path, rodent_cfg, suffix)


def _qpos_raw_round_trip(tmp_path, rodent_cfg, suffix):
    from stac_mjx_amd import io

    rng = np.random.default_rng(0)
    data = io.StacData(qpos=rng.random((6, 74), dtype=np.float32), xpos=rng.random((6, 67, 3), dtype=np.float32),
                       xquat=rng.random((6, 67, 4), dtype=np.float32), marker_sites=rng.random((6, 23, 3), dtype=np.float32),
                       offsets=rng.random((23, 3), dtype=np.float32), kp_data=rng.random((6, 69), dtype=np.float32),
                       names_qpos=[f"q{i}" for i in range(74)], names_xpos=[f"b{i}" for i in range(67)], kp_names=[f"k{i}" for i in range(23)])
    assert data.qpos_raw.size == 0 and "qpos_raw" not in data.as_dict()
    cfg = hs.stage_cfg(rodent_cfg)
    plain = io.save_data_to_h5(config=cfg, file_path=tmp_path / f"plain{suffix}", **data.as_dict())
    back = io.load_stac_data(plain)[1]
    assert back.qpos_raw.size == 0 and "qpos_raw" not in back.as_dict()  # a file without it loads with the empty array
    data.qpos_raw = rng.random((6, 74), dtype=np.float32)
    assert "qpos_raw" in data.as_dict()
    path = io.save_data_to_h5(config=cfg, file_path=tmp_path / f"smooth{suffix}", **data.as_dict())
    back = io.load_stac_data(path)[1]
    assert back.qpos_raw.dtype == np.float32
    np.testing.assert_array_equal(back.qpos_raw, data.qpos_raw)
    np.testing.assert_array_equal(back.qpos, data.qpos)
    if suffix == ".h5":
        import h5py

        with h5py.File(plain, "r") as f:
            assert "qpos_raw" not in f
        with h5py.File(path, "r") as f:
            assert f["qpos_raw"].shape == (6, 74)


def test_qpos_raw_in_sharded_results(tmp_path, rodent_cfg):
    from stac_mjx_amd import io

    rng = np.random.default_rng(1)
    cfg = hs.stage_cfg(rodent_cfg)
    raws = []
    for r in range(2):
        d = io.StacData(qpos=rng.random((4, 74), dtype=np.float32), xpos=rng.random((4, 67, 3), dtype=np.float32),
                        xquat=rng.random((4, 67, 4), dtype=np.float32), marker_sites=rng.random((4, 23, 3), dtype=np.float32),
                        offsets=np.zeros((23, 3), np.float32), kp_data=rng.random((4, 69), dtype=np.float32), names_qpos=["q"] * 74,
                        names_xpos=["b"] * 67, kp_names=["k"] * 23, qpos_raw=rng.random((4, 74), dtype=np.float32))
        raws.append(d.qpos_raw)
        io.save_data_to_h5(config=cfg, file_path=io.shard_path(tmp_path / "ik.h5", r, 2), **d.as_dict())
    manifest = io.write_manifest(io.manifest_path(tmp_path / "ik.h5"), tmp_path / "ik.h5", 2, 4, 2)
    np.testing.assert_array_equal(io.load_sharded_stac_data(manifest)[1].qpos_raw, np.concatenate(raws))
