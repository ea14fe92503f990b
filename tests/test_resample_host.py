"""stac.resample, the parts that need no GPU: the tap table against ``scipy.signal.resample_poly``, the normalised rows, the index
rules with Python integers (beyond int32 too), every refusal of the options, the pre-flight and the Python functions,
the argument checks of the entry point (they happen before the device is touched), and a
CPU build of csrc/stac_resample.hpp against the numpy restatement of tests/resample_cases.py, bit for bit."""

import ctypes as C
import functools

import numpy as np
import pytest

import resample_cases as rc
import host_scaffold as hs
from host_scaffold import STAC_ERR_INVALID

BIG = 2**31 + 5


@pytest.fixture(scope="module")
def lib():
    return hs.loaded_library()


# ---- the table -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,D", rc.SCIPY_RATIOS)
def test_table_is_scipys_filter(U, D):
    """The float64 restatement with the raw table against resample_poly with edge padding.  1e-12: a float64 sum of at most 257
    terms of magnitude at most 2 is good to about 1e-13."""
    signal = pytest.importorskip("scipy.signal")
    from stac_mjx_amd import post

    taps = rc.taps64(U, D, normalise=False)
    np.testing.assert_array_equal(post._resample_taps64(U, D, normalise=False), taps)  # the product's builder is the formula too
    for L in (1, 2, 7, 50, 400):
        x = np.random.default_rng([L, U, D]).standard_normal((L, 3)) * 2.0 / 3.0
        x = np.clip(x, -2.0, 2.0)
        ours = rc.restate(x, L, U, D, taps, dtype=np.float64)
        ref = signal.resample_poly(x, U, D, axis=0, window=("kaiser", 5.0), padtype="edge")
        k = min(len(ours), len(ref))
        assert k == rc.rows(L, U, D) == len(ours)  # (scipy adds the outputs beyond the last sample)
        err = np.abs(ours[:k] - ref[:k]).max()
        print(f"{U}/{D} L={L}: {k} rows, max |ours - scipy| = {err:.3g}")
        assert err <= 1e-12, (U, D, L, err)


@pytest.mark.parametrize("U,D,lobes", [(1, 6, 10), (5, 12, 10), (5, 3, 10), (2, 1, 1), (32, 1, 3), (3, 10, 16), (1, 12, 10)])
def test_normalised_rows_keep_a_constant(U, D, lobes):
    from stac_mjx_amd import post

    raw, t64 = rc.taps64(U, D, lobes, normalise=False), rc.taps64(U, D, lobes)
    assert np.abs(t64.sum(axis=1) - 1.0).max() <= 1e-15
    if (U, D, lobes) == (5, 3, 10):  # why the rows are normalised: at 30 -> 50 the raw phase sums miss 1 by 6.5e-4
        assert 6e-4 < np.abs(raw.sum(axis=1) - 1.0).max() < 7e-4
    np.testing.assert_array_equal(post._resample_taps64(U, D, lobes), t64)
    t32 = post.resample_taps(U, D, lobes)
    assert t32.dtype == np.float32 and t32.shape == t64.shape and t32.flags.c_contiguous
    np.testing.assert_array_equal(t32, t64.astype(np.float32))
    W = t32.shape[1]
    assert W == 2 * ((lobes * max(U, D)) // U + 1)
    for c in (np.float32(1.0), np.float32(-37.25), np.float32(3.1e-3)):
        out = rc.restate(np.full((23, 1), c, np.float32), 23, U, D, t32)
        assert np.abs(out.astype(np.float64) - float(c)).max() <= (W + 1) * 2.0**-23 * abs(float(c)), (U, D, c)


# ---- index rules -----------------------------------------------------------------------------------------------------------------
_DRIVER = r"""
#include <vector>
#include "stac_resample.hpp"
using namespace stac;
extern "C" void host_resample(const float *x, int64_t N, int32_t C, int64_t L, int32_t U, int32_t D, int32_t half, const float *taps,
                              const int32_t *quat_cols, int32_t n_quat, const float *lb, const float *ub, float *out) {
    const int32_t H = resample_half_rows(half, U), W = 2 * H;
    const int64_t Lo = resample_rows(L, U, D);
    std::vector<float> win((size_t)W * C);
    for (int64_t clip = 0; clip < N / L; ++clip)
        for (int64_t m = 0; m < Lo; ++m) {
            int64_t n;
            int32_t r;
            resample_index(m, U, D, &n, &r);
            for (int32_t j = 0; j < W; ++j) {
                int64_t row = n + (j - H + 1);
                row = row < 0 ? 0 : (row > L - 1 ? L - 1 : row);
                for (int32_t c = 0; c < C; ++c) win[(size_t)j * C + c] = x[(clip * L + row) * C + c];
            }
            float *o = out + (clip * Lo + m) * C;
            for (int32_t c = 0; c < C; ++c) {
                float v = resample_scalar(taps + r * W, win.data() + c, C, W);
                if (lb) v = smooth_clamp(v, lb[c], ub[c]);
                o[c] = v;
            }
            for (int32_t b = 0; b < n_quat; ++b)
                smooth_quat(taps + r * W, win.data() + quat_cols[b], C, W, x + (clip * L + n) * C + quat_cols[b], o + quat_cols[b]);
        }
}
extern "C" int64_t host_rows(int64_t L, int32_t U, int32_t D) { return resample_rows(L, U, D); }
extern "C" int64_t host_n(int64_t m, int32_t U, int32_t D) { int64_t n; int32_t r; resample_index(m, U, D, &n, &r); return n; }
extern "C" int32_t host_r(int64_t m, int32_t U, int32_t D) { int64_t n; int32_t r; resample_index(m, U, D, &n, &r); return r; }
extern "C" int64_t host_source_row(int64_t m, int64_t L, int32_t U, int32_t D) { return resample_source_row(m, L, U, D); }
extern "C" int32_t host_band_cols(int32_t C) { return resample_band_cols(C); }
extern "C" int32_t host_tile_rows(int32_t bw, int32_t U, int32_t D, int32_t H) { return resample_tile_rows(bw, U, D, H); }
extern "C" int32_t host_lds_floats(int32_t T, int32_t bw, int32_t U, int32_t D, int32_t H) { return resample_lds_floats(T, bw, U, D, H); }
extern "C" int32_t host_constant(int32_t i) {
    const int32_t v[] = {kResampleMaxUp, kResampleMaxDown, kResampleMaxWin, kResampleMaxQuat, kResampleMaxBand, kResampleOverhang,
                         kResampleLdsFloats, kResampleMaxTile};
    return v[i];
}
"""


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    h = hs.build_cpu_library(tmp_path_factory, "resample", _DRIVER)
    fp, ip, i32, i64 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int32, C.c_int64
    for name, res, args in (("host_resample", None, [fp, i64, i32, i64, i32, i32, i32, fp, ip, i32, fp, fp, fp]), ("host_rows", i64, [i64, i32, i32]),
                            ("host_n", i64, [i64, i32, i32]), ("host_r", i32, [i64, i32, i32]), ("host_source_row", i64, [i64, i64, i32, i32]),
                            ("host_band_cols", i32, [i32]), ("host_tile_rows", i32, [i32] * 4), ("host_lds_floats", i32, [i32] * 5),
                            ("host_constant", i32, [i32])):
        getattr(h, name).restype, getattr(h, name).argtypes = res, args
    return h


def test_index_rules_with_python_integers(hostlib, lib):
    from stac_mjx_amd import post

    for U, D in ((1, 6), (5, 12), (5, 3), (2, 1), (32, 1), (1, 64), (31, 64), (3, 10)):
        for L in (1, 2, 3, 7, 400, BIG):
            Lo = ((L - 1) * U) // D + 1
            assert post.resample_rows(L, U, D) == Lo == hostlib.host_rows(L, U, D) == lib.stac_post_resample_rows(L, U, D), (L, U, D)
            assert (Lo - 1) * D <= (L - 1) * U < Lo * D  # the last output is not beyond the last sample, the next one would be
            for m in sorted(m for m in {0, 1, Lo // 2, Lo - 2, Lo - 1} if 0 <= m < Lo):
                n, r = divmod(m * D, U)
                assert (hostlib.host_n(m, U, D), hostlib.host_r(m, U, D)) == (n, r) and n <= L - 1
                assert hostlib.host_source_row(m, L, U, D) == min(n + (1 if 2 * r > U else 0), L - 1), (m, L, U, D)
            if L < BIG:
                n, r = rc.index(L, U, D)
                src = post.resample_source_rows(L, U, D)
                assert src.dtype == np.int64 and src.shape == (Lo,)
                assert src.tolist() == [min(int(a) + (1 if 2 * int(b) > U else 0), L - 1) for a, b in zip(n, r)]
                assert src.tolist() == [hostlib.host_source_row(m, L, U, D) for m in range(Lo)]
    assert post.resample_source_rows(7, 5, 12).tolist() == [0, 2, 5]  # positions 0, 2.4, 4.8
    assert post.resample_source_rows(4, 2, 1).tolist() == [0, 0, 1, 1, 2, 2, 3]  # a tie goes down
    assert hostlib.host_n(BIG * 5, 32, 64) == BIG * 10 and lib.stac_post_resample_rows(BIG, 32, 1) == (BIG - 1) * 32 + 1


def test_tile_rule_of_header_and_python_agree(hostlib):
    from stac_mjx_amd import config, post

    names = ("RESAMPLE_MAX_UP", "RESAMPLE_MAX_DOWN", "RESAMPLE_MAX_WIN", "SMOOTH_MAX_QUAT", "RESAMPLE_MAX_BAND", "RESAMPLE_OVERHANG",
             "RESAMPLE_LDS_FLOATS", "RESAMPLE_MAX_TILE")
    assert [hostlib.host_constant(i) for i in range(8)] == [getattr(post, n) for n in names]
    assert (config.RESAMPLE_MAX_UP, config.RESAMPLE_MAX_DOWN, config.RESAMPLE_MAX_WIN, config.RESAMPLE_MAX_LOBES) == \
        (post.RESAMPLE_MAX_UP, post.RESAMPLE_MAX_DOWN, post.RESAMPLE_MAX_WIN, post.RESAMPLE_MAX_LOBES)
    for C_ in list(range(1, 200)) + [230, 255, 256, 257, 511, 512]:
        bw = post.resample_band_cols(C_)
        assert bw == hostlib.host_band_cols(C_) and 1 <= bw <= post.RESAMPLE_MAX_BAND and -(-C_ // bw) == -(-C_ // post.RESAMPLE_MAX_BAND)
    # nothing is refused for W <= 256: at least one output fits for every band, ratio and window
    for bw in (1, 7, 37, 58, 63, 64):
        for U, D in ((1, 1), (1, 6), (5, 12), (32, 1), (1, 64), (32, 63), (31, 64)):
            for H in (1, 2, 3, 25, 61, 121, 128):
                C_ = bw  # (a row of one band)
                T = post.resample_tile_rows(C_, U, D, 2 * H)
                assert T == hostlib.host_tile_rows(bw, U, D, H), (bw, U, D, H)
                lds = post.resample_lds_floats(T, bw, U, D, H)
                assert lds == hostlib.host_lds_floats(T, bw, U, D, H)
                assert 1 <= T <= post.RESAMPLE_MAX_TILE and lds <= post.RESAMPLE_LDS_FLOATS and (T < U or T % U == 0), (bw, U, D, H, T, lds)
    # what DESIGN.md states for the rodent's row
    assert post.resample_band_cols(74) == 37 and post.resample_tile_rows(74, 1, 6, 122) == 65 and post.resample_tile_rows(74, 5, 12, 50) == 125


# ---- options, pre-flight, Python arguments -----------------------------------------------------------------------------------------
_cfg = functools.partial(hs.stage_cfg, n_frames_per_clip=12)


def test_resample_options_and_their_refusals(rodent_cfg):
    from stac_mjx_amd.config import ConfigError, resample_options

    off = resample_options({})
    assert off == {"kind": "off", "from_hz": None, "to_hz": None, "up": None, "down": None, "lobes": 10, "beta": 5.0}
    assert resample_options({"resample": False}) == off and resample_options({"resample": None}) == off
    on = dict(resample="kaiser", mocap_hz=120, resample_hz=50, postprocess="gpu")
    assert resample_options(on) == {"kind": "kaiser", "from_hz": 120, "to_hz": 50, "up": 5, "down": 12, "lobes": 10, "beta": 5.0}
    assert resample_options(dict(on, mocap_hz=29.97, resample_hz=59.94))["up"] == 2
    assert resample_options(dict(on, mocap_hz=300, resample_lobes=16, resample_beta=0))["lobes"] == 16
    for bad, word in ((dict(on, resample="sinc"), "stac.resample "), (dict(on, resample=True), "stac.resample "),
                      (dict(on, mocap_hz=None), "stac.mocap_hz"), (dict(resample="kaiser", mocap_hz=120, postprocess="gpu"), "stac.resample_hz"),
                      (dict(on, mocap_hz=0), "stac.mocap_hz"), (dict(on, resample_hz=float("inf")), "stac.resample_hz"),
                      (dict(on, resample_hz="50"), "stac.resample_hz"), (dict(on, mocap_hz=True), "stac.mocap_hz"),
                      (dict(mocap_hz=-3), "stac.mocap_hz"),                                    # a bad rate is refused with resample off too
                      (dict(on, resample_lobes=0), "stac.resample_lobes"), (dict(on, resample_lobes=17), "stac.resample_lobes"),
                      (dict(on, resample_lobes=2.0), "stac.resample_lobes"), (dict(resample_beta=-1), "stac.resample_beta"),
                      (dict(on, resample_beta=float("nan")), "stac.resample_beta"),
                      (dict(on, mocap_hz=29.97), "5000 / 2997"),                              # U > 32
                      (dict(on, mocap_hz=1, resample_hz=33), "33 / 1"),                       # U > 32
                      (dict(on, mocap_hz=65, resample_hz=1), "1 / 65"),                       # D > 64
                      (dict(on, mocap_hz=600, resample_lobes=16), "386 taps"),                # W > 256
                      (dict(on, postprocess="host"), "stac.postprocess"), ({k: v for k, v in on.items() if k != "postprocess"}, "stac.postprocess"),
                      (dict(on, reference_marker_order=True), "reference_marker_order")):
        with pytest.raises(ConfigError) as e:
            resample_options(bad)
        assert word in str(e.value) and "stac." in str(e.value), (bad, str(e.value))
    # validate_config runs them, takes the five keys, and turns the boolean of a bare YAML off into the word
    assert _cfg(rodent_cfg, **on).stac.resample == "kaiser" and _cfg(rodent_cfg, resample=False).stac.resample == "off"
    with pytest.raises(ConfigError, match="stac.resample_lobes"):
        _cfg(rodent_cfg, **dict(on, resample_lobes=99))
    assert "resample" not in _cfg(rodent_cfg).stac


def test_run_stac_refuses_before_any_work(tmp_path, rodent_cfg):
    from stac_mjx_amd.config import RESAMPLE_SHARDED
    from stac_mjx_amd.main import _Preflight, resampled_path, run_stac

    names = list(rodent_cfg["KEYPOINT_MODEL_PAIRS"].keys())
    kp = np.zeros((12, 69), np.float32)
    on = dict(resample="kaiser", mocap_hz=120, resample_hz=50, postprocess="gpu")
    for key, value, word in (("postprocess", "host", "stac.postprocess"), ("resample_hz", None, "stac.resample_hz"),
                             ("mocap_hz", 29.97, "5000 / 2997"), ("reference_marker_order", True, "reference_marker_order"),
                             ("resample_lobes", 40, "stac.resample_lobes")):
        cfg = _cfg(rodent_cfg, **on)
        cfg.stac[key] = value  # a bad value set after validation
        with pytest.raises(ValueError, match=word):  # before the model is even looked for: the path does not exist
            run_stac(cfg, kp, names, base_path=tmp_path / "nowhere")
    assert not list(tmp_path.iterdir())
    # an explicit gather = none on more than one rank: the output is sharded
    pre = _Preflight(_cfg(rodent_cfg, gather="none", **on), 12, tmp_path / "fit.h5", kp_names=names)
    pre.check_config()
    assert pre.resample["up"] == 5 and pre.resample["down"] == 12
    with pytest.raises(ValueError) as e:
        pre.check_run(2)
    assert str(e.value) == RESAMPLE_SHARDED
    pre.check_run(1)
    off = _Preflight(_cfg(rodent_cfg, gather="none"), 12, tmp_path / "fit.h5", kp_names=names)
    off.check_config()
    off.check_run(2)
    assert off.resample is None
    skipped = _Preflight(_cfg(rodent_cfg, skip_ik_only=True, **on), 12, tmp_path / "fit.h5", kp_names=names)
    skipped.check_config()
    assert skipped.resample is None
    assert resampled_path(tmp_path / "ik_only.h5", 50) == tmp_path / "ik_only.50hz.h5"
    assert resampled_path("ik.npz", 29.97).name == "ik.29.97hz.npz" and resampled_path("ik.h5", 50.0).name == "ik.50hz.h5"


def test_python_functions_refuse_bad_arguments():
    from stac_mjx_amd import post

    assert post.resample_ratio(300, 50) == (1, 6) and post.resample_ratio(120, 50) == (5, 12) and post.resample_ratio(30, 50) == (5, 3)
    assert post.resample_ratio(29.97, 59.94) == (2, 1) and post.resample_ratio(np.float64(200.0), np.int64(50)) == (1, 4)
    assert post.resample_ratio(0.1, 0.3) == (3, 1)  # the decimal text, not the binary neighbour
    for a in ((29.97, 50), (1, 33), (65, 1), (0, 50), (50, -1), (float("nan"), 50), (50, float("inf")), (True, 50), ("120", 50)):
        with pytest.raises(ValueError):
            post.resample_ratio(*a)
    for a in ((0, 1, 1), (2, 33, 1), (2, 1, 65), (2, 0, 1), (2, True, 1), (2.0, 1, 1)):
        with pytest.raises(ValueError):
            post.resample_rows(*a)
    for kw in (dict(U=33, D=1), dict(U=1, D=65), dict(U=1, D=6, lobes=0), dict(U=1, D=6, lobes=17), dict(U=1, D=6, lobes=True),
               dict(U=1, D=6, beta=-0.5), dict(U=1, D=6, beta=float("nan")), dict(U=1, D=13, lobes=10), dict(U=1, D=64, lobes=2)):
        with pytest.raises(ValueError):  # (the last two: windows of 262 and 258 taps)
            post.resample_taps(**kw)
    assert post.resample_taps(1, 12, 10).shape == (1, 242) and post.resample_taps(32, 1, 1).shape == (32, 4)
    with pytest.raises(ValueError, match="CUDA"):
        post.resample(np.zeros((4, 3), np.float32), 4, 1, 2, post.resample_taps(1, 2))


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments_before_the_device(lib):
    """Made-up addresses: nothing may be read through them, every refusal comes from the arguments alone."""
    A = 1 << 20
    cols = (C.c_int32 * 2)(3, 9)
    good = dict(x=A, n_rows=40, n_cols=13, clip_len=10, up=5, down=12, half=12, taps=2 * A, cols=cols, n_quat=2, lb=3 * A, ub=4 * A, out=5 * A,
                out_rows=16, stream=None)

    def refused(word, **kw):
        a = dict(good)
        a.update(kw)
        rcode = lib.stac_post_resample(a["x"], a["n_rows"], a["n_cols"], a["clip_len"], a["up"], a["down"], a["half"], a["taps"], a["cols"],
                                       a["n_quat"], a["lb"], a["ub"], a["out"], a["out_rows"], a["stream"])
        msg = lib.stac_last_error().decode()
        assert rcode == STAC_ERR_INVALID and lib.stac_last_error_code() == STAC_ERR_INVALID, (kw, rcode, msg)
        assert msg.startswith("stac_post_resample: ") and word in msg, (kw, msg)

    assert rc.rows(10, 5, 12) * 4 == good["out_rows"]
    refused("n_rows >= 0", n_rows=-1)
    refused("n_cols >= 1", n_cols=0)
    refused("clip_len >= 1", clip_len=0)
    refused("up is outside", up=0)
    refused("up is outside", up=33)
    refused("down is outside", down=65)
    refused("down is outside", down=0)
    refused("256", half=5 * 128)         # H = 129, W = 258
    refused("negative", half=-1)
    refused("not whole clips", clip_len=16)
    refused("out_rows = 15", out_rows=15)
    refused("out_rows = 17", out_rows=17)
    refused("quaternion blocks, at most 64", n_quat=65)
    refused("quaternion blocks, at most 64", n_quat=-1)
    refused("null quat_cols", cols=None)
    refused("overlap", cols=(C.c_int32 * 2)(3, 6))
    refused("leaves the row", cols=(C.c_int32 * 2)(3, 10))
    refused("leaves the row", cols=(C.c_int32 * 2)(-1, 9))
    refused("null taps_dev", taps=None)
    refused("lb and ub", lb=None)
    refused("lb and ub", ub=None)
    refused("null x / out", x=None)
    refused("null x / out", out=None)
    for name in ("x", "taps", "lb", "ub", "out"):
        refused("4-byte aligned", **{name: good[name] + 2})
    refused("x and out overlap", out=A + 40 * 13 * 4 - 4)
    refused("taps_dev and out overlap", out=2 * A + 4)
    refused("lb and out overlap", out=3 * A - 16 * 13 * 4 + 4)
    refused("lb and ub overlap", ub=3 * A + 4 * 12)
    # nothing to do is no error, and is decided before any pointer is looked at
    assert lib.stac_post_resample(None, 0, 13, 10, 5, 12, 12, 2 * A, cols, 2, None, None, None, 0, None) == 0
    assert lib.stac_post_resample_rows(0, 1, 2) == STAC_ERR_INVALID and "stac_post_resample_rows" in lib.stac_last_error().decode()
    assert lib.stac_post_resample_rows(5, 33, 2) == STAC_ERR_INVALID and lib.stac_post_resample_rows(5, 1, 65) == STAC_ERR_INVALID


# ---- the header against numpy --------------------------------------------------------------------------------------------------------
def cpu_resample(h, x, L, U, D, taps, cols, lb=None, ub=None):
    W = taps.shape[1]
    out = np.full(((x.shape[0] // L) * rc.rows(L, U, D), x.shape[1]), -12345.0, np.float32)
    qc = np.ascontiguousarray(cols, dtype=np.int32)
    h.host_resample(hs.fp(x), x.shape[0], x.shape[1], L, U, D, (W // 2 - 1) * U, hs.fp(taps), qc.ctypes.data_as(C.POINTER(C.c_int32)), len(cols),
                    hs.fp(lb), hs.fp(ub), hs.fp(out))
    return out


def test_cpu_build_equals_restatement(hostlib):
    from stac_mjx_amd import post

    cases = rc.cases(post.resample_tile_rows, post.RESAMPLE_MAX_BAND)
    assert len(cases) > 40
    for label, U, D, taps, L, clips, ncol, cols, bounded in cases:
        x = rc.make_input(L, clips, ncol, cols)
        lb, ub = rc.make_bounds(ncol, cols) if bounded else (None, None)
        want = rc.restate(x, L, U, D, taps, cols, lb, ub)
        assert want.shape == (clips * rc.rows(L, U, D), ncol)
        rc.assert_same_bits(cpu_resample(hostlib, x, L, U, D, taps, cols, lb, ub), want, label=label)


def test_restatement_properties():
    """What the rule promises, on the restatement alone: clips do not see each other, a sign-alternating quaternion series comes out as
    if it did not alternate, a zero centre block takes the fallback, a NaN reaches exactly the outputs whose window holds it, and
    the bounds cut the overshoot of a step."""
    U, D = 5, 12
    taps = rc.taps32(U, D, 2)
    W = taps.shape[1]
    H = W // 2
    L, Lo = 40, rc.rows(40, U, D)
    n, _ = rc.index(L, U, D)
    # clips: three constants
    x = np.repeat(np.array([1.0, 100.0, -50.0], np.float32), L)[:, None]
    out = rc.restate(x, L, U, D, taps).reshape(3, Lo)
    for c, row in zip((1.0, 100.0, -50.0), out):
        assert np.abs(row.astype(np.float64) - c).max() <= (W + 1) * 2.0**-23 * abs(c)
    # quaternions: q, -q, q, ... comes out as the plain series does, times the sign of the centre row -- bit for bit, a sign is exact
    q, flip, sign = rc.alternating_quats(L, n)
    plain, alt = rc.restate(q, L, U, D, taps, [0]), rc.restate(flip, L, U, D, taps, [0])
    rc.assert_same_bits(alt, plain * sign, label="alternating signs")
    assert np.abs(np.linalg.norm(alt.astype(np.float64), axis=1) - 1.0).max() <= 2.0 * np.spacing(np.float32(1.0))
    # a zero block in the centre row decides no hemisphere (every dot product is 0 and counts as +): the rows are summed as they are;
    # the fallback is for a sum without a direction -- a window of zeros gives the centre block back
    z = q.copy()
    z[int(n[5])] = 0.0
    out = rc.restate(z, L, U, D, taps, [0])
    assert abs(float(np.linalg.norm(out[5].astype(np.float64))) - 1.0) <= 2.0 * np.spacing(np.float32(1.0))
    z[:] = 0.0
    z[L - 1] = q[L - 1]
    out = rc.restate(z, L, U, D, taps, [0])
    np.testing.assert_array_equal(out[0], np.zeros(4, np.float32))
    assert abs(float(np.linalg.norm(out[-1].astype(np.float64))) - 1.0) <= 2.0 * np.spacing(np.float32(1.0))
    # NaN
    x = rc.make_input(L, 1, 3, [], specials=False)
    x[17, 1] = np.nan
    out = rc.restate(x, L, U, D, taps)
    hit = np.flatnonzero((n - H + 1 <= 17) & (17 <= n + H))
    np.testing.assert_array_equal(np.flatnonzero(np.isnan(out[:, 1])), hit)
    assert hit.size and not np.isnan(out[:, [0, 2]]).any()
    # bounds
    step = np.where(np.arange(L) < 20, -1.0, 1.0).astype(np.float32)[:, None]
    free = rc.restate(step, L, U, D, taps)
    assert free.max() > 1.0 or free.min() < -1.0
    cut = rc.restate(step, L, U, D, taps, [], np.array([-1.0], np.float32), np.array([1.0], np.float32))
    assert cut.max() <= 1.0 and cut.min() >= -1.0
    rc.assert_same_bits(cut, np.clip(free, -1.0, 1.0))
