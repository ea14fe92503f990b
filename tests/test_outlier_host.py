"""reject_outliers, the parts that need no GPU: the rule of csrc/stac_outlier.hpp as a stand-alone CPU program against the numpy
reference of tests/outlier_cases.py, what the reference finds in a series with known spikes, the config keys, the argument checks of
``stac_prep_reject`` (they happen before the device is touched) and ``kp_rejected`` through the result files."""

import ctypes as C
import subprocess

import numpy as np
import pytest

import outlier_cases as oc
import host_scaffold as hs
from conftest import ROOT
from host_scaffold import STAC_ERR_INVALID

TILE = 64  # prep.TILE_FRAMES (asserted below)


# ---- the rule on the CPU, from the kernel's header --------------------------------------------------------------------------------
_PROGRAM = r"""
// The rule of csrc/stac_outlier.hpp run serially: the series is sanitized (missing keypoints and h frames beyond both ends are NaN),
// as the kernel's LDS image is, and outlier_coord decides every coordinate.
// usage: prog IN OUT.  IN: int64 n, then per case int64 T, K, h, double thr, min_dev and T * 3K floats.
// OUT: per case T * 3K floats, T * K bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "stac_outlier.hpp"
using namespace stac;

static void reject(const float *kp, int64_t T, int64_t K, int32_t h, double thr, double min_dev, float *out, uint8_t *flag) {
    const int64_t K3 = 3 * K;
    std::vector<float> img((T + 2 * h) * K3, outlier_nan());
    for (int64_t t = 0; t < T; ++t)
        for (int64_t k = 0; k < K; ++k) {
            const float *s = kp + t * K3 + 3 * k;
            if (!prep_missing(s[0], s[1], s[2]))
                for (int c = 0; c < 3; ++c) img[(t + h) * K3 + 3 * k + c] = s[c];
        }
    for (int64_t t = 0; t < T; ++t)
        for (int64_t k = 0; k < K; ++k) {
            const float *s = kp + t * K3 + 3 * k, *c = img.data() + (t + h) * K3 + 3 * k;
            float *o = out + t * K3 + 3 * k;
            bool rejected = false;
            if (!prep_missing(s[0], s[1], s[2]))
                rejected = outlier_coord(c, K3, h, thr, min_dev) || outlier_coord(c + 1, K3, h, thr, min_dev) ||
                           outlier_coord(c + 2, K3, h, thr, min_dev);
            for (int i = 0; i < 3; ++i) o[i] = rejected ? outlier_nan() : s[i];
            flag[t * K + k] = rejected ? 1 : 0;
        }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *outf = fopen(argv[2], "wb");
    if (!in || !outf) return 3;
    int64_t n = 0;
    if (fread(&n, 8, 1, in) != 1) return 4;
    for (int64_t c = 0; c < n; ++c) {
        int64_t hd[3];
        double par[2];
        if (fread(hd, 8, 3, in) != 3 || fread(par, 8, 2, in) != 2) return 5;
        const int64_t T = hd[0], K = hd[1];
        std::vector<float> kp(T * 3 * K), out(T * 3 * K, -12345.0f);
        std::vector<uint8_t> flag(T * K, 0xEE);
        if ((int64_t)fread(kp.data(), 4, kp.size(), in) != (int64_t)kp.size()) return 6;
        reject(kp.data(), T, K, (int32_t)hd[2], par[0], par[1], out.data(), flag.data());
        fwrite(out.data(), 4, out.size(), outf);
        fwrite(flag.data(), 1, flag.size(), outf);
    }
    fclose(outf);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return hs.build_cpu_program(tmp_path_factory, "outlier", _PROGRAM, "-O2")


@pytest.mark.parametrize("h", oc.HS)
def test_rule_on_the_cpu_equals_the_reference(program, tmp_path, h):
    """Every case of the GPU test with this half-width, one run of the program."""
    from stac_mjx_amd import prep

    assert prep.TILE_FRAMES == TILE
    cases = [c for c in oc.cases(TILE) if c[1] == h]
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.int64(len(cases)).tobytes())
        for name, h_, T, K, min_dev in cases:
            kp, _, _ = oc.reference(name, h_, T, K, TILE, min_dev)
            fh.write(np.array([T, K, h_], np.int64).tobytes())
            fh.write(np.array([oc.THR, min_dev], np.float64).tobytes())
            fh.write(kp.tobytes())
    res = subprocess.run([str(program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    raw = (tmp_path / "out.bin").read_bytes()
    pos = 0
    for name, h_, T, K, min_dev in cases:
        kp, want_out, want_flag = oc.reference(name, h_, T, K, TILE, min_dev)
        out = np.frombuffer(raw, np.float32, T * 3 * K, pos).reshape(T, 3 * K)
        pos += 4 * T * 3 * K
        flag = np.frombuffer(raw, np.uint8, T * K, pos).reshape(T, K)
        pos += T * K
        oc.check(out, flag, kp, want_out, want_flag, label=f"{name} h={h_} T={T} K={K} min_dev={min_dev}")
    assert pos == len(raw)


def test_the_cases_hold_what_they_are_meant_to():
    T, K = 2 * TILE + 1, 2
    assert oc.shapes_T(5, TILE) == [1, 2, 5, 6, 11, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5 * TILE + 7]
    assert len(oc.PATTERNS) == 14 and {c[3] for c in oc.cases(TILE)} == set(oc.KS) and {c[1] for c in oc.cases(TILE)} == set(oc.HS)
    for h in oc.HS:
        flag = lambda name, min_dev=0.0: oc.reference(name, h, T, K, TILE, min_dev)[2]  # noqa: E731
        f = flag("spikes_at_edges_and_tile_borders")
        if h > 1:  # every spike on an edge of the series or of a tile is found (h = 1: a window of two at the edges decides nothing)
            assert f[[0, T - 1, TILE - 1, TILE]].all(), h
        else:
            assert not f[[0, T - 1]].any()
        assert not flag("all_nan").any()
        kp, out, f = oc.reference("nan_in_one_coordinate", h, T, K, TILE, 0.0)
        x, o = kp.reshape(T, K, 3), out.reshape(T, K, 3)
        assert np.isnan(x[0, 0, 1]) and f[0, 0] == 0 and o[0, 0, 0].view(np.uint32) == x[0, 0, 0].view(np.uint32)
        kp = oc.reference("infinite_coordinates", h, T, K, TILE, 0.0)[0]
        assert np.isposinf(kp).any() and np.isneginf(kp).any()
        # a still marker: with min_dev = 0 every frame that differs in the last bit goes, with the floor only the real spike
        f0, f1 = flag("constant", 0.0), flag("constant", 0.01)
        assert f0[2].all() and f0[T // 2].all() and f1[T // 2].all() and f1.sum() == K, (h, f0.sum(), f1.sum())
        kp = oc.reference("spikes_next_to_nan_runs", h, T, K, TILE, 0.0)[0]
        valid = np.isfinite(kp.reshape(T, K, 3)).all(axis=2)[:, 0]
        n = np.array([valid[max(0, t - h):t + h + 1].sum() for t in range(T) if valid[t]])
        assert (n < 3).any() and (n[n >= 3] % 2 == 1).any() and (h == 1 or (n[n >= 3] % 2 == 0).any()), h  # (h = 1: n is 3 at most)
    kp = oc.reference("denormals", 5, T, K, TILE, 0.0)[0]
    assert (np.abs(kp[kp != 0]) < 1.2e-38).all()
    kp = oc.reference("ties_and_signed_zeros", 5, T, K, TILE, 0.0)[0]
    assert np.signbit(kp[kp == 0]).any() and not np.signbit(kp[kp == 0]).all()
    assert np.abs(oc.reference("magnitudes_of_1e30", 5, T, K, TILE, 0.0)[0]).max() > 1e38


def test_known_limit_a_run_longer_than_h_is_not_rejected():
    """h wrong frames in a row are each a minority of their window and go; of h + 1 the middle ones are the majority and stay."""
    for h in (5, 16):
        T = 6 * h
        x = np.zeros((T, 3), np.float32)
        x[:, 0] = np.linspace(0, 0.01, T)
        a, b = x.copy(), x.copy()
        a[2 * h:3 * h] += np.float32(0.5)
        b[2 * h:3 * h + 1] += np.float32(0.5)
        fa = oc.reference_reject(a, h, oc.THR, 0.001)[1][:, 0]
        fb = oc.reference_reject(b, h, oc.THR, 0.001)[1][:, 0]
        assert fa[2 * h:3 * h].all() and fa.sum() == h
        assert not fb[2 * h:3 * h + 1].all()


def test_recall_every_injected_spike_and_nothing_else():
    """A condition on the test's inputs (verified on the CPU): a slow movement (5 cm sinusoids of 330 - 1000 frames, at most 1 mm per
    frame) plus white noise of 0.2 mm, and single-frame spikes of 3 - 9 cm in one coordinate at known places at least 13 frames
    apart.  The reference with the default parameters (half-width 5, 3 sigma, floor 1 mm) flags exactly the spiked keypoints: a
    spike is 30 and more times the window's MAD (at most about 3 mm from the movement); a noise sample would have to lie 1 mm = 5 sigma
    from its window's median to pass the floor, and the series is seeded."""
    from stac_mjx_amd.config import OUTLIER_DEFAULTS

    T, K = 400, 6
    rng = np.random.default_rng(2024)
    t = np.arange(T, dtype=np.float64)[:, None, None]
    x = (rng.uniform(-0.3, 0.3, (1, K, 3)) + 0.05 * np.sin(2 * np.pi * rng.uniform(0.001, 0.003, (1, K, 3)) * t + rng.uniform(0, 6.28, (1, K, 3)))
         + 0.0002 * rng.standard_normal((T, K, 3))).astype(np.float32)
    want = np.zeros((T, K), np.uint8)
    for k in range(K):
        for f in rng.choice(np.arange(0, T, 13), size=8, replace=False):  # (frames 0 and 13 * 30 = 390 can be among them)
            x[f, k, rng.integers(0, 3)] += np.float32(rng.choice((-1.0, 1.0)) * rng.uniform(0.03, 0.09))
            want[f, k] = 1
    _, flag = oc.reference_reject(x.reshape(T, 3 * K), OUTLIER_DEFAULTS["outlier_window"], OUTLIER_DEFAULTS["outlier_nsigma"] * 1.4826,
                                  OUTLIER_DEFAULTS["outlier_min_dev"])
    assert want.sum() == 8 * K
    np.testing.assert_array_equal(flag, want)


# ---- config -----------------------------------------------------------------------------------------------------------------------
def test_config_reject_outliers_keys(rodent_cfg):
    from stac_mjx_amd import prep
    from stac_mjx_amd.config import OUTLIER_MAX_WINDOW
    from stac_mjx_amd.main import _reject_outliers_mode

    plain = hs.stage_cfg(rodent_cfg)
    assert _reject_outliers_mode(plain)[0] == "off" and "outlier" not in plain.to_yaml()  # absent stays absent
    assert _reject_outliers_mode(hs.stage_cfg(rodent_cfg, reject_outliers="off"))[0] == "off"
    assert _reject_outliers_mode(hs.stage_cfg(rodent_cfg, reject_outliers=False))[0] == "off"  # what YAML 1.1 makes of a bare `off`
    mode, args = _reject_outliers_mode(hs.stage_cfg(rodent_cfg, reject_outliers="hampel", fill_missing="linear"))
    assert mode == "hampel" and args == {"half_window": 5, "n_sigma": 3.0, "min_dev": 0.001}  # the defaults
    mode, args = _reject_outliers_mode(hs.stage_cfg(rodent_cfg, reject_outliers="hampel", fill_missing="hold", outlier_window=16,
                                            outlier_nsigma=2, outlier_min_dev=0))
    assert mode == "hampel" and args == {"half_window": 16, "n_sigma": 2.0, "min_dev": 0.0}
    assert OUTLIER_MAX_WINDOW == prep.MAX_HALF_WINDOW == 16
    header = (ROOT / "stac_mjx_amd" / "csrc" / "stac_outlier.hpp").read_text()
    assert f"kOutlierMaxHalf = {prep.MAX_HALF_WINDOW};" in header
    bad = [dict(reject_outliers="on"), dict(reject_outliers="Hampel"), dict(reject_outliers=True), dict(reject_outliers=1),
           dict(outlier_window=0), dict(outlier_window=17), dict(outlier_window=-1), dict(outlier_window=2.5), dict(outlier_window="5"),
           dict(outlier_window=True), dict(outlier_nsigma=-1.0), dict(outlier_nsigma=float("nan")), dict(outlier_nsigma=float("inf")),
           dict(outlier_nsigma="3"), dict(outlier_min_dev=-0.001), dict(outlier_min_dev=float("inf")), dict(outlier_min_dev=None)]
    for over in bad:
        with pytest.raises(ValueError):
            _reject_outliers_mode(hs.stage_cfg(rodent_cfg, fill_missing="linear", **over))
        cfg = hs.stage_cfg(rodent_cfg, fill_missing="linear")  # also when the key is set after validation: the run reads the caller's config
        cfg.stac.update(over)
        with pytest.raises(ValueError):
            _reject_outliers_mode(cfg)
    with pytest.raises(ValueError):
        hs.stage_cfg(rodent_cfg, outlier_windw=5)  # an unknown key stays an error
    for fill in ({}, dict(fill_missing="off")):  # the solver cannot take the NaNs
        with pytest.raises(ValueError, match="fill_missing"):
            _reject_outliers_mode(hs.stage_cfg(rodent_cfg, reject_outliers="hampel", **fill))


def test_run_stac_refuses_rejecting_without_filling_before_any_work(tmp_path, rodent_cfg):
    from stac_mjx_amd.main import run_stac

    cfg = hs.stage_cfg(rodent_cfg, reject_outliers="hampel")
    with pytest.raises(ValueError, match="fill_missing"):  # before the model is even looked for: the path does not exist
        run_stac(cfg, np.zeros((4, 6), np.float32), ["a", "b"], base_path=tmp_path / "nowhere")
    assert not list(tmp_path.iterdir())


# ---- C ABI and wrapper ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return hs.loaded_library()


def test_reject_argument_errors_need_no_device(lib):
    """Every pointer below is a fake non-NULL address: a call that got past its checks would fault, not return."""
    T, K = 100, 23
    kp, out, flag = 0x100000, 0x200000, 0x300000
    p = C.c_void_p

    def call(kp=kp, T=T, K=K, h=5, thr=oc.THR, min_dev=0.0, out=out, flag=flag):
        rc = lib.stac_prep_reject(p(kp) if kp else None, T, K, h, thr, min_dev, p(out) if out else None, p(flag) if flag else None, None)
        msg = lib.stac_last_error().decode()
        assert rc == STAC_ERR_INVALID and lib.stac_last_error_code() == STAC_ERR_INVALID and "stac_prep_reject" in msg, (rc, msg)
        return msg

    for null in ("kp", "out", "flag"):
        call(**{null: 0})
    for bad in (dict(T=0), dict(T=-3), dict(K=0), dict(K=-1)):
        call(**bad)
    for h in (0, -1, 17, 1000):
        assert str(h) in call(h=h)
    for v in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        call(thr=v)
        call(min_dev=v)
    call(kp=kp + 2)   # 4-byte alignment of the arrays
    call(out=out + 1)
    kp_bytes, flag_bytes = T * K * 12, T * K
    assert "overlap" in call(out=kp)  # in place
    call(out=kp + kp_bytes - 4)
    call(kp=out + kp_bytes - 4)
    call(flag=kp)
    call(flag=out + kp_bytes - 1)
    call(out=flag - kp_bytes + 4)


def test_python_wrapper_refuses_what_it_cannot_run():
    import torch

    from stac_mjx_amd import prep

    with pytest.raises(ValueError):
        prep.reject_outliers(torch.zeros(4, 6))  # a host tensor
    for bad in (dict(half_window=0), dict(half_window=17), dict(half_window=2.0), dict(n_sigma=-1), dict(n_sigma=float("nan")),
                dict(min_dev=-1e-9), dict(min_dev=float("inf")), dict(n_sigma=1.5e308)):
        with pytest.raises(ValueError):
            prep.outlier_params(**{**dict(half_window=5, n_sigma=3.0, min_dev=0.0), **bad})
    assert prep.outlier_params(5, 3.0, 0.0) == (5, oc.THR, 0.0) and oc.THR == 3.0 * 1.4826


# ---- kp_rejected through the result files -----------------------------------------------------------------------------------------
def _data(n, with_rejected, seed=0):
    from stac_mjx_amd.io import StacData

    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    d = StacData(qpos=f(n, 5), xpos=f(n, 2, 3), xquat=f(n, 2, 4), marker_sites=f(n, 3, 3), offsets=f(3, 3), kp_data=f(n, 9),
                 names_qpos=["a", "b"], names_xpos=["w", "v"], kp_names=["k0", "k1", "k2"])
    if with_rejected:
        d.kp_rejected = (rng.random((n, 3)) < 0.3).astype(np.uint8)
        d.kp_gap = d.kp_rejected.astype(np.int32) * 2
    return d


TODAY = {"config", "kp_names", "names_qpos", "names_xpos", "kp_data", "marker_sites", "offsets", "qpos", "qvel", "xpos", "xquat"}


def test_kp_rejected_round_trip_and_old_files(tmp_path, rodent_cfg):
    from stac_mjx_amd import io

    cfg = hs.stage_cfg(rodent_cfg)
    assert io.StacData.__dataclass_fields__["kp_rejected"] is list(io.StacData.__dataclass_fields__.values())[-1]  # a trailing field
    assert "kp_rejected" not in _data(4, False).as_dict() and set(_data(4, True).as_dict()) - set(_data(4, False).as_dict()) == {"kp_gap", "kp_rejected"}
    for suffix in hs.result_suffixes():
        for with_rejected in (False, True):
            d = _data(6, with_rejected)
            path = io.save_data_to_h5(config=cfg, file_path=tmp_path / f"r{int(with_rejected)}{suffix}", **d.as_dict())
            assert path.suffix == suffix
            # without the option: exactly today's datasets, which is also what a file from before this field looks like
            assert hs.dataset_names(path) == (TODAY | {"kp_gap", "kp_rejected"} if with_rejected else TODAY)
            _, back = io.load_stac_data(path)
            if with_rejected:
                assert back.kp_rejected.dtype == np.uint8 and back.kp_rejected.shape == (6, 3)
                np.testing.assert_array_equal(back.kp_rejected, d.kp_rejected)
                np.testing.assert_array_equal(back.kp_gap, d.kp_gap)
            else:
                assert isinstance(back.kp_rejected, np.ndarray) and back.kp_rejected.size == 0
            np.testing.assert_array_equal(back.qpos, d.qpos)
        # a file with kp_gap alone (written by a run with fill_missing only) loads with an empty kp_rejected
        d = _data(6, True)
        only_gap = {k: v for k, v in d.as_dict().items() if k != "kp_rejected"}
        path = io.save_data_to_h5(config=cfg, file_path=tmp_path / f"g{suffix}", **only_gap)
        assert hs.dataset_names(path) == TODAY | {"kp_gap"}
        back = io.load_stac_data(path)[1]
        assert back.kp_rejected.size == 0 and np.array_equal(back.kp_gap, d.kp_gap)


def test_kp_rejected_shard_concatenation(tmp_path, rodent_cfg):
    from stac_mjx_amd import io
    from stac_mjx_amd.dist import shard_range

    cfg = hs.stage_cfg(rodent_cfg)
    F, world = 2, 3
    for with_rejected in (True, False):
        full = _data(5 * F, with_rejected, seed=3)
        ik = tmp_path / f"ik{int(with_rejected)}.npz"
        manifest = io.write_manifest(io.manifest_path(ik), ik, world, 5, F)
        for r in range(world):
            lo, hi = shard_range(5, r, world)
            part = {k: (v[lo * F:hi * F] if isinstance(v, np.ndarray) and v.shape[:1] == (5 * F,) else v) for k, v in full.as_dict().items()}
            io.save_data_to_h5(config=cfg, file_path=io.shard_path(ik, r, world), **part)
        _, back = io.load_sharded_stac_data(manifest)
        np.testing.assert_array_equal(back.qpos, full.qpos)
        if with_rejected:
            assert back.kp_rejected.dtype == np.uint8
            np.testing.assert_array_equal(back.kp_rejected, full.kp_rejected)
        else:
            assert back.kp_rejected.size == 0
