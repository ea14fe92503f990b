"""fill_missing, the parts that need no GPU: the ``stac.fill_missing`` config key, the argument checks of the two entry points (they
happen before the device is touched), the staged scan of csrc/stac_prep.hip stated on the CPU from csrc/stac_prep.hpp with small
tile sizes against the numpy reference of tests/prep_cases.py, ``kp_gap`` through the result files, and the mask of ``viz_stac``."""

import ctypes as C
import subprocess

import numpy as np
import pytest

import prep_cases as pc
import host_scaffold as hs
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    return hs.loaded_library()


# ---- config ------------------------------------------------------------------------------------------------------------------
def test_config_fill_missing_key(rodent_cfg):
    from stac_mjx_amd.config import ConfigError
    from stac_mjx_amd.main import _fill_missing_mode

    plain = hs.stage_cfg(rodent_cfg)
    assert _fill_missing_mode(plain) == "off" and "fill_missing" not in plain.to_yaml()  # absent stays absent
    for mode in ("off", "linear", "hold"):
        assert _fill_missing_mode(hs.stage_cfg(rodent_cfg, fill_missing=mode)) == mode
    assert _fill_missing_mode(hs.stage_cfg(rodent_cfg, fill_missing=False)) == "off"  # what YAML 1.1 makes of a bare `off`
    for bad in ("on", "Linear", "cubic", True, 1, 0, "", None):
        with pytest.raises(ConfigError):
            hs.stage_cfg(rodent_cfg, fill_missing=bad)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_workspace_query(lib):
    from stac_mjx_amd import prep

    for T, K in ((0, 23), (-5, 23), (10, 0), (10, -1)):
        hs.invalid(lib, lib.stac_prep_fill_workspace(T, K))
    tile = prep.TILE_FRAMES
    for K in (1, 23, 70):
        last = 0
        for T in (1, tile - 1, tile, tile + 1, 10 * tile, 1_000_000, 2**40):
            b = lib.stac_prep_fill_workspace(T, K)
            assert b == 32 * K * ((T + tile - 1) // tile) and b % 8 == 0 and b >= last  # (ties the Python constant to the library)
            last = b
            assert prep.workspace_bytes(T, K) == b
            assert lib.stac_prep_fill_workspace(T, K + 1) > b  # monotone in K as well
    hs.invalid(lib, lib.stac_prep_fill_workspace(2**62, 2**30))  # beyond int64
    header = (ROOT / "stac_mjx_amd" / "csrc" / "stac_prep.hpp").read_text()
    assert f"kPrepTileFrames = {prep.TILE_FRAMES};" in header and f"kPrepMaxBlocks = {prep.MAX_BLOCKS};" in header


def test_fill_argument_errors_need_no_device(lib):
    """Every pointer below is a fake non-NULL address: a call that got past its checks would fault, not return."""
    T, K = 100, 23
    need = lib.stac_prep_fill_workspace(T, K)
    kp, out, gap, ws = 0x100000, 0x200000, 0x300000, 0x400000
    p = C.c_void_p

    def call(kp=kp, T=T, K=K, mode=0, out=out, gap=gap, ws=ws, nbytes=need):
        return lib.stac_prep_fill(p(kp) if kp else None, T, K, mode, p(out) if out else None, p(gap) if gap else None,
                                  p(ws) if ws else None, nbytes, None)

    for null in ("kp", "out", "gap", "ws"):
        hs.invalid(lib, call(**{null: 0}))
    hs.invalid(lib, call(T=0))
    hs.invalid(lib, call(T=-3))
    hs.invalid(lib, call(K=0))
    hs.invalid(lib, call(K=-1))
    for mode in (-1, 2, 7):
        assert str(mode) in hs.invalid(lib, call(mode=mode))
    assert str(need) in hs.invalid(lib, call(nbytes=need - 1))  # the message names the size it needs
    hs.invalid(lib, call(nbytes=0))
    hs.invalid(lib, call(ws=ws + 4))   # 8-byte alignment of the workspace
    hs.invalid(lib, call(kp=kp + 2))   # 4-byte alignment of the arrays
    # aliased buffers: the same array, a partial overlap at either end, the workspace inside an output
    kp_bytes, gap_bytes = T * K * 12, T * K * 4
    assert "overlap" in hs.invalid(lib, call(out=kp))
    hs.invalid(lib, call(out=kp + kp_bytes - 4))
    hs.invalid(lib, call(kp=out + kp_bytes - 4))
    hs.invalid(lib, call(gap=kp))
    hs.invalid(lib, call(gap=out + 8))
    hs.invalid(lib, call(ws=gap + gap_bytes - 8))
    hs.invalid(lib, call(ws=kp + 8))
    hs.invalid(lib, call(out=ws - kp_bytes + 8))


def test_python_wrapper_refuses_what_it_cannot_run():
    import torch

    from stac_mjx_amd import prep

    with pytest.raises(ValueError):
        prep.fill_missing(torch.zeros(4, 6), "linear")  # a host tensor
    with pytest.raises(ValueError):
        prep.fill_missing(torch.zeros(4, 6), "cubic")
    g = np.array([[0, 3, 2], [2, 3, 2], [2, 3, 0]], np.int32)
    s = prep.summary(g)
    np.testing.assert_array_equal(s["missing"], [2, 3, 2])
    np.testing.assert_array_equal(s["longest"], [2, 3, 2])
    assert s["empty"] == [1]
    s = prep.summary(np.zeros((5, 2), np.int32))
    assert s["empty"] == [] and not s["missing"].any() and not s["longest"].any()


# ---- the staged scan on the CPU, from the kernels' header, with any tile size ----------------------------------------------------
_PROGRAM = r"""
// The three stages of csrc/stac_prep.hip, run serially with a tile of any size, on the functions of stac_prep.hpp.
// usage: prog TILE IN OUT.  IN: int64 n, then per case int64 T, K, mode and T * 3K floats.  OUT: per case T * 3K floats, T * K int32.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "stac_prep.hpp"
using namespace stac;

static void fill(const float *kp, int64_t T, int64_t K, int mode, int64_t tile, float *out, int32_t *gap) {
    const int64_t tiles = prep_tiles(T, tile), K3 = 3 * K;
    std::vector<PrepSummary> sum(K * tiles);
    std::vector<int64_t> prev(K * tiles), next(K * tiles);
    auto missing = [&](int64_t t, int64_t k) { const float *s = kp + t * K3 + 3 * k; return prep_missing(s[0], s[1], s[2]); };
    for (int64_t i = 0; i < tiles; ++i)  // 1: tile summaries
        for (int64_t k = 0; k < K; ++k) {
            PrepSummary s = prep_none();
            for (int64_t t = i * tile; t < (i + 1) * tile && t < T; ++t)
                if (!missing(t, k)) s = prep_combine(s, PrepSummary{t, t});
            sum[k * tiles + i] = s;
        }
    for (int64_t k = 0; k < K; ++k) {  // 2: carries over the tiles
        PrepSummary run = prep_none();
        for (int64_t i = 0; i < tiles; ++i) {
            prev[k * tiles + i] = run.last;
            run = prep_combine(run, sum[k * tiles + i]);
        }
        run = prep_none();
        for (int64_t i = tiles - 1; i >= 0; --i) {
            next[k * tiles + i] = run.first;
            run = prep_combine(sum[k * tiles + i], run);
        }
    }
    for (int64_t i = 0; i < tiles; ++i)  // 3: fill
        for (int64_t t = i * tile; t < (i + 1) * tile && t < T; ++t)
            for (int64_t k = 0; k < K; ++k) {
                const float *s = kp + t * K3 + 3 * k;
                float *o = out + t * K3 + 3 * k;
                int32_t g = 0;
                o[0] = s[0], o[1] = s[1], o[2] = s[2];
                if (missing(t, k)) {
                    int64_t p = -1, n = -1;
                    for (int64_t u = t - 1; u >= i * tile && p < 0; --u)
                        if (!missing(u, k)) p = u;
                    for (int64_t u = t + 1; u < (i + 1) * tile && u < T && n < 0; ++u)
                        if (!missing(u, k)) n = u;
                    if (p < 0) p = prev[k * tiles + i];
                    if (n < 0) n = next[k * tiles + i];
                    g = prep_gap(p, n, T);
                    if (p >= 0 || n >= 0) {
                        const float *a = kp + (p >= 0 ? p : n) * K3 + 3 * k, *b = kp + (n >= 0 ? n : p) * K3 + 3 * k;
                        for (int c = 0; c < 3; ++c) o[c] = prep_fill(mode, t, p, n, a[c], b[c]);
                    }
                }
                gap[t * K + k] = g;
            }
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const int64_t tile = atoll(argv[1]);
    FILE *in = fopen(argv[2], "rb"), *outf = fopen(argv[3], "wb");
    if (!in || !outf || tile < 1) return 3;
    int64_t n = 0;
    if (fread(&n, 8, 1, in) != 1) return 4;
    for (int64_t c = 0; c < n; ++c) {
        int64_t h[3];
        if (fread(h, 8, 3, in) != 3) return 5;
        const int64_t T = h[0], K = h[1];
        std::vector<float> kp(T * 3 * K), out(T * 3 * K, -12345.0f);
        std::vector<int32_t> gap(T * K, -7);
        if ((int64_t)fread(kp.data(), 4, kp.size(), in) != (int64_t)kp.size()) return 6;
        fill(kp.data(), T, K, (int)h[2], tile, out.data(), gap.data());
        fwrite(out.data(), 4, out.size(), outf);
        fwrite(gap.data(), 4, gap.size(), outf);
    }
    fclose(outf);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return hs.build_cpu_program(tmp_path_factory, "prep", _PROGRAM, "-O1")


@pytest.mark.parametrize("tile", [1, 2, 4, 7])
def test_staged_scan_on_the_cpu_equals_the_reference(program, tmp_path, tile):
    """Every case of the GPU test at this tile size (borders placed by it), both modes, one run of the program."""
    from stac_mjx_amd import prep

    cases = [(name, T, K, mode) for mode in pc.MODES for T in pc.shapes_T(tile) for K in pc.KS for name in pc.PATTERNS]
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.int64(len(cases)).tobytes())
        for name, T, K, mode in cases:
            kp, _, _ = pc.reference(name, T, K, tile, mode)
            fh.write(np.array([T, K, prep.MODES[mode]], np.int64).tobytes())
            fh.write(kp.tobytes())
    res = subprocess.run([str(program), str(tile), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    raw = (tmp_path / "out.bin").read_bytes()
    pos = 0
    for name, T, K, mode in cases:
        kp, want_out, want_gap = pc.reference(name, T, K, tile, mode)
        out = np.frombuffer(raw, np.float32, T * 3 * K, pos).reshape(T, 3 * K)
        pos += 4 * T * 3 * K
        gap = np.frombuffer(raw, np.int32, T * K, pos).reshape(T, K)
        pos += 4 * T * K
        pc.check(out, gap, kp, want_out, want_gap, label=f"tile={tile} {name} T={T} K={K} {mode}")
    assert pos == len(raw)


def test_the_cases_hold_what_they_are_meant_to():
    """The patterns at the kernel's tile size: runs on the borders they name, a tie, every kind of run and of missing value."""
    from stac_mjx_amd import prep

    tile, T, K = prep.TILE_FRAMES, 5 * prep.TILE_FRAMES + 7, 23
    gap = lambda name, mode="linear": pc.reference(name, T, K, tile, mode)[2]  # noqa: E731
    assert not gap("none").any()
    g = gap("empty_track")
    assert (g[:, K // 2] == T).all() and not g[:, K // 2 - 1].any() and not g[:, K // 2 + 1].any()
    for name, t in (("single_valid_start", 0), ("single_valid_end", T - 1)):
        g = gap(name)[:, 0]
        assert g[t] == 0 and (np.delete(g, t) == T - 1).all()
    g = gap("single_valid_middle")[:, K - 1]
    assert g[T // 2] == 0 and (g[: T // 2] == T // 2).all() and (g[T // 2 + 1:] == T - 1 - T // 2).all()
    g = gap("run_ends_on_last_frame_of_tile")[:, 0]
    assert g[tile - 1] == 3 and g[tile] == 0 and g[tile - 4] == 0
    g = gap("run_starts_on_first_frame_of_tile")[:, 0]
    assert g[tile] == 3 and g[tile - 1] == 0 and g[tile + 3] == 0
    g = gap("run_over_three_tiles")[:, 0]
    assert g[tile - 1] == 0 and (g[tile:4 * tile + 3] == 3 * tile + 3).all() and g[4 * tile + 3] == 0
    g = gap("alternating")
    assert (g[1::2, 0] == 1).all() and not g[0::2, 0].any() and g[0, K - 1] == 1 and g[T - 1, K - 1] == 1
    kp, out, g = pc.reference("only_y_nan", T, K, tile, "linear")
    x = kp.reshape(T, K, 3)
    assert g[1, 0] == 1 and np.isfinite(x[1, 0, 0]) and np.isnan(x[1, 0, 1]) and out.reshape(T, K, 3)[1, 0, 0] != x[1, 0, 0]
    kp = pc.reference("infinities", T, K, tile, "linear")[0]
    assert np.isposinf(kp).any() and np.isneginf(kp).any() and not np.isnan(kp).any()
    kp, out, g = pc.reference("hold_tie", T, K, tile, "hold")
    assert (g[1:4, 0] == 3).all() and np.array_equal(out[2, :3], kp[0, :3]) and np.array_equal(out[3, :3], kp[4, :3])
    lin = pc.reference("hold_tie", T, K, tile, "linear")[1]
    assert not np.array_equal(lin[2, :3], kp[0, :3])
    g = gap("random_30_percent")
    assert 0.25 < np.count_nonzero(g) / g.size < 0.35


# ---- kp_gap through the result files ---------------------------------------------------------------------------------------------
def _data(n, with_gap, seed=0):
    from stac_mjx_amd.io import StacData

    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    d = StacData(qpos=f(n, 5), xpos=f(n, 2, 3), xquat=f(n, 2, 4), marker_sites=f(n, 3, 3), offsets=f(3, 3), kp_data=f(n, 9),
                 names_qpos=["a", "b"], names_xpos=["w", "v"], kp_names=["k0", "k1", "k2"])
    if with_gap:
        d.kp_gap = rng.integers(0, 4, (n, 3)).astype(np.int32)
    return d


TODAY = {"config", "kp_names", "names_qpos", "names_xpos", "kp_data", "marker_sites", "offsets", "qpos", "qvel", "xpos", "xquat"}


def test_kp_gap_round_trip(tmp_path, rodent_cfg):
    from stac_mjx_amd import io

    cfg = hs.stage_cfg(rodent_cfg)
    assert "kp_gap" not in _data(4, False).as_dict() and set(_data(4, True).as_dict()) - set(_data(4, False).as_dict()) == {"kp_gap"}
    for suffix in hs.result_suffixes():
        for with_gap in (False, True):
            d = _data(6, with_gap)
            path = io.save_data_to_h5(config=cfg, file_path=tmp_path / f"r{int(with_gap)}{suffix}", **d.as_dict())
            assert path.suffix == suffix
            assert hs.dataset_names(path) == (TODAY | {"kp_gap"} if with_gap else TODAY)  # without the option: exactly today's datasets
            _, back = io.load_stac_data(path)
            if with_gap:
                assert back.kp_gap.dtype == np.int32
                np.testing.assert_array_equal(back.kp_gap, d.kp_gap)
            else:
                assert isinstance(back.kp_gap, np.ndarray) and back.kp_gap.size == 0
            np.testing.assert_array_equal(back.qpos, d.qpos)
            np.testing.assert_array_equal(back.kp_data, d.kp_data)


def test_kp_gap_shard_concatenation(tmp_path, rodent_cfg):
    from stac_mjx_amd import io

    cfg = hs.stage_cfg(rodent_cfg)
    F, world = 2, 3
    for with_gap in (True, False):
        full = _data(5 * F, with_gap, seed=3)
        ik = tmp_path / f"ik{int(with_gap)}.npz"
        manifest = io.write_manifest(io.manifest_path(ik), ik, world, 5, F)
        for r in range(world):
            from stac_mjx_amd.dist import shard_range

            lo, hi = shard_range(5, r, world)
            part = {k: (v[lo * F:hi * F] if isinstance(v, np.ndarray) and v.shape[:1] == (5 * F,) else v) for k, v in full.as_dict().items()}
            io.save_data_to_h5(config=cfg, file_path=io.shard_path(ik, r, world), **part)
        _, back = io.load_sharded_stac_data(manifest)
        np.testing.assert_array_equal(back.qpos, full.qpos)
        if with_gap:
            np.testing.assert_array_equal(back.kp_gap, full.kp_gap)
        else:
            assert back.kp_gap.size == 0


# ---- viz_stac hands filled keypoints to the renderer as NaN ------------------------------------------------------------------------
def test_viz_stac_masks_filled_keypoints(tmp_path, rodent_cfg, monkeypatch):
    from stac_mjx_amd import io, stac as stac_mod, viz

    seen = {}

    class FakeStac:
        def __init__(self, xml_path, cfg, kp_names):
            pass

        def render(self, qposes, kp_data, *a, **k):
            seen["kp"] = np.array(kp_data)
            return ["frame"]

    monkeypatch.setattr(stac_mod, "Stac", FakeStac)
    cfg = hs.stage_cfg(rodent_cfg)
    d = _data(6, True, seed=5)
    d.kp_gap = np.zeros((6, 3), np.int32)
    d.kp_gap[1:3, 0] = 2
    d.kp_gap[5, 2] = 1
    path = io.save_data_to_h5(config=cfg, file_path=tmp_path / "ik.npz", **d.as_dict())
    _, frames = viz.viz_stac(path, 6, tmp_path / "v.avi", base_path=tmp_path)
    assert frames == ["frame"]
    want = d.kp_data.reshape(6, 3, 3).copy()
    want[d.kp_gap > 0] = np.nan
    np.testing.assert_array_equal(seen["kp"], want.reshape(6, 9))  # (NaN equals NaN here)
    assert np.isnan(seen["kp"]).sum() == 9 and np.isfinite(d.kp_data).all()
    viz.viz_stac(path, 6, tmp_path / "v.avi", base_path=tmp_path, show_filled=True)
    np.testing.assert_array_equal(seen["kp"], d.kp_data)
    # a file without kp_gap: what render gets is the file's kp_data
    plain = _data(6, False, seed=6)
    path = io.save_data_to_h5(config=cfg, file_path=tmp_path / "plain.npz", **plain.as_dict())
    viz.viz_stac(path, 6, tmp_path / "v.avi", base_path=tmp_path)
    np.testing.assert_array_equal(seen["kp"], plain.kp_data)
