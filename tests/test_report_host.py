"""The fit report, the parts that need no GPU: the ``stac.report`` config keys, the argument checks of the two entry points (they happen
before the device is touched), the workspace query, ``summarize`` on hand-made inputs, and the passes of csrc/stac_report.hip stated
on the CPU from csrc/stac_report.hpp with small tile sizes against the numpy reference of tests/report_cases.py."""

import ctypes as C
import json
import math
import subprocess

import numpy as np
import pytest

import report_cases as rc
import host_scaffold as hs
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    return hs.loaded_library()


# ---- config ------------------------------------------------------------------------------------------------------------------
def test_config_report_keys(rodent_cfg):
    from stac_mjx_amd.config import ConfigError
    from stac_mjx_amd.main import _report_mode

    plain = hs.stage_cfg(rodent_cfg)
    assert _report_mode(plain) == (False, (500, 900, 990), 10)
    assert "report" not in plain.to_yaml()  # absent stays absent (the three keys all hold the word)
    for value, on in (("off", False), ("on", True), (False, False), (True, True)):  # the bools: what YAML 1.1 makes of a bare off / on
        assert _report_mode(hs.stage_cfg(rodent_cfg, report=value))[0] is on
    assert _report_mode(hs.stage_cfg(rodent_cfg, report="on", report_quantiles=[0, 1000], report_worst=0)) == (True, (0, 1000), 0)
    assert _report_mode(hs.stage_cfg(rodent_cfg, report_quantiles=list(range(8))))[1] == tuple(range(8))
    for bad in ("yes", "On", 1, 0, "", 2.0, ["on"]):
        with pytest.raises(ConfigError):
            hs.stage_cfg(rodent_cfg, report=bad)
    for bad in ([], list(range(9)), [500.0], [-1], [1001], [True], "500", 500, None, [[500]]):
        with pytest.raises(ConfigError):
            hs.stage_cfg(rodent_cfg, report_quantiles=bad)
    for bad in (-1, 1.5, "3", True, None, [3]):
        with pytest.raises(ConfigError):
            hs.stage_cfg(rodent_cfg, report_worst=bad)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_workspace_query(lib):
    from stac_mjx_amd import report

    for N, K, Q in ((0, 23, 3), (-5, 23, 3), (10, 0, 3), (10, -1, 3), (10, 23, 0), (10, 23, 9), (10, 23, -1)):
        hs.invalid(lib, lib.stac_report_workspace(N, K, Q))
    tile = report.TILE_FRAMES
    for K in (1, 23, 70):
        for Q in (1, 3, 8):
            last = 0
            for N in (1, tile - 1, tile, tile + 1, 10 * tile, 1_000_000, 2**40):
                b = lib.stac_report_workspace(N, K, Q)
                assert b == report.workspace_formula(N, K, Q) and b % 8 == 0 and b >= last  # (ties the Python constants to the library)
                last = b
                assert report.workspace_bytes(N, K, Q) == b
                assert lib.stac_report_workspace(N, K + 1, Q) > b  # monotone in K
                if Q < report.MAX_QUANT:
                    assert lib.stac_report_workspace(N, K, Q + 1) > b  # and in Q
            assert lib.stac_report_workspace(tile + 1, K, Q) > lib.stac_report_workspace(tile, K, Q)
    hs.invalid(lib, lib.stac_report_workspace(2**62, 2**30, 3))  # beyond int64
    header = (ROOT / "stac_mjx_amd" / "csrc" / "stac_report.hpp").read_text()
    for name, value in (("kReportTileFrames", report.TILE_FRAMES), ("kReportMaxBlocks", report.MAX_BLOCKS), ("kReportSegFrames", report.SEG_FRAMES),
                        ("kReportMaxQuant", report.MAX_QUANT), ("kReportBins0", report.HIST_BINS)):
        assert f"{name} = {value};" in header, name
    from stac_mjx_amd import config

    assert config.REPORT_MAX_QUANTILES == report.MAX_QUANT and tuple(config.REPORT_DEFAULTS["report_quantiles"]) == report.DEFAULT_PERMILLE


NAMES = ("markers", "kp", "gap", "sqerr", "frame_sse", "frame_n", "count", "sum", "max", "argmax", "hist", "quant", "workspace")


def test_report_argument_errors_need_no_device(lib):
    """Every pointer below is a fake non-NULL address: a call that got past its checks would fault, not return."""
    from stac_mjx_amd import report

    N, K, Q = 100, 23, 3
    need = lib.stac_report_workspace(N, K, Q)
    base = {name: 0x10000000 * (i + 1) for i, name in enumerate(NAMES)}
    size = dict(markers=N * K * 12, kp=N * K * 12, gap=N * K * 4, sqerr=N * K * 4, frame_sse=N * 8, frame_n=N * 4, count=K * 8, sum=K * 8,
                max=K * 4, argmax=K * 8, hist=K * 1024 * 8, quant=K * Q * 4, workspace=need)

    def call(N=N, K=K, Q=Q, permille=(500, 900, 990), nbytes=need, null_permille=False, **ptr):
        a = dict(base)
        a.update(ptr)
        perm = (C.c_int32 * max(len(permille), 1))(*permille)
        p = report.Params(n_frames=N, n_kp=K, n_quant=Q, permille=None if null_permille else perm, workspace_bytes=nbytes, stream=None,
                          **{k: (v or None) for k, v in a.items()})
        return lib.stac_report_errors(C.byref(p))

    assert "stac_report_errors" in hs.invalid(lib, lib.stac_report_errors(None))
    for null in NAMES:
        if null != "gap":
            assert "stac_report_errors" in hs.invalid(lib, call(**{null: 0}))
    hs.invalid(lib, call(null_permille=True))
    for kw in (dict(N=0), dict(N=-3), dict(K=0), dict(K=-1), dict(Q=0), dict(Q=9), dict(Q=-1)):
        assert "stac_report_errors" in hs.invalid(lib, call(**kw))
    for bad in ((500, 900, 1001), (-1, 900, 990), (500, 2**20, 990)):
        assert "permille" in hs.invalid(lib, call(permille=bad))
    assert str(need) in hs.invalid(lib, call(nbytes=need - 1))  # the message names the size it needs
    hs.invalid(lib, call(nbytes=0))
    hs.invalid(lib, call(workspace=base["workspace"] + 4))  # 8-byte alignment of the workspace
    for name in ("markers", "kp", "gap", "sqerr", "frame_n", "max", "quant"):
        assert name in hs.invalid(lib, call(**{name: base[name] + 2}))  # 4-byte alignment of the arrays
    for name in ("frame_sse", "count", "sum", "argmax", "hist"):
        assert name in hs.invalid(lib, call(**{name: base[name] + 4}))  # 8-byte alignment of the 64-bit outputs
    # any two buffers that overlap: the same array, a partial overlap at either end
    for a in NAMES:
        for b in NAMES:
            if a == b:
                continue
            msg = hs.invalid(lib, call(**{a: base[b]}))
            assert "overlap" in msg and a in msg and b in msg, (a, b, msg)
            hs.invalid(lib, call(**{a: base[b] + size[b] - 8}))
            if size[a] > 8:
                hs.invalid(lib, call(**{a: base[b] - size[a] + 8}))


def test_python_wrapper_refuses_what_it_cannot_run():
    import torch

    from stac_mjx_amd import report

    with pytest.raises(ValueError):
        report.fit_errors(torch.zeros(4, 2, 3), torch.zeros(4, 6))  # host tensors
    for bad in ((), list(range(9)), (500.0,), (1001,), (-1,), (True,), "500", 500):
        with pytest.raises(ValueError):
            report.check_permille(bad)
    assert report.check_permille([0, np.int64(1000)]) == (0, 1000)


# ---- summarize -----------------------------------------------------------------------------------------------------------------
def _hand_made():
    N, K, Q = 6, 3, 3
    f32 = lambda *v: np.array(v, np.float32)  # noqa: E731
    hist = np.zeros((K, 1024), np.int64)
    res = {
        "sqerr": np.zeros((N, K), np.float32),
        "frame_sse": np.array([4.0, 9.0, 9.0, 0.5, 100.0, 9.0]),
        "frame_n": np.array([3, 2, 2, 1, 0, 2], np.int32),  # frame 4 has the largest sum and no counted keypoint
        "count": np.array([6, 4, 0], np.int64),
        "sum": np.array([24.0, 1.0, 0.0]),
        "max": f32(16.0, 0.25, np.nan),
        "argmax": np.array([2, 5, -1], np.int64),
        "hist": hist,
        "quant": np.array([[4.0, 9.0, 16.0], [0.0625, 0.25, 0.25], [np.nan] * 3], np.float32),
    }
    for k, values in ((0, (1.0, 1.0, 4.0, 4.0, 9.0, 16.0)), (1, (0.0625, 0.0625, 0.25, 0.25))):
        for v in values:
            hist[k, np.array([v], np.float32).view(np.uint32)[0] >> 21] += 1
    return res


def test_summarize_roots_ties_and_uncounted_frames():
    from stac_mjx_amd import report

    s = report.summarize(_hand_made(), ["a", "b", "c"], worst=3)
    a, b, c = (s["keypoints"][n] for n in "abc")
    assert a == {"n": 6, "rms": 2.0, "max": 4.0, "quantiles": [2.0, 3.0, 4.0], "argmax_frame": 2, "not_counted": 0.0}
    assert b["rms"] == 0.5 and b["max"] == 0.5 and b["quantiles"] == [0.25, 0.5, 0.5] and b["not_counted"] == pytest.approx(1 / 3)
    assert c == {"n": 0, "rms": None, "max": None, "quantiles": [None, None, None], "argmax_frame": -1, "not_counted": 1.0}
    o = s["overall"]
    assert o["n"] == 10 and o["rms"] == math.sqrt(25.0 / 10) and o["max"] == 4.0 and o["not_counted"] == pytest.approx(1 - 10 / 18)
    # merged histogram, ranks (p * 9) // 1000 = 4, 8, 8 of {1/16, 1/16, 1/4, 1/4, 1, 1, 4, 4, 9, 16}: the lower edges of their bins
    assert o["quantiles"] == [1.0, math.sqrt(8.0), math.sqrt(8.0)]  # (9 lies in the bin [8, 10))
    assert report.bin_lower_edge(np.array([9.0], np.float32).view(np.uint32)[0] >> 21) == 8.0
    assert o["frame_sse_mean"] == pytest.approx((4 + 9 + 9 + 0.5 + 9) / 5) and o["frame_sse_max"] == 9.0
    # the three frames of sum 9 tie: lower frames first; frame 4 (frame_n == 0) is not listed although its sum is the largest
    assert s["worst_frames"] == [{"frame": 1, "frame_sse": 9.0, "frame_n": 2}, {"frame": 2, "frame_sse": 9.0, "frame_n": 2},
                                 {"frame": 5, "frame_sse": 9.0, "frame_n": 2}]
    assert [w["frame"] for w in report.summarize(_hand_made(), "abc", worst=10)["worst_frames"]] == [1, 2, 5, 0, 3]
    assert report.summarize(_hand_made(), "abc", worst=0)["worst_frames"] == []
    assert json.loads(json.dumps(s)) == s  # plain types only: the JSON round-trips
    assert len(report.table_lines(s)) == 3 and len(report.overall_lines(s)) == 2
    with pytest.raises(ValueError):
        report.summarize(_hand_made(), ["a", "b"])
    with pytest.raises(ValueError):
        report.summarize(_hand_made(), "abc", permille=(500,))
    with pytest.raises(ValueError):
        report.summarize(_hand_made(), "abc", worst=-1)


def test_report_path_is_next_to_the_result_file(tmp_path):
    from stac_mjx_amd import io
    from stac_mjx_amd.main import report_path

    p = report_path(tmp_path / "fit.h5")
    assert p.parent == tmp_path and p.name == io.resolve_output_path(tmp_path / "fit.h5").name + ".report.json"


# ---- the passes on the CPU, from the kernels' header, with any tile size -----------------------------------------------------------
_PROGRAM = r"""
// The passes of csrc/stac_report.hip, run serially with a tile of any size up to 64, on the functions of stac_report.hpp.
// usage: prog TILE IN OUT.  IN: int64 n, then per case int64 N, K, Q, has_gap, Q int32 permille, N * 3K floats markers, N * 3K floats
// kp, has_gap * N * K int32.  OUT: per case sqerr, frame_sse, frame_n, count, sum, max, argmax, hist, quant.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "stac_report.hpp"
using namespace stac;

struct Out {
    std::vector<float> sqerr, max, quant;
    std::vector<double> frame_sse, sum;
    std::vector<int32_t> frame_n;
    std::vector<int64_t> count, argmax, hist;
};

static void report(const float *m, const float *y, const int32_t *gap, int64_t N, int64_t K, int Q, const int32_t *permille, int64_t tile, Out &o) {
    const int64_t tiles = (N + tile - 1) / tile;
    std::vector<uint32_t> keys(K * N);
    std::vector<double> psum(K * tiles, 0.0);
    std::vector<uint64_t> pmax(K * tiles, 0);
    for (int64_t i = 0; i < tiles; ++i)  // the first pass, tile by tile
        for (int64_t t = i * tile; t < (i + 1) * tile && t < N; ++t) {
            double sse = 0.0;
            int32_t n = 0;
            for (int64_t k = 0; k < K; ++k) {
                const int64_t at = t * K + k;
                const ReportPair p = report_pair(m[3 * at], m[3 * at + 1], m[3 * at + 2], y[3 * at], y[3 * at + 1], y[3 * at + 2], gap ? gap[at] : 0);
                o.sqerr[at] = p.sqerr;
                keys[k * N + t] = p.key;
                if (p.counted) {
                    sse = sse + p.e;
                    ++n;
                    psum[k * tiles + i] = psum[k * tiles + i] + p.e;
                    const uint64_t w = report_pack(p.key, (int)(t - i * tile));
                    if (w > pmax[k * tiles + i]) pmax[k * tiles + i] = w;
                }
            }
            o.frame_sse[t] = sse;
            o.frame_n[t] = n;
        }
    std::vector<ReportSel> sel(K * Q);
    for (int pass = 0; pass < 3; ++pass) {
        const int bins = report_bins(pass), slots = pass == 0 ? 1 : Q;
        std::vector<uint64_t> h(K * slots * bins, 0);
        for (int64_t k = 0; k < K; ++k)  // a counting pass
            for (int64_t t = 0; t < N; ++t)
                for (int q = 0; q < slots; ++q) {
                    const uint32_t key = keys[k * N + t];
                    if (report_match(pass, key, pass == 0 ? 0u : sel[k * Q + q].prefix)) ++h[(k * slots + q) * bins + report_digit(pass, key)];
                }
        for (int64_t k = 0; k < K; ++k) {  // its finishing step
            if (pass == 0) {
                double s = 0.0;
                uint64_t best = 0, c = 0;
                int64_t best_tile = -1;
                for (int64_t i = 0; i < tiles; ++i) {
                    s = s + psum[k * tiles + i];
                    if (report_tile_wins(best, best_tile, pmax[k * tiles + i], i)) best = pmax[k * tiles + i], best_tile = i;
                }
                for (int b = 0; b < bins; ++b) o.hist[k * bins + b] = (int64_t)h[k * bins + b], c += h[k * bins + b];
                o.count[k] = (int64_t)c;
                o.sum[k] = s;
                o.max[k] = report_float(c ? (uint32_t)(best >> 32) : kReportNanBits);
                o.argmax[k] = c ? best_tile * tile + (kReportTileFrames - (int64_t)(best & 0xFFFFFFFFull)) : -1;
            }
            for (int q = 0; q < Q; ++q) {
                ReportSel &r = sel[k * Q + q];
                if (pass == 0) {
                    r.prefix = kReportNoKey, r.rank = 0, r.pad = 0;
                    if (o.count[k] == 0) {
                        o.quant[k * Q + q] = report_float(kReportNanBits);
                        continue;
                    }
                    report_select(&h[k * bins], bins, (uint64_t)report_rank(permille[q], o.count[k]), &r.prefix, &r.rank);
                    continue;
                }
                if (r.prefix == kReportNoKey) continue;
                uint32_t d;
                uint64_t in;
                report_select(&h[(k * Q + q) * bins], bins, r.rank, &d, &in);
                if (pass == 1) r.prefix = (r.prefix << 11) | d, r.rank = in;
                else o.quant[k * Q + q] = report_float((r.prefix << 10) | d);
            }
        }
    }
}

template <class T> static bool rd(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <class T> static void wr(FILE *f, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const int64_t tile = atoll(argv[1]);
    FILE *in = fopen(argv[2], "rb"), *outf = fopen(argv[3], "wb");
    if (!in || !outf || tile < 1 || tile > kReportTileFrames) return 3;
    int64_t n = 0;
    if (fread(&n, 8, 1, in) != 1) return 4;
    for (int64_t c = 0; c < n; ++c) {
        int64_t h[4];
        if (fread(h, 8, 4, in) != 4) return 5;
        const int64_t N = h[0], K = h[1], Q = h[2];
        if (report_layout(N, K, Q).bytes < 0) return 7;
        std::vector<int32_t> permille(Q), gap(h[3] ? N * K : 0);
        std::vector<float> m(N * K * 3), y(N * K * 3);
        if (!rd(in, permille) || !rd(in, m) || !rd(in, y) || !rd(in, gap)) return 6;
        Out o;
        o.sqerr.assign(N * K, -12345.0f), o.max.assign(K, -12345.0f), o.quant.assign(K * Q, -12345.0f);
        o.frame_sse.assign(N, -7.0), o.sum.assign(K, -7.0), o.frame_n.assign(N, -7);
        o.count.assign(K, -7), o.argmax.assign(K, -7), o.hist.assign(K * kReportBins0, -7);
        report(m.data(), y.data(), h[3] ? gap.data() : nullptr, N, K, (int)Q, permille.data(), tile, o);
        wr(outf, o.sqerr), wr(outf, o.frame_sse), wr(outf, o.frame_n), wr(outf, o.count), wr(outf, o.sum), wr(outf, o.max);
        wr(outf, o.argmax), wr(outf, o.hist), wr(outf, o.quant);
    }
    fclose(outf);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return hs.build_cpu_program(tmp_path_factory, "report", _PROGRAM, "-O1")


def _read_outputs(raw, pos, N, K, Q):
    out = {}
    for name, dtype, shape in (("sqerr", np.float32, (N, K)), ("frame_sse", np.float64, (N,)), ("frame_n", np.int32, (N,)),
                               ("count", np.int64, (K,)), ("sum", np.float64, (K,)), ("max", np.float32, (K,)), ("argmax", np.int64, (K,)),
                               ("hist", np.int64, (K, 1024)), ("quant", np.float32, (K, Q))):
        n = int(np.prod(shape))
        out[name] = np.frombuffer(raw, dtype, n, pos).reshape(shape)
        pos += n * np.dtype(dtype).itemsize
    return out, pos


@pytest.mark.parametrize("tile", [1, 2, 4, 7])
def test_passes_on_the_cpu_equal_the_reference(program, tmp_path, tile):
    """Every case of the GPU test (its shapes come from the kernel's tile; the borders of this run's tiles fall elsewhere), one run
    of the program."""
    from stac_mjx_amd import report

    cases = rc.all_cases(report.TILE_FRAMES)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.int64(len(cases)).tobytes())
        for name, N, K, Q in cases:
            m, kp, gap, permille, _ = rc.reference(name, N, K, report.TILE_FRAMES, Q)
            fh.write(np.array([N, K, Q, gap is not None], np.int64).tobytes())
            fh.write(np.array(permille, np.int32).tobytes())
            fh.write(m.tobytes())
            fh.write(kp.tobytes())
            if gap is not None:
                fh.write(gap.tobytes())
    res = subprocess.run([str(program), str(tile), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    raw = (tmp_path / "out.bin").read_bytes()
    pos = 0
    for name, N, K, Q in cases:
        want = rc.reference(name, N, K, report.TILE_FRAMES, Q)[4]
        got, pos = _read_outputs(raw, pos, N, K, Q)
        rc.check(got, want, label=f"tile={tile} {name} N={N} K={K} Q={Q}")
    assert pos == len(raw)


def test_the_cases_hold_what_they_are_meant_to():
    """The patterns at the kernel's tile size and the largest shape of the GPU test."""
    from stac_mjx_amd import report

    tile = report.TILE_FRAMES
    N, K = 5 * tile + 7, 23
    ref = lambda name, Q=3, N=N, K=K: rc.reference(name, N, K, tile, Q)  # noqa: E731
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
    assert sorted(rc.n_quant_of(name, k) for k in rc.KS for name in rc.PATTERNS[:1]) == [1, 1, 3, 8]  # every set is met
    assert all(0 in rc.PERMILLE[q] or q == 1 for q in rc.PERMILLE) and all(1000 in p for p in rc.PERMILLE.values())
    for arrays in (ref("random")[:3], ref("random")[4].values()):
        assert not any(a.flags.writeable for a in arrays)
    w = ref("zero_residual")[4]
    assert not bits(w["sqerr"]).any() and not bits(w["quant"]).any() and not w["argmax"].any() and (w["count"] == N).all()
    assert (w["hist"][:, 0] == N).all()
    m, kp, gap, _, w = ref("one_counted")
    assert (w["count"] == 1).all() and [int(a) for a in w["argmax"][:3]] == [0, N // 2, N - 1]
    assert (bits(w["quant"]) == bits(w["max"])[:, None]).all() and np.isnan(kp).any() and (gap > 0).any()
    m, kp, gap, _, w = ref("none_counted")
    assert w["count"][0] == 0 and w["count"][K - 1] == 0 and (w["count"][1:K - 1] == N).all()
    assert (bits(w["max"])[[0, K - 1]] == rc.NAN_BITS).all() and (w["argmax"][[0, K - 1]] == -1).all()
    assert (bits(w["quant"])[[0, K - 1]] == rc.NAN_BITS).all() and not w["hist"][[0, K - 1]].any()
    assert (bits(w["sqerr"])[:, 0] == rc.NAN_BITS).all() and np.isfinite(w["sqerr"][:, K - 1]).all()  # the gapped one is still written
    m, kp, gap, _, w = ref("nonfinite_each_slot")
    y = kp.reshape(N, K, 3)
    for a in (m, y):
        for c in range(3):
            assert np.isnan(a[..., c]).any() and np.isposinf(a[..., c]).any() and np.isneginf(a[..., c]).any()
    assert (bits(w["sqerr"]) == rc.NAN_BITS).sum() == 18 and w["count"].sum() == N * K - 18
    m, kp, gap, _, w = ref("gap_excluded")
    assert (w["sqerr"][gap > 0] > 0.5).all() and (w["max"] < 1e-3).all() and (gap > 0).sum() > N * K // 20
    for name, shift in (("low_bits_only", 10), ("mid_bits_only", 21)):
        w = ref(name)[4]
        b = bits(w["sqerr"])
        assert len(np.unique(b >> shift)) == 1 and len(np.unique(b[:, 0])) > N // 4
    assert len(np.unique(bits(ref("mid_bits_only")[4]["sqerr"]) >> 10)) > 100
    w = ref("exponent_spread")[4]
    b = bits(w["sqerr"])
    assert ((b > 0) & (b < 0x00800000)).any() and (b == 0x7F800000).any() and w["hist"][:, 1020].all()  # denormals and +inf
    assert (w["hist"].sum(axis=0) > 0).sum() > 300 and not w["hist"][:, 1021:].any()
    assert np.isfinite(w["sum"]).all() and np.isinf(w["max"]).all()  # e itself stays finite in double
    m, kp, gap, permille, w = ref("rank_inside_a_tie")
    assert permille == (0, 500, 1000) and [float(v) for v in w["quant"][0]] == [0.25, 2.25, 6.25]
    n3 = N // 3
    assert (N - 1) // 2 not in (n3, 2 * n3 - 1) and n3 < (N - 1) // 2 < 2 * n3 - 1  # the middle of the run; 0 and N - 1 are a first and a last
    w = ref("argmax_tie")[4]
    for k in (0, 1):
        frames = rc.tie_frames(N, tile, k)
        assert len({t // tile for t in frames}) == 3 and w["argmax"][k] == frames[0]
        assert (bits(w["sqerr"])[frames, k] == bits(w["max"])[k]).all()
    m, kp, gap, _, w = ref("random")
    rms = np.sqrt(w["sum"] / w["count"])
    assert (0.0012 < rms).all() and (rms < 0.0023).all() and (gap > 0).any()  # sqrt(3) mm
