"""repair_swaps, the parts that need no GPU: the numpy reference of tests/swaps_cases.py against its vectorised statement and against
the rule of csrc/stac_swap.hpp as a stand-alone CPU program (once more under the address and undefined-behaviour sanitizers), what the
reference does with the 40-frame left / right swaps in the golden recording, the config keys and ``config.lr_pairs``, the pre-flight
refusals of ``run_stac``, the argument checks of ``stac_prep_swaps`` (they happen
before the device is touched) and ``kp_swapped`` through the result files."""

import ctypes as C
import json
import subprocess

import numpy as np
import pytest

import pairwise_cases as pc
import swaps_cases as sc
import host_scaffold as hs
from conftest import GOLDEN, ROOT
from host_scaffold import STAC_ERR_INVALID, STAC_ERR_CAPACITY


# ---- the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", sc.KS)
def test_the_reference_the_tests_share_is_the_plain_loop_reference(K):
    """``swaps_cases.reference`` decides all frames of a candidate at once; the loop per candidate and frame of ``reference_swaps``
    gives the same bits on every case."""
    for name, T, _ in sc.cases(ks=(K,)):
        kp, cand, thr, min_dev, min_bad, want = sc.reference(name, T, K)
        sc.check(sc.reference_swaps(kp, cand, thr, min_dev, min_bad), kp, cand, want, label=f"{name} T={T} K={K}")


def test_the_cases_hold_what_they_are_meant_to():
    assert sc.TS == (1, 2, 3, 63, 64, 65, 129, 1000) and sc.KS == (2, 3, 4, 5, 23, 64)
    cases = sc.cases()
    assert {(T, K) for _, T, K in cases} == {(T, K) for T in sc.TS for K in sc.KS}  # every shape of the grid
    for name, (_, t_min, k_min) in sc.PATTERNS.items():  # every pattern at every shape it fits
        assert {(T, K) for n, T, K in cases if n == name} == {(T, K) for T in sc.TS for K in sc.KS if T >= t_min and K >= k_min}, name
        assert t_min <= 5 and k_min <= 3
    assert [c for c in cases if c[0] == "ties"] == [("ties", 129, 5), ("ties", 1000, 23)]
    for T, K in ((129, 5), (1000, 23)):  # the decision's edge, both sides (make_case asserts it too)
        kp, cand, thr, min_dev, min_bad, want = sc.reference("ties", T, K)
        b0, b1 = sc.reference_swaps_all_frames(kp, cand, thr, min_dev, min_bad, counts=True)[5:]
        on, off = (2 * b1 == b0) & (b0 > 0), 2 * b1 == b0 + 1
        assert on.any() and off.any() and (want[1][on] == 1).all() and (want[1][off] == 0).all()
    for K in sc.KS:
        T = 129
        ref = lambda name: sc.reference(name, T, K)  # noqa: E731
        kp, cand, _, _, min_bad, (out, flag, n, med, mad) = ref("no_defect")
        assert len(cand) == K // 2 and min_bad == 3 and flag.shape == (T, K // 2) and flag.sum() == 0 and (n == T).all()
        np.testing.assert_array_equal(out.view(np.uint32), kp.view(np.uint32))
        kp, cand, _, _, _, (out, flag, _, _, _) = ref("swaps")
        assert len(cand) == K // 2 and len({k for ab in cand for k in ab}) == 2 * (K // 2) and (K < 64 or len(cand) == 32)
        (a, b), = ref("one_reversed")[1]
        assert (a, b) == (K - 1, K - 2) and a > b
        kp, cand, _, _, _, (out, flag, n, _, _) = ref("no_candidates")
        assert cand == [] and flag.shape == (T, 0) and n.shape == (K * (K - 1) // 2,)
        np.testing.assert_array_equal(out.view(np.uint32), kp.view(np.uint32))
        assert ref("min_bad_1")[4] == 1 and ref("min_bad_largest")[4] == max(2 * (K - 2), 1) and ref("min_bad_never")[4] == 2 * (K - 2) + 1
        assert ref("min_bad_never")[5][1].sum() == 0  # no frame has more than 2 (K - 2) counts
        if K == 2:  # no third keypoint: nothing counts, whatever min_bad
            for name in sc.PATTERNS:
                if sc.PATTERNS[name][2] <= 2:
                    assert ref(name)[5][1].sum() == 0, name
            continue
        if K == 4:  # DESIGN.md §15, what it does not catch: two candidates and nothing else cannot tell which pair is exchanged
            continue
        if K == 3:  # one third keypoint: two counts at most, below the default min_bad of 3
            assert ref("swaps")[5][1].sum() == 0 and ref("min_bad_1")[5][1].sum() > 5 and ref("min_bad_largest")[5][1].sum() > 5
            continue
        flag = ref("swaps")[5][1]
        assert flag.sum() > 0.05 * flag.size                     # (the cases do swap)
        assert ref("one_reversed")[5][1].sum() > 5 and ref("min_bad_1")[5][1].sum() > 5
        assert ref("min_bad_largest")[5][1].sum() > 0             # every one of the 2 (K - 2) distances is bad in some frame
        # swaps in the frames 63, 64, 65 and in the last one, and only there
        flag = ref("tile_edges")[5][1]
        S = flag.shape[1]
        assert all(flag[t, i % S] == 1 for i, t in enumerate((63, 64, 65, T - 1))) and flag.sum() == 4
        kp = ref("swaps_missing")[0]
        assert np.isnan(kp).any() and np.isposinf(kp).any() and np.isneginf(kp).any() and ref("swaps_missing")[5][1].sum() > 0
        # a candidate with a missing keypoint does not swap
        kp, cand, _, _, _, (out, flag, _, _, _) = ref("swaps_missing")
        present = np.isfinite(kp.reshape(T, K, 3)).all(axis=2)
        for s, (a, b) in enumerate(cand):
            assert not flag[~(present[:, a] & present[:, b]), s].any()
        n = ref("pair_counts")[5][2]
        assert [n[pc.pair_index(a, b, K)] for a, b in ((0, 1), (0, 2), (1, 2))] == [0, 2, 3]
        kp, _, _, _, _, (_, _, n, _, _) = ref("huge")
        assert np.isfinite(kp).all() and n[pc.pair_index(0, K - 1, K)] < T
        _, _, _, min_dev, _, (_, flag, _, _, mad) = ref("identical")
        assert (mad == 0).all() and min_dev > 0 and flag[T // 2, 0] == 1 and flag[T // 3, -1] == 1 and flag.sum() == 2
        # -0.0 and denormals move with their keypoint, bit for bit
        kp, cand, _, _, _, (out, flag, _, _, _) = ref("zeros_and_denormals")
        rows = flag[:, 0] == 1
        x, o = kp.reshape(T, K, 3).view(np.uint32), out.reshape(T, K, 3).view(np.uint32)
        assert cand[0] == (0, 1) and rows.sum() > 5
        moved = o[rows, 0]  # what sits at keypoint 0 after the repair: the words that the input had at keypoint 1
        np.testing.assert_array_equal(moved, x[rows, 1])
        assert (np.abs(out.reshape(T, K, 3)[:, :2, 1:]) < 1.2e-38).any() and (o[:, :2, 0] == 0x80000000).any()
    # T < 3 decides nothing
    for name, T, K in cases:
        if T < 3:
            kp, _, _, _, _, (out, flag, _, _, _) = sc.reference(name, T, K)
            assert flag.sum() == 0
            np.testing.assert_array_equal(out.view(np.uint32), kp.view(np.uint32))


# ---- the rule on the CPU, from the kernel's header ----------------------------------------------------------------------------------
_PROGRAM = r"""
// The rule of csrc/stac_swap.hpp run serially, by the passes of the kernels: the keys of every pair, the two middle order statistics
// by the three histogram passes of stac_report.hpp, the same again over the keys of the deviations, then per frame and candidate
// (unpacked from the table that swap_pack makes, as the kernel unpacks it) swap_count over the third keypoints and swap_decide.
// usage: prog IN OUT.  IN: int64 n, then per case int64 T, K, S, min_bad, double thr, min_dev, 2 S int32 and T * 3K floats.
// OUT: per case T * 3K floats, T * S bytes, P int64, P doubles, P doubles.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "stac_swap.hpp"
using namespace stac;

static uint32_t select_rank(const std::vector<uint32_t> &keys, uint64_t rank) {
    uint32_t prefix = 0;
    for (int pass = 0; pass < 3; ++pass) {
        std::vector<uint64_t> hist(report_bins(pass), 0);
        for (uint32_t key : keys)
            if (report_match(pass, key, prefix)) ++hist[report_digit(pass, key)];
        uint32_t d;
        uint64_t inside;
        report_select(hist.data(), report_bins(pass), rank, &d, &inside);
        prefix = pass == 0 ? d : (pass == 1 ? (prefix << 11) | d : (prefix << 10) | d);
        rank = inside;
    }
    return prefix;
}

static uint64_t count(const std::vector<uint32_t> &keys) {
    uint64_t n = 0;
    for (uint32_t key : keys) n += report_match(0, key, 0u) ? 1 : 0;
    return n;
}

static void run(const float *kp, int64_t T, int64_t K, const int32_t *cand, int32_t S, double thr, double min_dev, int32_t min_bad, float *out,
                uint8_t *flag, int64_t *pair_n, double *pair_med, double *pair_mad) {
    const PairwiseLayout L = pairwise_layout(T, K);
    if (L.bytes < 0 || L.pairs != pairwise_pairs(K)) exit(7);
    SwapCands packed;
    int32_t at = -1;
    if (swap_pack(cand, S, (int32_t)K, &packed, &at) != 0) exit(9);
    const int64_t P = L.pairs, K3 = 3 * K;
    std::vector<std::vector<uint32_t>> keys(P, std::vector<uint32_t>(T));
    for (int64_t a = 0; a + 1 < K; ++a)
        for (int64_t b = a + 1; b < K; ++b) {
            const int64_t p = pairwise_index(a, b, K);
            for (int64_t t = 0; t < T; ++t) {
                const float *r = kp + t * K3;
                keys[p][t] = pairwise_key(r[3 * a], r[3 * a + 1], r[3 * a + 2], r[3 * b], r[3 * b + 1], r[3 * b + 2]);
            }
            const uint64_t n = count(keys[p]);
            pair_n[p] = (int64_t)n;
            pair_med[p] = pair_mad[p] = pairwise_nan64();
            if (n < 3) continue;
            pair_med[p] = pairwise_median(report_float(select_rank(keys[p], (n - 1) / 2)), report_float(select_rank(keys[p], n / 2)));
            std::vector<uint32_t> dev(T);
            for (int64_t t = 0; t < T; ++t) dev[t] = pairwise_dev_key(keys[p][t], pair_med[p]);
            if (count(dev) != n) exit(8);
            pair_mad[p] = pairwise_median(report_float(select_rank(dev, (n - 1) / 2)), report_float(select_rank(dev, n / 2)));
        }
    memcpy(out, kp, sizeof(float) * T * K3);
    for (int64_t t = 0; t < T; ++t)
        for (int32_t s = 0; s < S; ++s) {
            const uint32_t c = (uint32_t)(packed.w[s >> 2] >> (16 * (s & 3))) & 0xFFFFu;
            const int32_t a = (int32_t)(c & 0xFFu), b = (int32_t)(c >> 8);
            if (a != cand[2 * s] || b != cand[2 * s + 1]) exit(10);
            int32_t b0 = 0, b1 = 0;
            for (int32_t k = 0; k < K; ++k) {
                if (k == a || k == b) continue;
                const int64_t pa = swap_pair(a, k, K), pb = swap_pair(b, k, K);
                swap_count(keys[pa][t], keys[pb][t], pair_n[pa], pair_n[pb], pair_med[pa], thr * pair_mad[pa], pair_med[pb], thr * pair_mad[pb],
                           min_dev, &b0, &b1);
            }
            const bool swaps = swap_decide(b0, b1, min_bad);
            flag[t * S + s] = swaps ? 1 : 0;
            if (swaps) {
                memcpy(out + t * K3 + 3 * a, kp + t * K3 + 3 * b, 12);
                memcpy(out + t * K3 + 3 * b, kp + t * K3 + 3 * a, 12);
            }
        }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *outf = fopen(argv[2], "wb");
    if (!in || !outf) return 3;
    int64_t n = 0;
    if (fread(&n, 8, 1, in) != 1) return 4;
    for (int64_t c = 0; c < n; ++c) {
        int64_t hd[4];
        double par[2];
        if (fread(hd, 8, 4, in) != 4 || fread(par, 8, 2, in) != 2) return 5;
        const int64_t T = hd[0], K = hd[1], S = hd[2], P = K * (K - 1) / 2;
        std::vector<int32_t> cand(2 * S + 1);
        if ((int64_t)fread(cand.data(), 4, 2 * S, in) != 2 * S) return 6;
        std::vector<float> kp(T * 3 * K), out(T * 3 * K, -12345.0f);
        std::vector<uint8_t> flag(T * S + 1, 0xEE);
        std::vector<int64_t> pn(P + 1, -7);
        std::vector<double> med(P + 1, -7.0), mad(P + 1, -7.0);
        if ((int64_t)fread(kp.data(), 4, kp.size(), in) != (int64_t)kp.size()) return 6;
        run(kp.data(), T, K, cand.data(), (int32_t)S, par[0], par[1], (int32_t)hd[3], out.data(), flag.data(), pn.data(), med.data(), mad.data());
        fwrite(out.data(), 4, out.size(), outf);
        fwrite(flag.data(), 1, T * S, outf);
        fwrite(pn.data(), 8, P, outf);
        fwrite(med.data(), 8, P, outf);
        fwrite(mad.data(), 8, P, outf);
    }
    fclose(in);
    fclose(outf);
    return 0;
}
"""


def _compile(tmp_path_factory, tag, extra):
    cxx = hs.host_cxx()
    d = tmp_path_factory.mktemp(tag)
    (d / "swaps_cpu.cpp").write_text(_PROGRAM)
    exe = d / "swaps_cpu"
    base = [cxx, "-O2", "-g", "-ffp-contract=off", "-std=c++17", f"-I{ROOT / 'stac_mjx_amd' / 'csrc'}", str(d / "swaps_cpu.cpp"), "-o", str(exe)]
    # (a host compiler without the sanitizers' runtimes builds the plain program, as tests/test_pairwise_host.py does)
    if not extra or subprocess.run(base + extra, capture_output=True, text=True).returncode != 0:
        res = subprocess.run(base, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _compile(tmp_path_factory, "swaps_host", [])


@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    """The same program with the address and undefined-behaviour sanitizers: a stand-alone binary, nothing is loaded into Python"""
    return _compile(tmp_path_factory, "swaps_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run_program(exe, tmp_path, cases):
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.int64(len(cases)).tobytes())
        for name, T, K in cases:
            kp, cand, thr, min_dev, min_bad, _ = sc.reference(name, T, K)
            fh.write(np.array([T, K, len(cand), min_bad], np.int64).tobytes())
            fh.write(np.array([thr, min_dev], np.float64).tobytes())
            fh.write(np.array(cand, np.int32).reshape(-1).tobytes())
            fh.write(kp.tobytes())
    res = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-3000:])
    raw = (tmp_path / "out.bin").read_bytes()
    pos = 0
    for name, T, K in cases:
        kp, cand, _, _, _, want = sc.reference(name, T, K)
        P, S = K * (K - 1) // 2, len(cand)
        got = []
        for dt, shape in ((np.float32, (T, 3 * K)), (np.uint8, (T, S)), (np.int64, (P,)), (np.float64, (P,)), (np.float64, (P,))):
            count = int(np.prod(shape))
            got.append(np.frombuffer(raw, dt, count, pos).reshape(shape))
            pos += count * np.dtype(dt).itemsize
        sc.check(got, kp, cand, want, label=f"{name} T={T} K={K}")
    assert pos == len(raw)


@pytest.mark.parametrize("K", sc.KS)
def test_rule_on_the_cpu_equals_the_reference(program, tmp_path, K):
    """Every case of the GPU test with this many keypoints, one run of the program."""
    _run_program(program, tmp_path, sc.cases(ks=(K,)))


def test_rule_on_the_cpu_under_the_sanitizers(sanitized_program, tmp_path):
    """A handful of cases: the capacity edge with 32 candidates, missing keypoints, no candidate, the smallest shapes, the edge of
    the decision."""
    _run_program(sanitized_program, tmp_path, [("swaps", 129, 64), ("swaps_missing", 65, 23), ("no_candidates", 64, 5), ("swaps", 1, 2),
                                               ("one_reversed", 63, 3), ("pair_counts", 129, 4), ("ties", 129, 5), ("huge", 3, 23)])


# ---- the motivating case -----------------------------------------------------------------------------------------------------------
def test_motivating_swaps_of_40_frames_in_the_golden_recording(rodent_mocap, rodent_cfg):
    """Each of the 9 left / right keypoint pairs of the rodent swapped for 40 consecutive frames (tests/pairwise_cases.py:
    ``swapped_recording``): 360 (frame, candidate) swaps, 720 keypoints.  With the defaults every one is flagged, nothing else is,
    the repaired series is the untouched recording bit for bit, and the untouched recording has no flag at all.  (The reference
    written from the rule gave exactly the figures of the issue's prototype, also for min_bad 2 and 4: DESIGN.md §15.)"""
    from stac_mjx_amd.config import SWAPS_DEFAULTS, lr_pairs

    names = list(rodent_cfg["KEYPOINT_MODEL_PAIRS"].keys())
    cand = lr_pairs(names)
    assert cand == pc.swap_pairs(names) and len(cand) == 9
    mocap = np.ascontiguousarray(rodent_mocap, dtype=np.float32)
    kp, wrong = pc.swapped_recording(mocap, names)
    truth = np.stack([wrong[:, a] & wrong[:, b] for a, b in cand], axis=1)
    assert truth.sum() == 360 and wrong.sum() == 720
    par = (SWAPS_DEFAULTS["swaps_nsigma"] * pc.MAD_TO_SIGMA, SWAPS_DEFAULTS["swaps_min_dev"], SWAPS_DEFAULTS["swaps_min_bad"])
    assert par == (sc.THR, sc.MIN_DEV, sc.MIN_BAD) and par[2] == 3
    table = {}
    for min_bad in (2, 3, 4):
        out, flag = sc.reference_swaps_all_frames(kp, cand, par[0], par[1], min_bad)[:2]
        clean_out, clean = sc.reference_swaps_all_frames(mocap, cand, par[0], par[1], min_bad)[:2]
        table[min_bad] = (int(flag[truth].sum()), int(flag[~truth].sum()), int(clean.sum()))
        if min_bad == 3:
            np.testing.assert_array_equal(flag, truth.astype(np.uint8))                    # all 360, and nothing else
            np.testing.assert_array_equal(out.view(np.uint32), mocap.view(np.uint32))      # the untouched recording, bit for bit
            assert clean.sum() == 0                                                        # the untouched recording: no flag at all
            np.testing.assert_array_equal(clean_out.view(np.uint32), mocap.view(np.uint32))
            rejected = pc.reference_pairwise_all_pairs(out, pc.THR, pc.MIN_DEV, 2)[1].mean()
            untouched = pc.reference_pairwise_all_pairs(mocap, pc.THR, pc.MIN_DEV, 2)[1].mean()
            assert rejected == untouched and abs(untouched - 0.0234) < 0.0001             # reject_pairwise after the repair: 2.34 %
    print("min_bad: (found of 360, false in the swapped recording, false in the untouched one):", table)
    assert table == {2: (360, 37, 0), 3: (360, 0, 0), 4: (360, 0, 0)}


def test_the_96_frames_of_the_end_to_end_run(rodent_mocap, rodent_cfg):
    """What tests/test_gpu_swaps.py runs end to end: the untouched 96 frames have no swap, the first two pairs swapped for 24 frames
    each are found, 48 of 48, and nothing else."""
    from stac_mjx_amd.config import lr_pairs

    names = list(rodent_cfg["KEYPOINT_MODEL_PAIRS"].keys())
    cand = lr_pairs(names)
    clean = np.ascontiguousarray(rodent_mocap[200:296], dtype=np.float32)
    assert sc.reference_swaps_all_frames(clean, cand, sc.THR, sc.MIN_DEV, sc.MIN_BAD)[1].sum() == 0
    kp = clean.copy()
    hit = np.zeros((96, len(cand)), bool)
    hit[20:44, 0] = hit[50:74, 1] = True
    sc.exchange_frames(kp.reshape(96, 23, 3), cand, hit)
    out, flag = sc.reference_swaps_all_frames(kp, cand, sc.THR, sc.MIN_DEV, sc.MIN_BAD)[:2]
    np.testing.assert_array_equal(flag, hit.astype(np.uint8))
    np.testing.assert_array_equal(out.view(np.uint32), clean.view(np.uint32))


# ---- config -----------------------------------------------------------------------------------------------------------------------
def test_config_repair_swaps_keys(rodent_cfg):
    from stac_mjx_amd.config import SWAPS_DEFAULTS, swaps_options
    from stac_mjx_amd.main import _reject_outliers_mode, _reject_pairwise_mode, _repair_swaps_mode

    names = list(rodent_cfg["KEYPOINT_MODEL_PAIRS"].keys())
    plain = hs.stage_cfg(rodent_cfg)
    assert SWAPS_DEFAULTS == {"swaps_nsigma": 6.0, "swaps_min_dev": 0.002, "swaps_min_bad": 3}
    assert swaps_options(plain.stac) == ("off", 6.0, 0.002, 3) and "swaps" not in plain.to_yaml()  # absent stays absent
    assert _repair_swaps_mode(plain, names) == ([], {"n_sigma": 6.0, "min_dev": 0.002, "min_bad": 3})
    assert swaps_options(hs.stage_cfg(rodent_cfg, repair_swaps="off").stac)[0] == "off"
    off = hs.stage_cfg(rodent_cfg, repair_swaps=False)  # what YAML 1.1 makes of a bare `off`
    assert swaps_options(off.stac)[0] == "off" and off.stac.repair_swaps == "off" and _repair_swaps_mode(off, names)[0] == []
    lr = hs.stage_cfg(rodent_cfg, repair_swaps="lr")  # needs no fill_missing: it makes no NaN
    pairs, args = _repair_swaps_mode(lr, names)
    assert pairs == pc.swap_pairs(names) and args == {"n_sigma": 6.0, "min_dev": 0.002, "min_bad": 3}
    named = hs.stage_cfg(rodent_cfg, repair_swaps=[["KneeR", "KneeL"], ["Snout", "TailBase"]], swaps_nsigma=8, swaps_min_dev=0, swaps_min_bad=5)
    pairs, args = _repair_swaps_mode(named, names)
    assert pairs == [(names.index("KneeR"), names.index("KneeL")), (names.index("Snout"), names.index("TailBase"))]
    assert args == {"n_sigma": 8.0, "min_dev": 0.0, "min_bad": 5}
    assert swaps_options(named.stac)[0] == [("KneeR", "KneeL"), ("Snout", "TailBase")]
    # the siblings are untouched
    assert _reject_pairwise_mode(lr) == _reject_pairwise_mode(plain) and _reject_outliers_mode(lr) == _reject_outliers_mode(plain)
    bad = [dict(repair_swaps="on"), dict(repair_swaps="LR"), dict(repair_swaps=True), dict(repair_swaps=1), dict(repair_swaps="mad"),
           dict(repair_swaps=[]), dict(repair_swaps=[["KneeL"]]), dict(repair_swaps=[["KneeL", "KneeR", "HipL"]]),
           dict(repair_swaps=[["KneeL", 3]]), dict(repair_swaps=["KneeL", "KneeR"]), dict(repair_swaps=[["KneeL", ""]]),
           dict(repair_swaps={"KneeL": "KneeR"}), dict(swaps_nsigma=-1.0), dict(swaps_nsigma=float("nan")), dict(swaps_nsigma=float("inf")),
           dict(swaps_nsigma="6"), dict(swaps_nsigma=True), dict(swaps_min_dev=-0.001), dict(swaps_min_dev=float("inf")),
           dict(swaps_min_dev=None), dict(swaps_min_bad=0), dict(swaps_min_bad=-2), dict(swaps_min_bad=3.0), dict(swaps_min_bad="3"),
           dict(swaps_min_bad=True), dict(swaps_min_bad=None), dict(swaps_min_bad=2**31)]
    for over in bad:
        with pytest.raises(ValueError):
            hs.stage_cfg(rodent_cfg, **over)
        cfg = hs.stage_cfg(rodent_cfg)  # also when the key is set after validation: the run reads the caller's config
        cfg.stac.update(over)
        with pytest.raises(ValueError):
            _repair_swaps_mode(cfg, names)
    with pytest.raises(ValueError):
        hs.stage_cfg(rodent_cfg, swaps_nsigm=5)  # an unknown key stays an error
    # what only the keypoint names can say
    for over in (dict(repair_swaps=[["KneeL", "Knee"]]), dict(repair_swaps=[["KneeL", "KneeL"]]),
                 dict(repair_swaps=[["KneeL", "KneeR"], ["HipL", "KneeR"]])):
        with pytest.raises(ValueError):
            _repair_swaps_mode(hs.stage_cfg(rodent_cfg, **over), names)
    with pytest.raises(ValueError, match="left / right"):
        _repair_swaps_mode(lr, ["a", "b", "c"])


def test_lr_pairs_of_the_three_animals(rodent_cfg):
    from stac_mjx_amd.config import lr_pairs

    def names_of(animal):
        with open(GOLDEN / f"{animal}_model_cfg.json") as fh:
            return list(json.load(fh)["KEYPOINT_MODEL_PAIRS"].keys())

    rodent = names_of("rodent")
    assert rodent == list(rodent_cfg["KEYPOINT_MODEL_PAIRS"].keys())
    pairs = lr_pairs(rodent)
    assert pairs == pc.swap_pairs(rodent) and len(pairs) == 9
    assert [(rodent[a], rodent[b]) for a, b in pairs][:3] == [("AnkleL", "AnkleR"), ("EarL", "EarR"), ("ElbowL", "ElbowR")]
    assert "SpineL" in rodent and rodent.index("SpineL") not in {k for ab in pairs for k in ab}  # (no SpineR: no pair)
    mouse = names_of("mouse")
    got = [(mouse[a], mouse[b]) for a, b in lr_pairs(mouse)]
    want = sorted(n for n in mouse if n.endswith("_L"))
    assert got == [(n, n[:-1] + "R") for n in want] and len(got) == 11 and ("Knee_L", "Knee_R") in got and ("Lisfranc_L", "Lisfranc_R") in got
    fly = names_of("fly")
    got = [(fly[a], fly[b]) for a, b in lr_pairs(fly)]
    assert got == [(n, "R" + n[1:]) for n in sorted(n for n in fly if n.startswith("L"))] and len(got) == 15 and got[0] == ("L1A", "R1A")
    for names in (rodent, mouse, fly):  # every keypoint in at most one pair
        ks = [k for ab in lr_pairs(names) for k in ab]
        assert len(ks) == len(set(ks))
    assert lr_pairs(["a", "b"]) == [] and lr_pairs([]) == []
    assert lr_pairs(["LegL", "LegR", "RegL"]) == [(0, 1)]  # the trailing letter first; a keypoint is in one pair only


def test_run_stac_refuses_bad_candidates_before_any_work(tmp_path, rodent_cfg):
    from stac_mjx_amd.main import run_stac

    names = list(rodent_cfg["KEYPOINT_MODEL_PAIRS"].keys())
    kp = np.zeros((4, 69), np.float32)
    for over, what in ((dict(repair_swaps=[["KneeL", "Elbow"]]), "Elbow"), (dict(repair_swaps=[["KneeL", "KneeR"], ["KneeR", "HipL"]]), "two pairs"),
                       (dict(repair_swaps=[["HipL", "HipL"]]), "twice")):
        with pytest.raises(ValueError, match=what):  # before the model is even looked for: the path does not exist
            run_stac(hs.stage_cfg(rodent_cfg, **over), kp, names, base_path=tmp_path / "nowhere")
    with pytest.raises(ValueError, match="left / right"):
        run_stac(hs.stage_cfg(rodent_cfg, repair_swaps="lr"), np.zeros((4, 6), np.float32), ["a", "b"], base_path=tmp_path / "nowhere")
    cfg = hs.stage_cfg(rodent_cfg)
    cfg.stac.swaps_min_bad = 0  # a bad value set after validation
    with pytest.raises(ValueError, match="swaps_min_bad"):
        run_stac(cfg, kp, names, base_path=tmp_path / "nowhere")
    assert not list(tmp_path.iterdir())


# ---- C ABI and wrapper ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return hs.loaded_library()


def test_workspace_is_the_pairwise_workspace(lib):
    for T, K in ((1, 1), (1, 2), (64, 2), (65, 3), (1000, 23), (10**6, 23), (129, 64)):
        assert lib.stac_prep_swaps_workspace(T, K) == lib.stac_prep_pairwise_workspace(T, K) >= 8, (T, K)
    for T, K in ((0, 3), (-1, 3), (5, 0), (5, -2), (2**45, 2)):
        assert lib.stac_prep_swaps_workspace(T, K) == STAC_ERR_INVALID and lib.stac_last_error_code() == STAC_ERR_INVALID
        assert "stac_prep_swaps_workspace" in lib.stac_last_error().decode()
    assert lib.stac_prep_swaps_workspace(5, 65) == STAC_ERR_CAPACITY and lib.stac_last_error_code() == STAC_ERR_CAPACITY


def test_swaps_argument_errors_need_no_device(lib):
    """Every device pointer below is a fake non-NULL address: a call that got past its checks would fault, not return."""
    T, K = 100, 23
    P = K * (K - 1) // 2
    need = lib.stac_prep_swaps_workspace(T, K)
    good = dict(kp=0x100000, T=T, K=K, cand=[(0, 1), (5, 4), (21, 22)], thr=sc.THR, min_dev=0.002, min_bad=3, out=0x200000, flag=0x300000,
                pair_n=0x400000, pair_med=0x500000, pair_mad=0x600000, work=0x10000000, nbytes=need)
    p = lambda a: C.c_void_p(a) if a else None  # noqa: E731

    def call(code=STAC_ERR_INVALID, **over):
        a = {**good, **over}
        cand = a["cand"]
        n_cand = a.get("n_cand", len(cand) if cand is not None else 0)
        table = (C.c_int32 * max(2 * len(cand), 1))(*[v for ab in cand for v in ab]) if cand is not None else None
        rc = lib.stac_prep_swaps(p(a["kp"]), a["T"], a["K"], table, n_cand, a["thr"], a["min_dev"], a["min_bad"], p(a["out"]), p(a["flag"]),
                                 p(a["pair_n"]), p(a["pair_med"]), p(a["pair_mad"]), p(a["work"]), a["nbytes"], None)
        msg = lib.stac_last_error().decode()
        assert rc == code and lib.stac_last_error_code() == code and "stac_prep_swaps" in msg, (over, rc, msg)
        return msg

    for null in ("kp", "out", "flag", "pair_n", "pair_med", "pair_mad", "work"):
        assert "null" in call(**{null: 0})
    assert "null cand" in call(cand=None, n_cand=2)
    for bad in (dict(T=0), dict(T=-3), dict(K=0), dict(K=-1), dict(n_cand=-1), dict(n_cand=-2**31)):
        call(**bad)
    for K_ in (65, 70, 1000):
        assert str(K_) in call(code=STAC_ERR_CAPACITY, K=K_)
    assert "outside" in call(cand=[(0, 23)]) and "outside" in call(cand=[(-1, 3)]) and "outside" in call(cand=[(0, 1), (2, 64)])
    assert "outside" in call(cand=[(3, 2**31 - 1)]) and "outside" in call(cand=[(-2**31, 3)])
    assert "twice" in call(cand=[(0, 1), (7, 7)])
    assert "earlier" in call(cand=[(0, 1), (2, 0)]) and "earlier" in call(cand=[(0, 1), (1, 2)]) and "candidate 2" in call(cand=[(0, 1), (2, 3), (3, 4)])
    for v in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        call(thr=v)
        call(min_dev=v)
    for v in (0, -1, -2**31):
        assert "min_bad" in call(min_bad=v)
    assert str(need) in call(nbytes=need - 1)
    call(nbytes=0)
    call(nbytes=-5)
    for name, align in (("kp", 4), ("out", 4), ("pair_n", 8), ("pair_med", 8), ("pair_mad", 8), ("work", 8)):
        assert "aligned" in call(**{name: good[name] + align // 2})
    kp_bytes = T * K * 12
    assert "overlap" in call(out=good["kp"])  # in place
    call(out=good["kp"] + kp_bytes - 4)
    call(kp=good["out"] + kp_bytes - 4)
    call(flag=good["kp"])
    call(flag=good["out"] + kp_bytes - 1)
    call(out=good["flag"] + 3 * T - 1 - (good["flag"] + 3 * T - 1) % 4)  # the last bytes of flag [T][3]
    call(cand=[], out=good["flag"] + T - 4)                            # no candidate: flag still has T bytes
    call(pair_med=good["pair_n"] + 8 * P - 8)
    call(pair_mad=good["pair_med"])
    call(work=good["out"] + 8)
    call(out=good["work"] + need - 4)
    call(pair_n=good["work"] + 64)


def test_python_wrapper_refuses_what_it_cannot_run():
    import torch

    from stac_mjx_amd import prep

    with pytest.raises(ValueError):
        prep.repair_swaps(torch.zeros(4, 6), [(0, 1)])  # a host tensor
    good = dict(n_sigma=6.0, min_dev=0.002, min_bad=3)
    for bad in (dict(n_sigma=-1), dict(n_sigma=float("nan")), dict(n_sigma="6"), dict(min_dev=-1e-9), dict(min_dev=float("inf")),
                dict(n_sigma=1.5e308), dict(min_bad=0), dict(min_bad=1.0), dict(min_bad=True), dict(min_bad=2**31)):
        with pytest.raises(ValueError):
            prep.swaps_params(**{**good, **bad})
    assert prep.swaps_params(**good) == (sc.THR, 0.002, 3) and sc.THR == 6.0 * 1.4826
    assert prep.swaps_pairs([(0, 1), [3, 2], np.array([4, 5])], 6) == [(0, 1), (3, 2), (4, 5)] and prep.swaps_pairs([], 3) == []
    for bad in ([(0, 0)], [(0, 6)], [(-1, 2)], [(0, 1), (1, 2)], [(0, 1, 2)], [(0.0, 1)], [(True, 2)], [("a", "b")]):
        with pytest.raises(ValueError):
            prep.swaps_pairs(bad, 6)


# ---- kp_swapped through the result files ----------------------------------------------------------------------------------------
def test_kp_swapped_round_trip_and_old_files(tmp_path, rodent_cfg):
    from stac_mjx_amd import io

    rng = np.random.default_rng(15)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    n = 6
    d = io.StacData(qpos=f(n, 5), xpos=f(n, 2, 3), xquat=f(n, 2, 4), marker_sites=f(n, 3, 3), offsets=f(3, 3), kp_data=f(n, 9),
                    names_qpos=["a", "b"], names_xpos=["w", "v"], kp_names=["k0", "k1", "k2"])
    assert d.kp_swapped.size == 0 and "kp_swapped" not in d.as_dict()
    assert list(io.StacData.__dataclass_fields__)[-1] == "kp_rejected"  # (the trailing field stays the trailing field)
    cfg = hs.stage_cfg(rodent_cfg)
    suffixes = [".npz"] + ([".h5"] if io.h5py is not None else [])
    for suffix in suffixes:
        plain = io.save_data_to_h5(config=cfg, file_path=tmp_path / f"plain{suffix}", **d.as_dict())
        assert io.load_stac_data(plain)[1].kp_swapped.size == 0  # a file without the dataset, as every file so far
        with_swaps = io.StacData(**{**d.__dict__})
        with_swaps.kp_swapped = (rng.random((n, 3)) < 0.4).astype(np.uint8)
        assert "kp_swapped" in with_swaps.as_dict() and "kp_rejected" not in with_swaps.as_dict()
        path = io.save_data_to_h5(config=cfg, file_path=tmp_path / f"swaps{suffix}", **with_swaps.as_dict())
        back = io.load_stac_data(path)[1]
        assert back.kp_swapped.dtype == np.uint8 and back.kp_rejected.size == 0 and back.kp_rejected_pairwise.size == 0
        np.testing.assert_array_equal(back.kp_swapped, with_swaps.kp_swapped)
