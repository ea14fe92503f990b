"""reject_pairwise, the parts that need no GPU: the rule of csrc/stac_pairwise.hpp as a stand-alone CPU program against the numpy
reference of tests/pairwise_cases.py, what the reference finds in the golden recording with 40-frame left / right swaps (and what the
Hampel identifier finds there), the config keys, the argument checks of
``stac_prep_pairwise`` (they happen before the device is touched) and ``kp_rejected_pairwise`` through the result files."""

import ctypes as C
import subprocess

import numpy as np
import pytest

import outlier_cases as oc
import pairwise_cases as pc
import host_scaffold as hs
from conftest import ROOT
from host_scaffold import STAC_ERR_INVALID, STAC_ERR_CAPACITY


# ---- the rule on the CPU, from the kernels' header ---------------------------------------------------------------------------------
_PROGRAM = r"""
// The rule of csrc/stac_pairwise.hpp run serially, by the passes of the kernels: the keys of every pair, the two middle order
// statistics by the three histogram passes of stac_report.hpp, the same again over the keys of the deviations, the bad pairs of a
// frame as K words of 64 bits, pairwise_blame.
// usage: prog IN OUT.  IN: int64 n, then per case int64 T, K, votes, double thr, min_dev and T * 3K floats.
// OUT: per case T * 3K floats, T * K bytes, P int64, P doubles, P doubles.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "stac_pairwise.hpp"
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

static void run(const float *kp, int64_t T, int64_t K, double thr, double min_dev, int32_t votes, float *out, uint8_t *flag, int64_t *pair_n,
                double *pair_med, double *pair_mad) {
    const PairwiseLayout L = pairwise_layout(T, K);
    if (L.bytes < 0 || L.pairs != pairwise_pairs(K)) exit(7);
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
    std::vector<uint64_t> m(K);
    for (int64_t t = 0; t < T; ++t) {
        for (int64_t k = 0; k < K; ++k) m[k] = 0;
        for (int64_t a = 0; a + 1 < K; ++a)
            for (int64_t b = a + 1; b < K; ++b) {
                const int64_t p = pairwise_index(a, b, K);
                const uint32_t key = keys[p][t];
                if (pair_n[p] < 3 || key == kReportNoKey) continue;
                const double bound = thr * pair_mad[p];
                if (pairwise_bad(pairwise_dev(report_float(key), pair_med[p]), bound, min_dev)) {
                    m[a] |= 1ull << b;
                    m[b] |= 1ull << a;
                }
            }
        const uint64_t rejected = pairwise_blame(m.data(), 1, (int32_t)K, votes);
        for (int64_t k = 0; k < K; ++k) {
            const bool r = (rejected >> k) & 1;
            for (int c = 0; c < 3; ++c) out[t * K3 + 3 * k + c] = r ? report_float(kPairwiseNanBits) : kp[t * K3 + 3 * k + c];
            flag[t * K + k] = r ? 1 : 0;
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
        int64_t hd[3];
        double par[2];
        if (fread(hd, 8, 3, in) != 3 || fread(par, 8, 2, in) != 2) return 5;
        const int64_t T = hd[0], K = hd[1], P = K * (K - 1) / 2;
        std::vector<float> kp(T * 3 * K), out(T * 3 * K, -12345.0f);
        std::vector<uint8_t> flag(T * K, 0xEE);
        std::vector<int64_t> pn(P, -7);
        std::vector<double> med(P, -7.0), mad(P, -7.0);
        if ((int64_t)fread(kp.data(), 4, kp.size(), in) != (int64_t)kp.size()) return 6;
        run(kp.data(), T, K, par[0], par[1], (int32_t)hd[2], out.data(), flag.data(), pn.data(), med.data(), mad.data());
        fwrite(out.data(), 4, out.size(), outf);
        fwrite(flag.data(), 1, flag.size(), outf);
        if (P > 0) {  // (K = 1: no pairs, and an empty vector has no data)
            fwrite(pn.data(), 8, pn.size(), outf);
            fwrite(med.data(), 8, med.size(), outf);
            fwrite(mad.data(), 8, mad.size(), outf);
        }
    }
    fclose(outf);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return hs.build_cpu_program(tmp_path_factory, "pairwise", _PROGRAM, "-O2")


@pytest.mark.parametrize("K", pc.KS)
def test_rule_on_the_cpu_equals_the_reference(program, tmp_path, K):
    """Every case of the GPU test with this many keypoints, one run of the program."""
    cases = pc.cases(ks=(K,))
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.int64(len(cases)).tobytes())
        for name, T, K_ in cases:
            kp, thr, min_dev, votes, _ = pc.reference(name, T, K_)
            fh.write(np.array([T, K_, votes], np.int64).tobytes())
            fh.write(np.array([thr, min_dev], np.float64).tobytes())
            fh.write(kp.tobytes())
    res = subprocess.run([str(program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    raw = (tmp_path / "out.bin").read_bytes()
    pos, P = 0, K * (K - 1) // 2
    for name, T, K_ in cases:
        kp, _, _, _, want = pc.reference(name, T, K_)
        got = []
        for dt, shape in ((np.float32, (T, 3 * K)), (np.uint8, (T, K)), (np.int64, (P,)), (np.float64, (P,)), (np.float64, (P,))):
            count = int(np.prod(shape))
            got.append(np.frombuffer(raw, dt, count, pos).reshape(shape))
            pos += count * np.dtype(dt).itemsize
        pc.check(got, kp, want, label=f"{name} T={T} K={K}")
    assert pos == len(raw)


@pytest.mark.parametrize("K", pc.KS)
def test_the_reference_the_tests_share_is_the_plain_loop_reference(K):
    """``pairwise_cases.reference`` computes all pairs at once; the loop per pair of ``reference_pairwise`` gives the same bits on
    every case."""
    for name, T, _ in pc.cases(ks=(K,)):
        kp, thr, min_dev, votes, want = pc.reference(name, T, K)
        pc.check(pc.reference_pairwise(kp, thr, min_dev, votes), kp, want, label=f"{name} T={T} K={K}")


def test_the_cases_hold_what_they_are_meant_to():
    assert set(pc.TS) == {1, 2, 3, 63, 64, 65, 129, 1000} and set(pc.KS) == {1, 2, 3, 23, 64}
    cases = pc.cases()
    assert {(T, K) for _, T, K in cases} == {(T, K) for T in pc.TS for K in pc.KS}  # every shape of the grid
    for name, (_, t_min, k_min) in pc.PATTERNS.items():  # every pattern at every shape it fits, and at more than one K and T
        assert {(T, K) for n, T, K in cases if n == name} == {(T, K) for T in pc.TS for K in pc.KS if T >= t_min and K >= k_min}, name
        assert t_min <= 5 and k_min <= 4
    assert {pc.reference(n, 129, 23)[3] for n in pc.PATTERNS} == {1, 2, 22}  # votes of 1, 2 and K - 1
    T = 129
    for K in (2, 3, 23, 64):
        ref = lambda name: pc.reference(name, T, K)  # noqa: E731
        kp, _, _, _, (out, flag, n, med, mad) = ref("no_defect")
        assert flag.sum() == 0 and (n == T).all() and np.isfinite(med).all() and (mad > 0).all()
        np.testing.assert_array_equal(out.view(np.uint32), kp.view(np.uint32))
        kp = ref("missing")[0]
        assert (~np.isfinite(kp.reshape(T, K, 3)).all(axis=2)).any(axis=0).all()  # every keypoint, in some frames
        assert np.isnan(kp).any() and np.isposinf(kp).any() and np.isneginf(kp).any()
        # a tie of c_k between two wrong keypoints: the lowest index goes, and with votes = K - 1 the other one stays
        a, b = pc._tie_kps(K)
        _, _, _, votes, (_, flag, _, _, _) = ref("tie")
        assert votes == K - 1 and a < b and flag[T // 2, a] == 1 and flag[T // 2, b] == 0 and flag[T // 2].sum() == 1
        # mad = 0 everywhere: min_dev alone decides: 0.5 mm stays, 50 cm goes
        _, _, min_dev, _, (_, flag, _, _, mad) = ref("identical")
        assert (mad == 0).all() and min_dev > 0.0005 and flag.sum() == 1 and flag[T // 2].sum() == 0 and flag[T // 3].sum() == 1
        # 1e20: the keypoints are present, their pairs are not valid in those frames
        kp, _, _, _, (out, flag, n, _, _) = ref("huge")
        frames = np.flatnonzero(np.arange(T) % 7 == 3)
        assert np.isfinite(kp).all() and n[pc.pair_index(0, K - 1, K)] == T - frames.size and not flag[frames][:, [0, K - 1]].any()
        # -0.0 and denormals: not rejected, so they pass bit for bit
        kp, _, _, _, (out, flag, _, _, _) = ref("zeros_and_denormals")
        x = kp.reshape(T, K, 3)
        assert flag[:, 0].sum() == 0 and np.signbit(x[1::2, 0, 0]).all() and (x[1::2, 0, 0] == 0).all()
        assert (np.abs(x[:, 0, 1:]) < 1.2e-38).all() and (x[1:50, 0, 1] > 0).all()
        np.testing.assert_array_equal(out.reshape(T, K, 3)[:, 0].view(np.uint32), x[:, 0].view(np.uint32))
        # the selection passes: the keys of d of the pair (0, 1) differ in the middle 11 bits alone / in the last 10 alone
        for name, same, differ in (("second_pass_only", 0xFFE003FF, 0x001FFC00), ("third_pass_only", 0xFFFFFC00, 0x000003FF)):
            x = ref(name)[0].reshape(T, K, 3)
            keys = x[:, 1, 0].view(np.uint32)
            assert len(np.unique(keys & np.uint32(same))) == 1 and len(np.unique(keys & np.uint32(differ))) > 20, name
            med = ref(name)[4][3][0]
            assert med == np.float64(np.sort(x[:, 1, 0])[(T - 1) // 2])  # (T is odd)
        # the rank (n - 1) / 2 at the first, a middle and the last element of a run of equal values
        for where in ("first", "middle", "last"):
            d = np.sort(ref(f"tie_rank_{where}")[0].reshape(T, K, 3)[:, 1, 0])
            r = (T - 1) // 2
            lo, hi = np.searchsorted(d, d[r], "left"), np.searchsorted(d, d[r], "right") - 1
            assert d[r] == 2.0 and hi - lo >= 2 and {"first": r == lo, "middle": lo < r < hi, "last": r == hi}[where], (where, lo, r, hi)
        if K >= 3:
            n = ref("pair_counts")[4][2]
            assert [n[pc.pair_index(a, b, K)] for a, b in ((0, 1), (0, 2), (1, 2))] == [0, 2, 3]
            med = ref("pair_counts")[4][3]
            assert (med[:2].view(np.uint64) == pc.QNAN64).all() and np.isfinite(med[pc.pair_index(1, 2, K)])
        if K >= 4:
            # two wrong keypoints: some innocent third keypoint has two bad pairs in that frame, and only the two are rejected
            a, b = pc._two_wrong_kps(K)
            flag = ref("two_wrong")[4][1]
            assert flag[T // 2, a] == 1 and flag[T // 2, b] == 1 and flag[T // 2].sum() == 2
        if K >= 23:  # (with two keypoints no keypoint ever has two bad pairs)
            assert ref("noise_votes_2")[4][1].sum() > 0 and ref("noise_votes_1")[4][1].sum() > ref("noise_votes_2")[4][1].sum()
            assert ref("noise_votes_K_minus_1")[4][1].sum() > 0
    # K = 1 has no pairs and passes everything through; T < 3 decides nothing
    for name, T, K in cases:
        if K == 1 or T < 3:
            kp, _, _, _, (out, flag, n, _, _) = pc.reference(name, T, K)
            assert flag.sum() == 0 and n.shape == (K * (K - 1) // 2,)
            np.testing.assert_array_equal(out.view(np.uint32), kp.view(np.uint32))


def test_motivating_swaps_of_40_frames_in_the_golden_recording(rodent_mocap, rodent_cfg):
    """Each of the 9 left / right keypoint pairs of the rodent swapped for 40 consecutive frames (the first run starts at frame 50,
    each later one 60 frames after the one before): 720 wrong keypoints.  The reference with the default parameters, measured:
    650 of the 720 = 90.3 % found, 2.34 % of the untouched recording rejected; the Hampel reference at its defaults finds 1 of the
    720 (0.14 %): by its known limit it keeps all but the ends of every run."""
    from stac_mjx_amd.config import OUTLIER_DEFAULTS, PAIRWISE_DEFAULTS

    names = list(rodent_cfg["KEYPOINT_MODEL_PAIRS"].keys())
    swaps = pc.swap_pairs(names)
    assert len(names) == 23 and len(swaps) == 9 and [names[l] for l, _ in swaps][:2] == ["AnkleL", "EarL"]
    kp, wrong = pc.swapped_recording(rodent_mocap, names)
    assert wrong.sum() == 720 and wrong[50:90, list(swaps[0])].all() and wrong[110:150, list(swaps[1])].all() and not wrong[:50].any()
    par = (PAIRWISE_DEFAULTS["pairwise_nsigma"] * pc.MAD_TO_SIGMA, PAIRWISE_DEFAULTS["pairwise_min_dev"], PAIRWISE_DEFAULTS["pairwise_votes"])
    assert par == (pc.THR, pc.MIN_DEV, 2)
    flag = pc.reference_pairwise(kp, *par)[1]
    clean = pc.reference_pairwise(np.asarray(rodent_mocap, np.float32), *par)[1]
    hampel = oc.reference_reject(kp, OUTLIER_DEFAULTS["outlier_window"], OUTLIER_DEFAULTS["outlier_nsigma"] * 1.4826,
                                 OUTLIER_DEFAULTS["outlier_min_dev"])[1]
    found, false, found_hampel = flag[wrong].mean(), clean.mean(), hampel[wrong].mean()
    print(f"swapped keypoints found: {found:.4f} ({int(flag[wrong].sum())} of 720); rejected in the untouched recording: {false:.4f}; "
          f"found by hampel: {found_hampel:.4f} ({int(hampel[wrong].sum())} of 720)")
    assert found >= 0.80
    assert false <= 0.03
    assert hampel[wrong].sum() < flag[wrong].sum()


# ---- config -----------------------------------------------------------------------------------------------------------------------
def test_config_reject_pairwise_keys(rodent_cfg):
    from stac_mjx_amd import prep
    from stac_mjx_amd.config import PAIRWISE_NEEDS_FILL, pairwise_options
    from stac_mjx_amd.main import _reject_outliers_mode, _reject_pairwise_mode

    plain = hs.stage_cfg(rodent_cfg)
    assert _reject_pairwise_mode(plain)[0] == "off" and "pairwise" not in plain.to_yaml()  # absent stays absent
    assert pairwise_options(plain.stac) == ("off", 6.0, 0.002, 2)
    assert _reject_pairwise_mode(hs.stage_cfg(rodent_cfg, reject_pairwise="off"))[0] == "off"
    off = hs.stage_cfg(rodent_cfg, reject_pairwise=False)  # what YAML 1.1 makes of a bare `off`
    assert _reject_pairwise_mode(off)[0] == "off" and off.stac.reject_pairwise == "off"
    mode, args = _reject_pairwise_mode(hs.stage_cfg(rodent_cfg, reject_pairwise="mad", fill_missing="linear"))
    assert mode == "mad" and args == {"n_sigma": 6.0, "min_dev": 0.002, "votes": 2}  # the defaults
    mode, args = _reject_pairwise_mode(hs.stage_cfg(rodent_cfg, reject_pairwise="mad", fill_missing="hold", pairwise_nsigma=8, pairwise_min_dev=0,
                                            pairwise_votes=3))
    assert mode == "mad" and args == {"n_sigma": 8.0, "min_dev": 0.0, "votes": 3}
    # the sibling is untouched: same return value with and without the new keys
    assert _reject_outliers_mode(hs.stage_cfg(rodent_cfg, reject_pairwise="mad", fill_missing="linear")) == _reject_outliers_mode(plain)
    header = (ROOT / "stac_mjx_amd" / "csrc" / "stac_pairwise.hpp").read_text()
    assert f"kPairwiseMaxKp = {prep.PAIRWISE_MAX_KP};" in header and prep.PAIRWISE_MAX_KP == 64
    bad = [dict(reject_pairwise="on"), dict(reject_pairwise="MAD"), dict(reject_pairwise=True), dict(reject_pairwise=1),
           dict(reject_pairwise="hampel"), dict(pairwise_nsigma=-1.0), dict(pairwise_nsigma=float("nan")), dict(pairwise_nsigma=float("inf")),
           dict(pairwise_nsigma="6"), dict(pairwise_nsigma=True), dict(pairwise_min_dev=-0.001), dict(pairwise_min_dev=float("inf")),
           dict(pairwise_min_dev=None), dict(pairwise_votes=0), dict(pairwise_votes=-2), dict(pairwise_votes=2.0), dict(pairwise_votes="2"),
           dict(pairwise_votes=True), dict(pairwise_votes=None), dict(pairwise_votes=2**31)]
    for over in bad:
        with pytest.raises(ValueError):
            _reject_pairwise_mode(hs.stage_cfg(rodent_cfg, fill_missing="linear", **over))
        cfg = hs.stage_cfg(rodent_cfg, fill_missing="linear")  # also when the key is set after validation: the run reads the caller's config
        cfg.stac.update(over)
        with pytest.raises(ValueError):
            _reject_pairwise_mode(cfg)
    with pytest.raises(ValueError):
        hs.stage_cfg(rodent_cfg, pairwise_nsigm=5)  # an unknown key stays an error
    for fill in ({}, dict(fill_missing="off")):  # the solver cannot take the NaNs: one text
        with pytest.raises(ValueError) as err:
            _reject_pairwise_mode(hs.stage_cfg(rodent_cfg, reject_pairwise="mad", **fill))
        assert str(err.value) == PAIRWISE_NEEDS_FILL and "fill_missing" in PAIRWISE_NEEDS_FILL


def test_run_stac_refuses_pairwise_without_filling_before_any_work(tmp_path, rodent_cfg):
    from stac_mjx_amd.config import PAIRWISE_NEEDS_FILL
    from stac_mjx_amd.main import run_stac

    cfg = hs.stage_cfg(rodent_cfg, reject_pairwise="mad")
    with pytest.raises(ValueError) as err:  # before the model is even looked for: the path does not exist
        run_stac(cfg, np.zeros((4, 6), np.float32), ["a", "b"], base_path=tmp_path / "nowhere")
    assert str(err.value) == PAIRWISE_NEEDS_FILL
    assert not list(tmp_path.iterdir())


# ---- C ABI and wrapper ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return hs.loaded_library()


def test_workspace_arithmetic(lib):
    ws = lib.stac_prep_pairwise_workspace
    for T, K in ((1, 1), (1, 2), (64, 2), (65, 3), (1000, 23), (10**6, 23), (129, 64)):
        P, stride = K * (K - 1) // 2, (T + 63) // 64 * 64
        assert ws(T, K) == max(P * (4 * stride + 8 * (1024 + 2 * 2048 + 2 * 1024) + 32), 8), (T, K)
    assert ws(10**6, 23) < 1.1 * 2**30  # the recording of the issue: about 1 GiB
    for T, K in ((0, 3), (-1, 3), (5, 0), (5, -2), (2**45, 2)):
        assert ws(T, K) == STAC_ERR_INVALID and lib.stac_last_error_code() == STAC_ERR_INVALID and "stac_prep_pairwise_workspace" in lib.stac_last_error().decode()
    assert ws(5, 65) == STAC_ERR_CAPACITY and lib.stac_last_error_code() == STAC_ERR_CAPACITY and "65" in lib.stac_last_error().decode()


def test_pairwise_argument_errors_need_no_device(lib):
    """Every pointer below is a fake non-NULL address: a call that got past its checks would fault, not return."""
    T, K = 100, 23
    P = K * (K - 1) // 2
    need = lib.stac_prep_pairwise_workspace(T, K)
    good = dict(kp=0x100000, T=T, K=K, thr=pc.THR, min_dev=0.002, votes=2, out=0x200000, flag=0x300000, pair_n=0x400000, pair_med=0x500000,
                pair_mad=0x600000, work=0x10000000, nbytes=need)
    p = lambda a: C.c_void_p(a) if a else None  # noqa: E731

    def call(code=STAC_ERR_INVALID, **over):
        a = {**good, **over}
        rc = lib.stac_prep_pairwise(p(a["kp"]), a["T"], a["K"], a["thr"], a["min_dev"], a["votes"], p(a["out"]), p(a["flag"]), p(a["pair_n"]),
                                    p(a["pair_med"]), p(a["pair_mad"]), p(a["work"]), a["nbytes"], None)
        msg = lib.stac_last_error().decode()
        assert rc == code and lib.stac_last_error_code() == code and "stac_prep_pairwise" in msg, (over, rc, msg)
        return msg

    for null in ("kp", "out", "flag", "pair_n", "pair_med", "pair_mad", "work"):
        assert "null" in call(**{null: 0})
    for bad in (dict(T=0), dict(T=-3), dict(K=0), dict(K=-1)):
        call(**bad)
    for K_ in (65, 70, 1000):
        assert str(K_) in call(code=STAC_ERR_CAPACITY, K=K_)
    for v in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        call(thr=v)
        call(min_dev=v)
    for v in (0, -1, -2**31):
        assert "votes" in call(votes=v)
    assert str(need) in call(nbytes=need - 1)
    call(nbytes=0)
    call(nbytes=-5)
    for name, align in (("kp", 4), ("out", 4), ("pair_n", 8), ("pair_med", 8), ("pair_mad", 8), ("work", 8)):
        assert "aligned" in call(**{name: good[name] + align // 2})
    assert "aligned" in call(pair_n=good["pair_n"] + 4)
    kp_bytes = T * K * 12
    assert "overlap" in call(out=good["kp"])  # in place
    call(out=good["kp"] + kp_bytes - 4)
    call(kp=good["out"] + kp_bytes - 4)
    call(flag=good["kp"])
    call(flag=good["out"] + kp_bytes - 1)
    call(pair_med=good["pair_n"] + 8 * P - 8)
    call(pair_mad=good["pair_med"])
    call(work=good["out"] + 8)
    call(out=good["work"] + need - 4)
    call(pair_n=good["work"] + 64)


def test_python_wrapper_refuses_what_it_cannot_run():
    import torch

    from stac_mjx_amd import prep

    with pytest.raises(ValueError):
        prep.reject_pairwise(torch.zeros(4, 6))  # a host tensor
    good = dict(n_sigma=6.0, min_dev=0.002, votes=2)
    for bad in (dict(n_sigma=-1), dict(n_sigma=float("nan")), dict(n_sigma="6"), dict(min_dev=-1e-9), dict(min_dev=float("inf")),
                dict(n_sigma=1.5e308), dict(votes=0), dict(votes=1.0), dict(votes=True), dict(votes=2**31)):
        with pytest.raises(ValueError):
            prep.pairwise_params(**{**good, **bad})
    assert prep.pairwise_params(**good) == (pc.THR, 0.002, 2) and pc.THR == 6.0 * 1.4826


# ---- kp_rejected_pairwise through the result files ---------------------------------------------------------------------------------
def test_kp_rejected_pairwise_round_trip_and_old_files(tmp_path, rodent_cfg):
    from stac_mjx_amd import io

    rng = np.random.default_rng(5)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    n = 6
    d = io.StacData(qpos=f(n, 5), xpos=f(n, 2, 3), xquat=f(n, 2, 4), marker_sites=f(n, 3, 3), offsets=f(3, 3), kp_data=f(n, 9),
                    names_qpos=["a", "b"], names_xpos=["w", "v"], kp_names=["k0", "k1", "k2"])
    assert "kp_rejected_pairwise" not in d.as_dict()
    assert list(io.StacData.__dataclass_fields__)[-1] == "kp_rejected"  # (the trailing field stays the trailing field)
    cfg = hs.stage_cfg(rodent_cfg)
    suffixes = [".npz"] + ([".h5"] if io.h5py is not None else [])
    for suffix in suffixes:
        plain = io.save_data_to_h5(config=cfg, file_path=tmp_path / f"plain{suffix}", **d.as_dict())
        assert io.load_stac_data(plain)[1].kp_rejected_pairwise.size == 0  # a file without the dataset, as every file so far
        both = io.StacData(**{**d.__dict__})
        both.kp_rejected_pairwise = (rng.random((n, 3)) < 0.3).astype(np.uint8)
        both.kp_rejected = both.kp_rejected_pairwise | (rng.random((n, 3)) < 0.2).astype(np.uint8)
        both.kp_gap = both.kp_rejected.astype(np.int32)
        path = io.save_data_to_h5(config=cfg, file_path=tmp_path / f"both{suffix}", **both.as_dict())
        back = io.load_stac_data(path)[1]
        assert back.kp_rejected_pairwise.dtype == np.uint8
        np.testing.assert_array_equal(back.kp_rejected_pairwise, both.kp_rejected_pairwise)
        np.testing.assert_array_equal(back.kp_rejected, both.kp_rejected)
