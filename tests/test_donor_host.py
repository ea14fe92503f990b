"""fill_donors, the parts that need no GPU: the rule of csrc/stac_donor.hpp as a stand-alone CPU program (under the address and
undefined-behaviour sanitizers where the host compiler has them) that runs the staged scan serially with small tiles, against the
numpy reference of tests/donor_cases.py; the config keys and the pre-flight refusal;
the argument checks of the entry points (they happen before the device is touched); ``prep.donor_table`` on hand-made
statistics; ``kp_gap`` through ``_prepare_series`` and the result files; and what the rule is worth, on the reference alone."""

import ctypes as C
import subprocess

import numpy as np
import pytest

import donor_cases as dc
import pairwise_cases as pw
import prep_cases as pc
import host_scaffold as hs
from host_scaffold import STAC_ERR_INVALID, STAC_ERR_CAPACITY


@pytest.fixture(scope="module")
def lib():
    return hs.loaded_library()


# ---- the rule on the CPU, from the kernel's header, with any tile size -------------------------------------------------------------
_PROGRAM = r"""
// The three stages of csrc/stac_donor.hip, run serially with a tile of any size, on the functions of stac_prep.hpp and stac_donor.hpp.
// usage: prog TILE IN OUT.  IN: int64 n, then per case int64 T, K, D, T * 3K floats and K * D * 3 int32.
// OUT: per case T * 3K floats, T * K int32, T * K bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "stac_donor.hpp"
using namespace stac;

static void fill(const float *kp, int64_t T, int32_t K, const int32_t *don, int32_t D, int64_t tile, float *out, int32_t *gap, uint8_t *src) {
    const int64_t tiles = prep_tiles(T, tile), K3 = 3 * (int64_t)K;
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
    for (int64_t i = 0; i < tiles; ++i)  // 3: the donor fill
        for (int64_t t = i * tile; t < (i + 1) * tile && t < T; ++t)
            for (int32_t k = 0; k < K; ++k) {
                const float *s = kp + t * K3 + 3 * k;
                float *o = out + t * K3 + 3 * k;
                int32_t g = 0, from = kDonorObserved;
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
                    from = kDonorLeft;
                    if (p >= 0 || n >= 0)
                        for (int32_t d = 0; d < D; ++d) {
                            const int32_t *row = don + ((int64_t)k * D + d) * 3;
                            if (!donor_row(k, K, row[0], row[1], row[2])) break;
                            float r[3];
                            if (!missing(t, row[0]) && !missing(t, row[1]) && !missing(t, row[2]) &&
                                donor_try(kp, K3, t, p, n, k, row[0], row[1], row[2], r)) {
                                o[0] = r[0], o[1] = r[1], o[2] = r[2];
                                from = d + 1;
                                break;
                            }
                        }
                }
                gap[t * K + k] = g;
                src[t * K + k] = (uint8_t)from;
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
        const int64_t T = h[0], K = h[1], D = h[2];
        std::vector<float> kp(T * 3 * K), out(T * 3 * K, -12345.0f);
        std::vector<int32_t> don(K * D * 3), gap(T * K, -7);
        std::vector<uint8_t> src(T * K, 77);
        if ((int64_t)fread(kp.data(), 4, kp.size(), in) != (int64_t)kp.size()) return 6;
        if ((int64_t)fread(don.data(), 4, don.size(), in) != (int64_t)don.size()) return 7;
        fill(kp.data(), T, (int32_t)K, don.data(), (int32_t)D, tile, out.data(), gap.data(), src.data());
        fwrite(out.data(), 4, out.size(), outf);
        fwrite(gap.data(), 4, gap.size(), outf);
        fwrite(src.data(), 1, src.size(), outf);
    }
    fclose(outf);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return hs.build_cpu_program(tmp_path_factory, "donor", _PROGRAM, "-O1")


@pytest.mark.parametrize("tile", [1, 2, 4, 7])
def test_rule_on_the_cpu_equals_the_reference(program, tmp_path, tile):
    """Every case of the GPU test, the staged scan with this tile size, one run of the program, tolerance 0."""
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.int64(len(dc.CASES)).tobytes())
        for case in dc.CASES:
            kp, don = dc.reference(*case)[:2]
            fh.write(np.array([kp.shape[0], don.shape[0], don.shape[1]], np.int64).tobytes())
            fh.write(kp.tobytes())
            fh.write(don.astype(np.int32).tobytes())
    res = subprocess.run([str(program), str(tile), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    raw = (tmp_path / "out.bin").read_bytes()
    pos = 0
    for case in dc.CASES:
        kp, don, want_out, want_gap, want_src = dc.reference(*case)
        T, K = want_gap.shape
        out = np.frombuffer(raw, np.float32, T * 3 * K, pos).reshape(T, 3 * K)
        pos += 4 * T * 3 * K
        gap = np.frombuffer(raw, np.int32, T * K, pos).reshape(T, K)
        pos += 4 * T * K
        src = np.frombuffer(raw, np.uint8, T * K, pos).reshape(T, K)
        pos += T * K
        dc.check(out, gap, src, kp, want_out, want_gap, want_src, label=f"tile={tile} {case}")
    assert pos == len(raw)


def test_the_cases_hold_what_they_are_meant_to():
    case = lambda name, T=200, K=23, D=4: dc.reference(name, T, K, D)  # noqa: E731
    assert {c[1] for c in dc.CASES} == set(dc.TS) and {c[2] for c in dc.CASES} == set(dc.KS) and {c[3] for c in dc.CASES} == set(dc.DS)
    for name in dc.PATTERNS:  # every pattern meets every T, every K and every D
        mine = [c for c in dc.CASES if c[0] == name]
        assert {c[1] for c in mine} == set(dc.TS) and {c[2] for c in mine} >= set(dc.KS) and {c[3] for c in mine} == set(dc.DS), name
    kp, don, out, gap, src = case("none")
    assert not src.any() and not gap.any() and np.array_equal(out.view(np.uint32), kp.view(np.uint32))
    assert (kp.view(np.uint32) == 0x80000000).any() and ((kp != 0) & (np.abs(kp) < 1e-38)).any()  # -0.0 and denormals pass through
    kp, don, out, gap, src = case("tile_borders")
    assert (gap[60:71, 0] == 11).all() and (np.delete(src[60:71, 0], 4) == 1).all()  # crosses the border of the first tile
    assert src[64, 0] == 3                                                     # (keypoint 2, in its rows 0 and 1, is missing in frame 64)
    assert (gap[10:151, 22] == 141).all() and (src[10:151, 22] >= 1).all() and (src[10:151, 22] < 255).all()  # longer than two tiles
    assert gap[127, 1] == 8 and gap[128, 1] == 0 and gap[64, 2] == 1
    kp, don, out, gap, src = case("leading_trailing")
    assert (gap[:6, 0] == 6).all() and (src[:6, 0] == 1).all() and (gap[196:, 1] == 4).all() and (src[196:, 1] == 1).all()
    assert 1 <= src[0, 22] < 255 and 1 <= src[199, 22] < 255 and gap[0, 22] == 1 and gap[199, 22] == 1  # both on one track
    kp, don, out, gap, src = case("empty_track")
    assert (gap[:, 2] == 200).all() and (src[:, 2] == 255).all() and np.isnan(out.reshape(200, 23, 3)[:, 2]).all()
    assert (src[3:7, 0] == 3).all()  # rows 0 and 1 of keypoint 0 name the empty track: row 2 fills
    kp, don, out, gap, src = case("donor_missing")
    assert src[5:10, 0].tolist() == [1, 1, 2, 1, 1]                            # the donor is missing at t only
    assert (src[20:25, 0] == 2).all() and (src[40:45, 0] == 2).all()           # at p only, at n only
    kp, don, out, gap, src = case("all_unusable")
    assert (src[3] == 255).all() and (src[10:13, 0] == 255).all() and np.isnan(out[3]).all()
    kp, don, out, gap, src = case("degenerate")
    assert (src[2:5, 0] == 3).all() and (src[62:67, 0] == 3).all()             # coincident, collinear, then a good row
    assert (case("degenerate", K=5)[4][2:5, 0] == 255).all() and (case("degenerate", K=4)[4][2:5, 0] == 255).all()
    kp, don, out, gap, src = case("mutual")
    assert (src[4:9, :2] == 2).all() and (src[61:68, :2] == 2).all()
    kp, don, out, gap, src = case("infinities")
    assert np.isposinf(kp).any() and np.isneginf(kp).any() and not np.isnan(kp).any() and np.isfinite(out).all()
    assert src[200 // 3, 0] == 3  # keypoint 2, a donor of the rows 0 and 1, is -inf in that frame
    kp, don, out, gap, src = case("table_ends")
    for k in (0, 1, 2, 4, 5):
        assert (src[5 + 8 * k:10 + 8 * k, k] == 255).all(), k
    assert (src[29:34, 3] == 1).all() and (src[60:62, 3] == 255).all() and dc.is_triple(3, 23, don[3, 2])
    kp, don, out, gap, src = case("random_holes")
    assert 0.1 < np.count_nonzero(gap) / gap.size < 0.4 and len(np.unique(src)) >= 3


# ---- config and pre-flight ---------------------------------------------------------------------------------------------------------
def test_config_fill_donors_keys(rodent_cfg):
    from stac_mjx_amd.config import DONOR_DEFAULTS, DONORS_NEED_FILL, donor_options
    from stac_mjx_amd.main import _fill_donors_mode, _reject_pairwise_mode, _repair_swaps_mode

    plain = hs.stage_cfg(rodent_cfg)
    assert DONOR_DEFAULTS == {"fill_donors_triples": 4}
    assert donor_options(plain.stac) == ("off", 4) and _fill_donors_mode(plain) == ("off", 4) and "donors" not in plain.to_yaml()
    off = hs.stage_cfg(rodent_cfg, fill_donors=False)  # what YAML 1.1 makes of a bare `off`
    assert off.stac.fill_donors == "off" and _fill_donors_mode(off) == ("off", 4)
    assert _fill_donors_mode(hs.stage_cfg(rodent_cfg, fill_donors="off", fill_donors_triples=8)) == ("off", 8)
    for fill in ("linear", "hold"):
        on = hs.stage_cfg(rodent_cfg, fill_donors="auto", fill_missing=fill, fill_donors_triples=1)
        assert _fill_donors_mode(on) == ("auto", 1)
        assert _reject_pairwise_mode(on) == _reject_pairwise_mode(plain) and _repair_swaps_mode(on) == _repair_swaps_mode(plain)
    # auto without the fill: what no triple can fill would reach the solver as NaN
    for over in (dict(fill_donors="auto"), dict(fill_donors="auto", fill_missing="off")):
        cfg = hs.stage_cfg(rodent_cfg, **over)  # (the values are fine: the refusal is the pre-flight's)
        with pytest.raises(ValueError) as e:
            _fill_donors_mode(cfg)
        assert str(e.value) == DONORS_NEED_FILL
    bad = [dict(fill_donors="on"), dict(fill_donors="Auto"), dict(fill_donors=True), dict(fill_donors=1), dict(fill_donors="linear"),
           dict(fill_donors=["auto"]), dict(fill_donors_triples=0), dict(fill_donors_triples=9), dict(fill_donors_triples=-1),
           dict(fill_donors_triples=4.0), dict(fill_donors_triples="4"), dict(fill_donors_triples=True), dict(fill_donors_triples=None)]
    for over in bad:
        with pytest.raises(ValueError):
            hs.stage_cfg(rodent_cfg, fill_missing="linear", **over)
        cfg = hs.stage_cfg(rodent_cfg, fill_missing="linear")  # also when the key is set after validation: the run reads the caller's config
        cfg.stac.update(over)
        with pytest.raises(ValueError):
            _fill_donors_mode(cfg)
    with pytest.raises(ValueError):
        hs.stage_cfg(rodent_cfg, fill_donor="auto")  # an unknown key stays an error


def test_run_stac_refuses_donors_without_fill_before_any_work(tmp_path, rodent_cfg):
    from stac_mjx_amd.config import DONORS_NEED_FILL
    from stac_mjx_amd.main import run_stac

    names = list(rodent_cfg["KEYPOINT_MODEL_PAIRS"].keys())
    kp = np.zeros((4, 69), np.float32)
    with pytest.raises(ValueError) as e:  # before the model is even looked for: the path does not exist
        run_stac(hs.stage_cfg(rodent_cfg, fill_donors="auto"), kp, names, base_path=tmp_path / "nowhere")
    assert str(e.value) == DONORS_NEED_FILL
    cfg = hs.stage_cfg(rodent_cfg, fill_missing="linear", fill_donors="auto")
    cfg.stac.fill_donors_triples = 9  # a bad value set after validation
    with pytest.raises(ValueError, match="fill_donors_triples"):
        run_stac(cfg, kp, names, base_path=tmp_path / "nowhere")
    assert not list(tmp_path.iterdir())


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_workspace_is_the_fill_workspace(lib):
    from stac_mjx_amd import prep

    for T, K in ((1, 1), (64, 2), (65, 3), (1000, 23), (10**6, 23), (129, 64)):
        assert lib.stac_prep_donor_workspace(T, K) == lib.stac_prep_fill_workspace(T, K) == prep.donor_workspace_bytes(T, K) >= 32, (T, K)
    for T, K in ((0, 3), (-1, 3), (5, 0), (5, -2), (2**62, 2**30)):
        assert lib.stac_prep_donor_workspace(T, K) == STAC_ERR_INVALID and lib.stac_last_error_code() == STAC_ERR_INVALID
        assert "stac_prep_donor_workspace" in lib.stac_last_error().decode()
    assert lib.stac_prep_donor_workspace(5, 65) == STAC_ERR_CAPACITY and lib.stac_last_error_code() == STAC_ERR_CAPACITY


def test_donor_argument_errors_need_no_device(lib):
    """Every device pointer below is a fake non-NULL address: a call that got past its checks would fault, not return."""
    T, K, D = 100, 23, 4
    need = lib.stac_prep_donor_workspace(T, K)
    good = dict(kp=0x100000, T=T, K=K, don=0x180000, D=D, out=0x200000, gap=0x300000, src=0x400000, work=0x10000000, nbytes=need)
    p = lambda a: C.c_void_p(a) if a else None  # noqa: E731

    def call(code=STAC_ERR_INVALID, **over):
        a = {**good, **over}
        rc = lib.stac_prep_donor(p(a["kp"]), a["T"], a["K"], p(a["don"]), a["D"], p(a["out"]), p(a["gap"]), p(a["src"]), p(a["work"]),
                                 a["nbytes"], None)
        msg = lib.stac_last_error().decode()
        assert rc == code and lib.stac_last_error_code() == code and "stac_prep_donor" in msg, (over, rc, msg)
        return msg

    for null in ("kp", "don", "out", "gap", "src", "work"):
        assert "null" in call(**{null: 0})
    for bad in (dict(T=0), dict(T=-3), dict(K=0), dict(K=-1)):
        call(**bad)
    for K_ in (65, 70, 1000):
        assert str(K_) in call(code=STAC_ERR_CAPACITY, K=K_, nbytes=2**40)
    for D_ in (0, -1, 9, 2**31 - 1, -2**31):
        assert "n_triples" in call(D=D_)
    assert str(need) in call(nbytes=need - 1)
    call(nbytes=0)
    call(nbytes=-5)
    for name, align in (("kp", 4), ("don", 4), ("out", 4), ("gap", 4), ("work", 8)):
        assert "aligned" in call(**{name: good[name] + align // 2})
    kp_bytes, gap_bytes, don_bytes = T * K * 12, T * K * 4, K * D * 12
    assert "overlap" in call(out=good["kp"])  # in place
    call(out=good["kp"] + kp_bytes - 4)
    call(kp=good["out"] + kp_bytes - 4)
    call(gap=good["kp"])
    call(gap=good["out"] + 8)
    call(src=good["gap"] + gap_bytes - 1)
    call(src=good["kp"] + 5)
    call(out=good["src"] + T * K - 1 - (good["src"] + T * K - 1) % 4)  # the last bytes of src
    call(don=good["out"] + 8)
    call(out=good["don"] + don_bytes - 4)
    call(work=good["out"] + 8)
    call(out=good["work"] + need - 4)
    call(don=good["work"] + 64)


def test_python_wrapper_refuses_what_it_cannot_run():
    import torch

    from stac_mjx_amd import prep

    with pytest.raises(ValueError):
        prep.fill_donors(torch.zeros(4, 12), dc.default_table(4, 2))  # a host tensor
    for bad in (0, 9, -1, 4.0, "4", True, None):
        with pytest.raises(ValueError, match="n_triples"):
            prep.donor_triples(bad)
        with pytest.raises(ValueError):
            prep.donor_table({"pair_n": np.zeros(6, np.int64), "pair_mad": np.zeros(6)}, 4, bad)
    with pytest.raises(ValueError):
        prep.donor_table({"pair_n": np.zeros(5, np.int64), "pair_mad": np.zeros(5)}, 4)  # not the pairs of 4 keypoints
    for K in (0, 65):
        with pytest.raises(ValueError):
            prep.donor_table({"pair_n": np.zeros(0, np.int64), "pair_mad": np.zeros(0)}, K)


# ---- the automatic table -------------------------------------------------------------------------------------------------------------
def _stats(K, mad, n=None):
    """hand-made statistics: mad[(a, b)] for a < b, every other pair 1.0; n likewise, every other pair 100"""
    pair_n, pair_mad = np.full(K * (K - 1) // 2, 100, np.int64), np.ones(K * (K - 1) // 2)
    for (a, b), v in mad.items():
        pair_mad[pw.pair_index(a, b, K)] = v
    for (a, b), v in (n or {}).items():
        pair_n[pw.pair_index(a, b, K)] = v
    return {"pair_n": pair_n, "pair_mad": pair_mad}


def test_donor_table_on_hand_made_statistics():
    from stac_mjx_amd.prep import donor_table

    K = 6
    # keypoint 0: its partners by mad are 3 (0.1), 5 (0.2), 1 (0.3), 2 (0.4), 4 (1.0)
    st = _stats(K, {(0, 3): 0.1, (0, 5): 0.2, (0, 1): 0.3, (0, 2): 0.4})
    don = donor_table(st, K, 4)
    assert don.dtype == np.int32 and don.shape == (K, 4, 3)
    assert don[0].tolist() == [[3, 5, 1], [3, 5, 2], [3, 1, 2], [5, 1, 2]]
    assert donor_table(st, K, 2)[0].tolist() == [[3, 5, 1], [3, 5, 2]] and donor_table(st, K, 1)[0].tolist() == [[3, 5, 1]]
    assert donor_table(st, K, 8)[0].tolist() == don[0].tolist() + [[-1, -1, -1]] * 4  # four candidates give four triples
    for k in range(K):
        for row in don[k]:
            assert dc.is_triple(k, K, row)
    # ties go to the lower index: all of keypoint 4's pairs are 1.0
    assert don[4].tolist() == [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]]
    # keypoint 1 sees 0 at 0.3 and the rest tied at 1.0
    assert don[1, 0].tolist() == [0, 2, 3]
    # pairs without statistics (n < 3, their mad NaN) are no candidates; a NaN alone is none either
    nan = float("nan")
    st = _stats(K, {(0, 3): nan, (0, 5): nan, (0, 1): 0.3, (0, 2): 0.4, (0, 4): 0.5}, {(0, 3): 2, (0, 5): 0})
    assert donor_table(st, K, 4)[0].tolist() == [[1, 2, 4]] + [[-1, -1, -1]] * 3  # three candidates: one triple
    st = _stats(K, {(0, 4): nan}, {(0, 3): 2, (0, 5): 0})
    assert donor_table(st, K, 4)[0].tolist() == [[-1, -1, -1]] * 4  # two candidates: none
    st["pair_n"][pw.pair_index(0, 4, K)] = 2  # (as the library writes it: NaN where n < 3)
    assert donor_table(st, K, 4)[0].tolist() == [[-1, -1, -1]] * 4
    # K < 4: nobody has three partners
    for K_ in (1, 2, 3):
        assert (donor_table(_stats(K_, {}), K_, 4) == -1).all()
    # torch tensors are taken like arrays
    import torch

    st = _stats(K, {(0, 3): 0.1, (0, 5): 0.2, (0, 1): 0.3, (0, 2): 0.4})
    assert np.array_equal(donor_table({k: torch.as_tensor(v) for k, v in st.items()}, K, 4), don)


def test_donor_table_from_the_reference_statistics_of_the_recording(rodent_mocap):
    """The table the rodent gets: every row a triple, and the rows of a keypoint are its four steadiest partners"""
    from stac_mjx_amd.prep import donor_table

    kp = np.ascontiguousarray(rodent_mocap[:300], np.float32)
    _, _, pair_n, _, pair_mad = pw.reference_pairwise(kp, pw.THR, pw.MIN_DEV, 2**31 - 1)
    don = donor_table({"pair_n": pair_n, "pair_mad": pair_mad}, 23, 4)
    for k in range(23):
        mads = sorted((pair_mad[pw.pair_index(min(j, k), max(j, k), 23)], j) for j in range(23) if j != k)
        assert set(don[k].reshape(-1)) == {j for _, j in mads[:4]} and all(dc.is_triple(k, 23, r) for r in don[k]), k


# ---- kp_gap through _prepare_series and the result files ---------------------------------------------------------------------------
class _ReferenceStac:
    """The two preparation stages of a ``Stac`` by the numpy references: what ``_prepare_series`` calls, and what it was called with"""

    def __init__(self, K):
        self.K, self.pair_stats, self.calls = K, None, []

    def fill_donors(self, kp_data, don=None, n_triples=4):
        from stac_mjx_amd.prep import donor_table

        self.calls.append(("fill_donors", don, n_triples))
        if don is None:
            _, _, pair_n, _, pair_mad = pw.reference_pairwise(kp_data, pw.THR, pw.MIN_DEV, 2**31 - 1)
            don = donor_table({"pair_n": pair_n, "pair_mad": pair_mad}, self.K, n_triples)
        return dc.reference_donor(kp_data, don)

    def fill_missing(self, kp_data, mode=None):
        self.calls.append(("fill_missing", mode))
        return pc.reference_fill(kp_data, mode)


TODAY = {"config", "kp_names", "names_qpos", "names_xpos", "kp_data", "marker_sites", "offsets", "qpos", "qvel", "xpos", "xquat"}


def test_kp_gap_of_a_run_is_the_gap_of_the_raw_series(tmp_path, rodent_cfg, rodent_mocap, capsys):
    from stac_mjx_amd import io
    from stac_mjx_amd.io import StacData
    from stac_mjx_amd.main import _Preflight, _fill_missing_mode, _prepare_series

    names = list(rodent_cfg["KEYPOINT_MODEL_PAIRS"].keys())
    K, T = len(names), 80
    raw = np.ascontiguousarray(rodent_mocap[100:100 + T], np.float32).reshape(T, K, 3).copy()
    raw[10:30, 3] = np.nan
    raw[40:45, 7] = np.nan
    raw[12, :] = np.nan            # a frame without any donor: left to fill_missing
    raw = raw.reshape(T, 3 * K)
    raw_gap = pc.reference_fill(raw, "linear")[1]

    def prepare(**over):
        cfg = hs.stage_cfg(rodent_cfg, n_fit_frames=40, n_frames_per_clip=40, **over)
        pre = _Preflight(cfg, T, tmp_path / "fit.h5", kp_names=names)
        pre.check_config()
        pre.fill_mode = _fill_missing_mode(cfg)
        stac = _ReferenceStac(K)
        return cfg, stac, _prepare_series(stac, cfg, raw.copy(), pre)

    cfg, stac, series = prepare(fill_missing="linear", fill_donors="auto", fill_donors_triples=2)
    assert [c[0] for c in stac.calls] == ["fill_donors", "fill_missing"] and stac.calls[0][1] is None and stac.calls[0][2] == 2
    log = capsys.readouterr().out
    assert "fill_donors: of the keypoints of the 40 fit frames, filled by triple 1:" in log and "triple 2:" in log and "triple 3" not in log
    assert "left to fill_missing:" in log
    assert set(series.marks) == {"kp_gap"} and series.marks["kp_gap"].dtype == np.int32
    np.testing.assert_array_equal(series.marks["kp_gap"], raw_gap)  # not the gap of what the donors left
    _, _, pair_n, _, pair_mad = pw.reference_pairwise(raw, pw.THR, pw.MIN_DEV, 2**31 - 1)
    from stac_mjx_amd.prep import donor_table

    d_out, d_gap, d_src = dc.reference_donor(raw, donor_table({"pair_n": pair_n, "pair_mad": pair_mad}, K, 2))
    assert (d_src[12] == 255).all() and (d_src[10:12, 3] > 0).all() and (d_src[10:12, 3] < 255).all() and np.isfinite(series.kp_data).all()
    np.testing.assert_array_equal(series.kp_data.view(np.uint32), pc.reference_fill(d_out, "linear")[0].view(np.uint32))
    # with the key off or absent the stage is not called and the series is the fill's alone
    for over in (dict(fill_missing="linear"), dict(fill_missing="linear", fill_donors="off")):
        _, stac, plain = prepare(**over)
        assert [c[0] for c in stac.calls] == ["fill_missing"] and "fill_donors" not in capsys.readouterr().out
        np.testing.assert_array_equal(plain.kp_data.view(np.uint32), pc.reference_fill(raw, "linear")[0].view(np.uint32))
        np.testing.assert_array_equal(plain.marks["kp_gap"], raw_gap)
    # through the files: kp_gap and no new dataset
    rng = np.random.default_rng(0)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    data = StacData(qpos=f(T, 5), xpos=f(T, 2, 3), xquat=f(T, 2, 4), marker_sites=f(T, K, 3), offsets=f(K, 3), kp_data=series.kp_data,
                    names_qpos=["a", "b"], names_xpos=["w", "v"], kp_names=names)
    series.attach(data, 0, T)
    for suffix in [".npz"] + ([".h5"] if io.h5py is not None else []):
        path = io.save_data_to_h5(config=cfg, file_path=tmp_path / f"ik{suffix}", **data.as_dict())
        if suffix == ".npz":
            with np.load(path) as fh:
                datasets = set(fh.files)
        else:
            with io.h5py.File(path, "r") as fh:
                datasets = set(fh.keys())
        assert datasets == TODAY | {"kp_gap"}
        back_cfg, back = io.load_stac_data(path)
        np.testing.assert_array_equal(back.kp_gap, raw_gap)
        assert back_cfg.stac.fill_donors == "auto" and back_cfg.stac.fill_donors_triples == 2
    assert len(io.OPTIONAL_FIELDS) == 5


def test_statistics_of_an_earlier_stage_are_taken_where_one_ran(tmp_path, rodent_cfg, rodent_mocap):
    """reject_pairwise in the same run: the table comes from its statistics (no second pairwise call) and is handed to fill_donors"""
    from stac_mjx_amd.main import _Preflight, _fill_missing_mode, _prepare_series
    from stac_mjx_amd.prep import donor_table

    names = list(rodent_cfg["KEYPOINT_MODEL_PAIRS"].keys())
    K, T = len(names), 64
    raw = np.ascontiguousarray(rodent_mocap[:T], np.float32)

    class WithPairwise(_ReferenceStac):
        def reject_pairwise(self, kp_data, n_sigma, min_dev, votes):
            out, flag, pair_n, _, pair_mad = pw.reference_pairwise(kp_data, n_sigma * pw.MAD_TO_SIGMA, min_dev, votes)
            self.pair_stats = {"pair_n": pair_n, "pair_mad": pair_mad}
            return out, flag

    cfg = hs.stage_cfg(rodent_cfg, n_fit_frames=32, n_frames_per_clip=32, fill_missing="linear", fill_donors="auto", reject_pairwise="mad")
    pre = _Preflight(cfg, T, tmp_path / "fit.h5", kp_names=names)
    pre.check_config()
    pre.fill_mode = _fill_missing_mode(cfg)
    stac = WithPairwise(K)
    series = _prepare_series(stac, cfg, raw.copy(), pre)
    call = [c for c in stac.calls if c[0] == "fill_donors"][0]
    assert np.array_equal(call[1], donor_table(stac.pair_stats, K, 4)) and call[2] == 4
    assert set(series.marks) == {"kp_rejected_pairwise", "kp_rejected", "kp_gap"}
    assert np.array_equal(series.marks["kp_gap"] > 0, series.marks["kp_rejected"] > 0)  # the recording itself has no hole


# ---- what it is worth, on the reference alone -------------------------------------------------------------------------------------
def _table_of(kp, K, n_triples=4):
    from stac_mjx_amd.prep import donor_table

    _, _, pair_n, _, pair_mad = pw.reference_pairwise(kp, pw.THR, pw.MIN_DEV, 2**31 - 1)
    return donor_table({"pair_n": pair_n, "pair_mad": pair_mad}, K, n_triples)


def _errors(truth, filled, holes):
    """distance between the filled and the true position of every punched (frame, keypoint)"""
    T, K = holes.shape
    d = filled.reshape(T, K, 3).astype(np.float64) - truth.reshape(T, K, 3).astype(np.float64)
    return np.sqrt((d * d).sum(axis=2))[holes]


def test_a_rigid_shape_that_turns_is_followed_where_a_line_is_not():
    """6 points, 300 frames, three 40-frame holes per point, the shape turning 0.83 rad over a gap and drifting: the donor fill
    is exact up to the float32 rounding of the input (measured: max 3.5e-8), the straight line is off by the chord (rms 8.9e-3)."""
    T, K = 300, 6
    truth = dc.rigid_series(T, K)
    donor_err, linear_err = [], []
    for k in range(K):
        kp, holes = dc.punch(truth, k, (30 + 7 * k, 120 + 7 * k, 210 + 7 * k), 40)
        assert holes.sum() == 120
        out, gap, src = dc.reference_donor(kp, _table_of(kp, K))
        assert (src[holes] == 1).all() and (gap[holes] == 40).all()
        donor_err.append(_errors(truth, out, holes))
        linear_err.append(_errors(truth, dc.linear_fill(kp), holes))
    donor_err, linear_err = np.concatenate(donor_err), np.concatenate(linear_err)
    rms = lambda e: float(np.sqrt(np.mean(e * e)))  # noqa: E731
    print(f"rigid shape: donor max {donor_err.max():.3g} rms {rms(donor_err):.3g}, linear rms {rms(linear_err):.3g}")
    assert donor_err.max() < 1e-6 and rms(linear_err) > 1e-3


@pytest.mark.parametrize("length", [40, 120])
def test_holes_in_the_golden_recording(rodent_mocap, length):
    """tests/golden/rodent_mocap_1000.npy, one keypoint punched at a time, from frame 60 on every 173 frames (the holes that leave a
    valid frame behind them): the donor fill's rms error is below the straight line's.  It is not so for every keypoint (DESIGN.md §17
    has the table), which is why the option is off by default."""
    truth = np.ascontiguousarray(rodent_mocap, np.float32)
    T, K = truth.shape[0], truth.shape[1] // 3
    assert (T, K) == (1000, 23) and np.isfinite(truth).all()
    don = _table_of(truth, K)  # (of the recording as it is: 40 to 120 missing frames of 1000 in one track do not move a median)
    donor_err, linear_err, worse = [], [], 0
    for k in range(K):
        kp, holes = dc.punch(truth, k, range(60, T, 173), length)
        out, gap, src = dc.reference_donor(kp, don)
        assert (src[holes] >= 1).all() and (src[holes] <= 4).all()
        donor_err.append(_errors(truth, out, holes))
        linear_err.append(_errors(truth, dc.linear_fill(kp), holes))
        worse += np.mean(donor_err[-1] ** 2) > np.mean(linear_err[-1] ** 2)
    donor_err, linear_err = np.concatenate(donor_err), np.concatenate(linear_err)
    rms = lambda e: float(np.sqrt(np.mean(e * e)))  # noqa: E731
    print(f"rodent holes of {length}: donor rms {rms(donor_err):.4g} p99 {np.quantile(donor_err, 0.99):.4g}, linear rms {rms(linear_err):.4g} "
          f"p99 {np.quantile(linear_err, 0.99):.4g}, ratio {rms(donor_err) / rms(linear_err):.3f}, worse for {worse} of {K} keypoints")
    assert rms(donor_err) < rms(linear_err)
