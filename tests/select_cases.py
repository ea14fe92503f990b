"""Cases and checkers of the calibration-frame selection (stac.fit_frames: diverse), shared by tests/test_select_host.py and
tests/test_gpu_select.py: ``cpu_rule``, a CPU build of the rule of csrc/select/stac_select.hpp (select_reference, through
host_scaffold.build_cpu_library), and ``judge`` / ``greedy64``, a numpy float64 judge that shares none of the rule's arithmetic (its
distances are numpy norms in double, its squared distances dot products)."""

import ctypes as C

import numpy as np

import host_scaffold as hs
from conftest import GOLDEN

DRIVER = r"""
#include "select/stac_select.hpp"
extern "C" long long select_rule(const float *kp, long long T, int K, const unsigned char *cand, long long n, long long *sel, float *radius2,
                                 float *vec, float *dmin, unsigned char *flag) {
    return stac::select_reference(kp, T, K, cand, n, (int64_t *)sel, radius2, vec, dmin, flag);
}
extern "C" long long select_bytes(long long T, long long K) { return stac::select_layout(T, K).bytes; }
"""


def cpu_rule(tmp_path_factory):
    """-> rule(kp [T, 3K] float32, cand [T] or None, n) -> (sel [n] int64, radius2 [n] float32, n_selected), and the library"""
    lib = hs.build_cpu_library(tmp_path_factory, "select", DRIVER)
    lib.select_rule.restype = C.c_longlong
    lib.select_rule.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.select_bytes.restype = C.c_longlong
    lib.select_bytes.argtypes = [C.c_longlong, C.c_longlong]

    def rule(kp, cand, n):
        kp = np.ascontiguousarray(kp, dtype=np.float32)
        T, K = kp.shape[0], kp.shape[1] // 3
        c = None if cand is None else np.ascontiguousarray(np.asarray(cand) != 0, dtype=np.uint8)
        sel, radius2 = np.full(n, -7, np.int64), np.full(n, -7.0, np.float32)
        vec, dmin, flag = np.zeros(K * (K - 1) // 2, np.float32), np.zeros(T, np.float32), np.zeros(T, np.uint8)
        got = lib.select_rule(kp.ctypes.data, T, K, c.ctypes.data if c is not None else None, n, sel.ctypes.data, radius2.ctypes.data,
                              vec.ctypes.data, dmin.ctypes.data, flag.ctypes.data)
        return sel, radius2, int(got)

    return rule, lib


# ---- the float64 judge -----------------------------------------------------------------------------------------------------------
def descriptors64(kp):
    """[T, P] float64: the keypoint distances of every frame, pairs (a, b), a < b, in lexicographic order"""
    x = np.asarray(kp, dtype=np.float64).reshape(kp.shape[0], -1, 3)
    a, b = np.triu_indices(x.shape[1], 1)
    return np.linalg.norm(x[:, a] - x[:, b], axis=-1)


def candidates(kp, cand):
    ok = np.isfinite(np.asarray(kp)).all(axis=1)
    return ok if cand is None else ok & (np.asarray(cand) != 0)


def _dist2_to(D, s):
    d = D - D[s]
    return np.einsum("tp,tp->t", d, d)


def greedy64(kp, cand, n):
    """Plain greedy farthest-point picks in float64 (ties to the lowest index; stops at a distance of 0) -> list of frames"""
    ok = candidates(kp, cand)
    if not ok.any():
        return []
    D = descriptors64(np.where(ok[:, None], kp, 0.0))
    picks = [int(np.flatnonzero(ok)[0])]
    dmin = np.where(ok, np.inf, -1.0)
    while len(picks) < n:
        dmin = np.where(ok, np.minimum(dmin, _dist2_to(D, picks[-1])), -1.0)
        s = int(np.argmax(dmin))  # (the first of equal maxima)
        if not dmin[s] > 0:
            break
        picks.append(s)
    return picks


def judge(kp, cand, n, sel, radius2, n_selected, slack=1e-5, label=""):
    """The properties of a selection against float64: the first pick is the lowest-index candidate; given the picks before it,
    every pick's float64 dmin is at least (1 - slack) of the float64 maximum over the candidates; radius2 is non-increasing from
    index 1 and equals the pick's float64 dmin to float32 accuracy; no pick is a non-candidate or repeats; the tails are -1 / NaN; and
    where the selection stopped early, no candidate is left at a float64 distance above what float32 can take for 0.
    Float32 accuracy, from the formats: a float32 distance d is within delta = 4 * 2^-23 * max d of the float64 one (five roundings of
    the subtraction, squares, sums and root, generously), so e = d - d' is within 2 delta, e^2 within 4 delta |e| + 4 delta^2, and the
    sum of P of them, each addition rounding by 2^-24 relative, within 4 delta sqrt(P acc) + 4 P delta^2 + P 2^-23 acc of acc."""
    ok = candidates(kp, cand)
    sel, radius2 = np.asarray(sel), np.asarray(radius2)
    assert sel.shape == (n,) and radius2.shape == (n,) and 0 <= n_selected <= n, label
    assert (sel[n_selected:] == -1).all() and np.isnan(radius2[n_selected:]).all(), label
    if not ok.any():
        assert n_selected == 0, label
        return
    assert n_selected >= 1 and sel[0] == np.flatnonzero(ok)[0] and np.isposinf(radius2[0]), label
    picks = sel[:n_selected]
    assert ok[picks].all() and len(set(picks.tolist())) == n_selected, label
    assert (np.diff(radius2[1:n_selected]) <= 0).all(), label
    D = descriptors64(np.where(ok[:, None], kp, 0.0))
    P = D.shape[1]
    delta = 4.0 * 2.0 ** -23 * float(D.max())
    bound = lambda acc: 4.0 * delta * np.sqrt(P * acc) + 4.0 * P * delta * delta + P * 2.0 ** -23 * acc  # noqa: E731
    dmin = np.full(kp.shape[0], np.inf)
    for i in range(1, n_selected):
        dmin = np.minimum(dmin, _dist2_to(D, picks[i - 1]))
        best = float(dmin[ok].max())
        assert dmin[picks[i]] >= (1.0 - slack) * best, (label, i, dmin[picks[i]], best)
        assert abs(float(radius2[i]) - dmin[picks[i]]) <= bound(dmin[picks[i]]), (label, i, float(radius2[i]), dmin[picks[i]])
    if n_selected < n:
        dmin = np.minimum(dmin, _dist2_to(D, picks[-1]))
        assert float(dmin[ok].max()) <= 16.0 * P * delta * delta, (label, "stopped early with a candidate left")


# ---- recordings ------------------------------------------------------------------------------------------------------------------
def golden_rodent():
    return np.load(GOLDEN / "rodent_mocap_1000.npy").astype(np.float32)


def resting(kp):
    """A mostly resting recording of the same animal: rows 0..39 forwards and backwards eleven times (880 frames), then rows 500..619"""
    lap = np.concatenate([np.arange(40), np.arange(39, -1, -1)])
    rows = np.concatenate([np.tile(lap, 11), np.arange(500, 620)])
    assert rows.size == 1000
    return np.ascontiguousarray(kp[rows]), rows


def series(T, K, seed):
    return np.random.default_rng(seed).normal(0.0, 0.05, (T, 3 * K)).astype(np.float32)


KS = (2, 3, 23, 64)
TS = (1, 63, 64, 65, 255, 256, 257)
NS = (1, 2, 30)
T_PARTIALS, K_PARTIALS = 16643, 23    # 66 workgroups of the update pass: more partials than one wavefront of the pick, ragged tail
T_STRIDED, K_STRIDED = 1024 * 256 + 5, 3  # more frames than the capped grid has threads: it strides


def shape_cases(K, T):
    """(label, kp, cand, n) for one shape: plain series with cand NULL / all ones / sparse and the n of NS that fit"""
    out = []
    for j, n in enumerate(NS):
        if n > T and n != NS[0]:
            continue
        kp = series(T, K, 1000 * K + T + j)
        cand = (None, np.ones(T, np.uint8), (np.random.default_rng(T + K).random(T) < 0.6).astype(np.uint8))[j % 3]
        if cand is not None and j % 3 == 2 and T >= 2:
            cand[[0, T - 1]] = 0  # (the first pick moves)
        out.append((f"K{K}_T{T}_n{min(n, T)}", kp, cand, min(n, T)))
    return out


def edge_cases():
    """Cases by what they are about, at the smallest shapes where it can go wrong"""
    out = []
    K = 3
    kp = series(65, K, 1)
    out.append(("all_candidates_T65", kp, None, 65))  # n equal to all candidates
    cand = np.ones(65, np.uint8)
    cand[::3] = 0
    out.append(("all_sparse_candidates_T65", kp, cand, int(cand.sum())))
    kp = series(600, K, 2)  # missing frames in the first and the last block (three blocks of 256)
    kp[0, 4] = np.nan
    kp[3, 0] = np.inf
    kp[599, 8] = -np.inf
    kp[590:597] = np.nan
    out.append(("missing_first_last_block", kp, None, 30))
    kp = series(600, K, 3)  # two equal farthest frames on both sides of a block border: the lower index is picked
    kp[255] = kp[256] = 3.0 * series(1, K, 4)[0]
    kp[511] = kp[512] = kp[63] = kp[64]
    out.append(("ties_across_block_borders", kp, None, 30))
    kp = np.tile(series(1, 23, 5), (300, 1))  # all frames equal: one pick, tails -1 / NaN
    out.append(("all_equal", kp, None, 30))
    kp = np.tile(series(5, K, 6), (60, 1))  # 5 distinct rows among 300: stops at 5
    out.append(("five_distinct", kp, None, 30))
    kp = series(70, K, 7)
    kp[:] = np.nan  # no candidate at all
    out.append(("no_candidate", kp, None, 3))
    kp = series(70, 2, 8)
    out.append(("none_allowed", kp, np.zeros(70, np.uint8), 3))
    return out
