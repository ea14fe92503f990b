// Repairing left / right keypoint swaps before the fit (pairwise_swap_kernel of stac_pairwise.hip).  DESIGN.md "Repairing keypoint
// swaps".
//
// Two keypoints that carry each other's label in a frame were both observed correctly; the distances say so.  With n_p, med_p, mad_p
// and the key of every (pair, frame) exactly as in stac_pairwise.hpp, computed over the series as given, and S CANDIDATES (a_s, b_s),
// a != b, every keypoint in at most one of them: for a candidate (a, b) in a frame t, every k outside {a, b} COUNTS iff the pairs
// {a, k} and {b, k} both have n >= 3 and are both valid in t, and then, with
//   bad(d; p) = pairwise_bad(pairwise_dev(d, med_p), thr * mad_p, min_dev)   (the single IEEE operations of stac_pairwise.hpp)
//   b0 += bad(d_ak(t); {a, k}) + bad(d_bk(t); {b, k})   the frame as it is labelled
//   b1 += bad(d_bk(t); {a, k}) + bad(d_ak(t); {b, k})   the frame with the two labels exchanged
// The candidate SWAPS in the frame iff b0 >= min_bad and 2 * b1 <= b0 (integers).  Every decision is taken from the input frame:
// decisions do not depend on each other or on another frame.  Where a candidate swaps, the three words of a and of b are exchanged
// bit for bit; every other element passes bit for bit.  A candidate with a missing keypoint has no valid pair: nothing counts.
//
// What the kernel, the CPU program of tests/test_swaps_host.py and the numpy reference share is below.
#pragma once

#include <stdint.h>

#include "stac_pairwise.hpp"

namespace stac {

constexpr int kSwapMaxCand = kPairwiseMaxKp / 2;  // every keypoint is in at most one candidate
constexpr int kSwapCandWords = kSwapMaxCand / 4;  // the packed table: four candidates of 16 bits (a | b << 8) per word of 64
constexpr uint32_t kSwapNoCand = 0xFFu;           // cand_of of a keypoint that is in no candidate

// The index of the pair {i, j}, i != j, in either order
STAC_PAIRWISE_HD int64_t swap_pair(int64_t i, int64_t j, int64_t K) { return i < j ? pairwise_index(i, j, K) : pairwise_index(j, i, K); }

// bad(d; p) of a valid key: bound = thr * mad_p (one double multiplication per pair, by the caller)
STAC_PAIRWISE_HD int32_t swap_bad(uint32_t key, double med, double bound, double min_dev) {
    return pairwise_bad(pairwise_dev(report_float(key), med), bound, min_dev) ? 1 : 0;
}

// What one third keypoint k adds to b0 and b1.  key_*: the keys of {a, k} and {b, k} in the frame, n_*, med_*, bound_*: of those pairs
STAC_PAIRWISE_HD void swap_count(uint32_t key_ak, uint32_t key_bk, int64_t n_ak, int64_t n_bk, double med_ak, double bound_ak, double med_bk,
                                 double bound_bk, double min_dev, int32_t *b0, int32_t *b1) {
    if (n_ak < 3 || n_bk < 3 || key_ak == kReportNoKey || key_bk == kReportNoKey) return;
    *b0 += swap_bad(key_ak, med_ak, bound_ak, min_dev) + swap_bad(key_bk, med_bk, bound_bk, min_dev);
    *b1 += swap_bad(key_bk, med_ak, bound_ak, min_dev) + swap_bad(key_ak, med_bk, bound_bk, min_dev);
}

// b0 <= 2 (K - 2) <= 124: no overflow
STAC_PAIRWISE_HD bool swap_decide(int32_t b0, int32_t b1, int32_t min_bad) { return b0 >= min_bad && 2 * b1 <= b0; }

// The candidate table as the kernel takes it, by value: candidate s is the 16 bits (a | b << 8) at bit 16 (s & 3) of w[s >> 2]
struct SwapCands {
    unsigned long long w[kSwapCandWords];
};

// Checks cand [n_cand][2] against K and packs it.  -> 0, or 1: a keypoint out of [0, K), 2: a == b, 3: a keypoint in two candidates,
// 4: more candidates than kSwapMaxCand; *at: the candidate that is refused.  HOST.
inline int swap_pack(const int32_t *cand, int32_t n_cand, int32_t K, SwapCands *out, int32_t *at) {
    uint64_t seen = 0;
    for (int i = 0; i < kSwapCandWords; ++i) out->w[i] = 0ull;
    for (int32_t s = 0; s < n_cand; ++s) {
        const int32_t a = cand[2 * s], b = cand[2 * s + 1];
        *at = s;
        if (s >= kSwapMaxCand) return 4;
        if (a < 0 || a >= K || b < 0 || b >= K || a >= kPairwiseMaxKp || b >= kPairwiseMaxKp) return 1;
        if (a == b) return 2;
        if (((seen >> a) | (seen >> b)) & 1ull) return 3;
        seen |= (1ull << a) | (1ull << b);
        out->w[s >> 2] |= (unsigned long long)((uint32_t)a | ((uint32_t)b << 8)) << (16 * (s & 3));
    }
    return 0;
}

}  // namespace stac
