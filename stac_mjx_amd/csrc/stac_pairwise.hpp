// Rejecting keypoints that break pairwise distances before the fit (stac_pairwise.hip).  DESIGN.md "Rejecting keypoints by pairwise
// distances".
//
// The distance between two keypoints has a distribution over the whole recording; a keypoint that is swapped or displaced in a frame
// leaves many of those distributions at once, however long the defect lasts.  For the pairs (a, b), a < b, in lexicographic order
// (p = a (2K - a - 1) / 2 + (b - a - 1), P = K (K - 1) / 2), missing as in stac_prep.hpp:
//   d_p(t) = sqrtf((dx*dx + dy*dy) + dz*dz), dx = x_a - x_b, all in float32; the pair is VALID in frame t iff neither keypoint is
//            missing there and d_p(t) is finite; n_p = the number of valid frames.  n_p < 3: the pair decides nothing, its med and mad
//            are the quiet NaN 0x7FF8000000000000.
//   med_p  = 0.5 * ((double)s[(n-1)/2] + (double)s[n/2]), s = the valid d_p in ascending order
//   e_p(t) = (float)fabs((double)d_p(t) - med_p)
//   mad_p  = 0.5 * ((double)E[(n-1)/2] + (double)E[n/2]), E = the e_p in ascending order
//   pair p is BAD in frame t iff it is valid there and (double)e_p(t) > thr * mad_p and (double)e_p(t) > min_dev (both strict).
// Blame, per frame: c_k = the number of bad pairs that contain k; take k* with the largest c_k (ties to the lowest k); stop if
// c_k* < votes; else reject k*, remove every pair that contains it, and repeat.  A rejected keypoint leaves as three quiet NaN
// 0x7FC00000 with flag 1; everything else passes bit for bit.
//
// What the kernels, the CPU program of tests/test_pairwise_host.py and the numpy reference share is below.  d and e are
// non-negative finite float32, so their bit patterns sort like their values: the order statistics are selected exactly by the
// three histogram passes of stac_report.hpp over those bits (the KEY of a pair in a frame; kReportNoKey where it is not valid).
// Every floating-point operation is a single IEEE operation in a stated order (the library is built with -ffp-contract=off).
#pragma once

#include <stdint.h>

#include "stac_prep.hpp"
#include "stac_report.hpp"

#if defined(__HIPCC__)
#define STAC_PAIRWISE_HD __host__ __device__ inline
#else
#define STAC_PAIRWISE_HD inline
#endif

namespace stac {

constexpr int kPairwiseMaxKp = 64;        // one frame's bad pairs are 64 words of 64 bits
constexpr int kPairwiseTileFrames = 64;   // frames of a tile: one wavefront lane per frame
constexpr int kPairwiseMaxBlocks = 1024;  // workgroups of 256 threads of a launch at most: the grids stride over the work beyond that
constexpr int kPairwiseMaxWaves = 4096;   // workgroups of ONE wavefront (the decision pass) of a launch at most
constexpr uint32_t kPairwiseNanBits = 0x7FC00000u;
constexpr uint64_t kPairwiseNan64Bits = 0x7FF8000000000000ull;

STAC_PAIRWISE_HD int64_t pairwise_pairs(int64_t K) { return K * (K - 1) / 2; }
STAC_PAIRWISE_HD int64_t pairwise_index(int64_t a, int64_t b, int64_t K) { return a * (2 * K - a - 1) / 2 + (b - a - 1); }  // a < b

STAC_PAIRWISE_HD double pairwise_nan64() {
    const uint64_t b = kPairwiseNan64Bits;
    double v;
    __builtin_memcpy(&v, &b, 8);
    return v;
}

// d_p(t): five float32 operations and one correctly rounded float32 square root
STAC_PAIRWISE_HD float pairwise_dist(float xa, float ya, float za, float xb, float yb, float zb) {
    const float dx = xa - xb, dy = ya - yb, dz = za - zb;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float xy = xx + yy;
    const float s = xy + zz;
    return __builtin_sqrtf(s);
}

// The key of a pair in a frame: the bits of d_p(t), or kReportNoKey where the pair is not valid
STAC_PAIRWISE_HD uint32_t pairwise_key(float xa, float ya, float za, float xb, float yb, float zb) {
    if (prep_missing(xa, ya, za) || prep_missing(xb, yb, zb)) return kReportNoKey;
    const float d = pairwise_dist(xa, ya, za, xb, yb, zb);
    return prep_finite(d) ? report_bits(d) : kReportNoKey;
}

// The median of n values from its two middle order statistics s[(n-1)/2] and s[n/2]: one double addition, one multiplication
STAC_PAIRWISE_HD double pairwise_median(float s0, float s1) {
    const double sum = (double)s0 + (double)s1;
    return 0.5 * sum;
}

// e_p(t): one double subtraction, one rounding to float32
STAC_PAIRWISE_HD float pairwise_dev(float d, double med) { return (float)__builtin_fabs((double)d - med); }

// The key of e_p(t) from the key of d_p(t)
STAC_PAIRWISE_HD uint32_t pairwise_dev_key(uint32_t key, double med) {
    return key == kReportNoKey ? kReportNoKey : report_bits(pairwise_dev(report_float(key), med));
}

// bound = thr * mad_p: one double multiplication per pair
STAC_PAIRWISE_HD bool pairwise_bad(float e, double bound, double min_dev) { return (double)e > bound && (double)e > min_dev; }

STAC_PAIRWISE_HD int pairwise_popcount(uint64_t v) { return __builtin_popcountll(v); }

// The blame of one frame.  m[k * stride], k < K: bit j is set iff the pair {k, j} is bad in the frame (symmetric, no diagonal).
// -> the rejected keypoints as bits; m is consumed.  No array is kept: a frame's words live where the caller put them (the
// kernel: a column of LDS per lane).
STAC_PAIRWISE_HD uint64_t pairwise_blame(uint64_t *m, int64_t stride, int32_t K, int32_t votes) {
    uint64_t rejected = 0;
    for (;;) {
        int32_t best = 0, c_best = -1;
        for (int32_t k = 0; k < K; ++k) {
            const int32_t c = pairwise_popcount(m[k * stride]);
            if (c > c_best) {  // (strict: a tie keeps the lowest k)
                c_best = c;
                best = k;
            }
        }
        if (c_best < votes) return rejected;  // (votes >= 1: a keypoint without a bad pair is never rejected)
        const uint64_t bit = 1ull << best;
        rejected |= bit;
        for (int32_t k = 0; k < K; ++k) m[k * stride] &= ~bit;
        m[best * stride] = 0;
    }
}

// Workspace of stac_prep_pairwise (byte offsets, all multiples of 8): keys uint32 [P][stride] (the bits of d_p(t), one row per pair),
// hist0 uint64 [P][1024], hist1 uint64 [P][2][2048], hist2 uint64 [P][2][1024] (the histograms of the three passes, for the two
// ranks of a median), sel ReportSel [P][2].  bytes < 0: bad arguments (or a size beyond int64).  K = 1 has no pairs: 8 bytes.
struct PairwiseLayout {
    int64_t pairs, tiles, stride, nseg, keys, hist0, hist1, hist2, sel, bytes;
};

STAC_PAIRWISE_HD PairwiseLayout pairwise_layout(int64_t T, int64_t K) {
    PairwiseLayout L = {0, 0, 0, 0, 0, 0, 0, 0, 0, -1};
    if (T < 1 || K < 1 || K > kPairwiseMaxKp || T > ((int64_t)1 << 44)) return L;
    L.pairs = pairwise_pairs(K);
    L.tiles = (T - 1) / kPairwiseTileFrames + 1;
    L.stride = L.tiles * kPairwiseTileFrames;
    L.nseg = (T - 1) / kReportSegFrames + 1;
    L.keys = 0;
    L.hist0 = L.keys + 4 * L.pairs * L.stride;
    L.hist1 = L.hist0 + 8 * L.pairs * kReportBins0;
    L.hist2 = L.hist1 + 8 * L.pairs * 2 * kReportBins1;
    L.sel = L.hist2 + 8 * L.pairs * 2 * kReportBins2;
    L.bytes = L.sel + 16 * L.pairs * 2;
    if (L.bytes < 8) L.bytes = 8;
    return L;
}

}  // namespace stac
