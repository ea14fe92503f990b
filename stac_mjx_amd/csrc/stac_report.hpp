// Fit report: per-keypoint marker errors and exact quantiles (stac_report.hip).  DESIGN.md "Fit report".
//
// What the kernels, a CPU statement of the same passes (tests/test_report_host.py) and the numpy reference share: the error of a
// (frame, keypoint) pair, which pairs are counted, the key a counted pair is selected by, the digits of the three-pass radix
// select, the rank rule and the workspace layout.  Host + device inline functions; every float64 operation is a single IEEE
// operation in a stated order (the library is built with -ffp-contract=off).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define STAC_REPORT_HD __host__ __device__ inline
#else
#define STAC_REPORT_HD inline
#endif

namespace stac {

constexpr int kReportTileFrames = 64;   // frames of a tile of the first pass: one wavefront lane per frame
constexpr int kReportMaxBlocks = 1024;  // 256 CUs x 4 workgroups: the grid strides over the work beyond that
constexpr int kReportSegFrames = 8192;  // frames of one keypoint that a workgroup of a counting pass histograms at a time
constexpr int kReportMaxQuant = 8;      // quantiles of a call at most
constexpr int kReportBins0 = 1024;      // bits >> 21 of a non-negative float: the `hist` output
constexpr int kReportBins1 = 2048;      // (bits >> 10) & 0x7FF
constexpr int kReportBins2 = 1024;      // bits & 0x3FF
constexpr uint32_t kReportNanBits = 0x7FC00000u;
constexpr uint32_t kReportNoKey = 0xFFFFFFFFu;  // key of a pair that is not counted; as a prefix: matches no key

STAC_REPORT_HD bool report_finite(float v) {  // the exponent bits are not all ones (a bit test: no compiler flag can fold it away)
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return (b & 0x7F800000u) != 0x7F800000u;
}

STAC_REPORT_HD uint32_t report_bits(float v) {
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return b;
}

STAC_REPORT_HD float report_float(uint32_t b) {
    float v;
    __builtin_memcpy(&v, &b, 4);
    return v;
}

// One (frame, keypoint) pair: e = the squared distance in double, left to right; sqerr = (float)e, or the quiet NaN when one of
// the six inputs is not finite; counted iff the six are finite and gap == 0; key = the bits of sqerr if counted, else kReportNoKey.
struct ReportPair {
    double e;
    float sqerr;
    bool counted;
    uint32_t key;
};

STAC_REPORT_HD ReportPair report_pair(float m0, float m1, float m2, float y0, float y1, float y2, int32_t gap) {
    ReportPair p;
    const bool fin = report_finite(m0) && report_finite(m1) && report_finite(m2) && report_finite(y0) && report_finite(y1) && report_finite(y2);
    const double d0 = (double)m0 - (double)y0, d1 = (double)m1 - (double)y1, d2 = (double)m2 - (double)y2;
    const double a = d0 * d0, b = d1 * d1, c = d2 * d2;
    const double ab = a + b;
    p.e = ab + c;
    p.sqerr = fin ? (float)p.e : report_float(kReportNanBits);
    p.counted = fin && gap == 0;
    p.key = p.counted ? report_bits(p.sqerr) : kReportNoKey;
    return p;
}

// Nearest rank, lower: the index into the ascending counted values of a keypoint (count >= 1)
STAC_REPORT_HD int64_t report_rank(int32_t permille, int64_t count) { return ((int64_t)permille * (count - 1)) / 1000; }

// The three passes of the select: pass 0 counts every counted key by its top 11 bits, pass 1 the keys whose top 11 bits equal the
// prefix by their next 11, pass 2 the keys whose top 22 bits equal the prefix by their last 10.
STAC_REPORT_HD bool report_match(int pass, uint32_t key, uint32_t prefix) {
    return pass == 0 ? (key >> 21) < (uint32_t)kReportBins0 : (pass == 1 ? (key >> 21) == prefix : (key >> 10) == prefix);
}
STAC_REPORT_HD uint32_t report_digit(int pass, uint32_t key) { return pass == 0 ? key >> 21 : (pass == 1 ? (key >> 10) & 0x7FFu : key & 0x3FFu); }
STAC_REPORT_HD int report_bins(int pass) { return pass == 1 ? kReportBins1 : kReportBins0; }

// The bin that holds rank `rank` of the values counted in bins[0 .. n): the smallest d with bins[0] + .. + bins[d] > rank, and
// the rank inside it.  The caller guarantees rank < the total; the scan stops at the last bin whatever it is given.
STAC_REPORT_HD void report_select(const uint64_t *bins, int n, uint64_t rank, uint32_t *digit, uint64_t *rank_in) {
    uint64_t cum = 0;
    int d = 0;
    while (d < n - 1 && cum + bins[d] <= rank) cum += bins[d++];
    *digit = (uint32_t)d;
    *rank_in = rank - cum;
}

// Maximum and argmax of a tile as one word: (key << 32) | (64 - f) for the counted frame f of the tile with the largest key, the
// smallest such f; 0 = the tile has no counted frame.  Larger words are better inside a tile; between tiles the key decides and
// the lower tile index keeps a tie.
STAC_REPORT_HD uint64_t report_pack(uint32_t key, int f) { return ((uint64_t)key << 32) | (uint64_t)(kReportTileFrames - f); }
STAC_REPORT_HD bool report_tile_wins(uint64_t best, int64_t best_tile, uint64_t cand, int64_t cand_tile) {
    return cand != 0 && (best == 0 || (cand >> 32) > (best >> 32) || ((cand >> 32) == (best >> 32) && cand_tile < best_tile));
}

// What the select of one (keypoint, quantile) has narrowed down so far
struct ReportSel {
    uint64_t rank;    // rank inside the values that match the prefix
    uint32_t prefix;  // the top 11 (after pass 0) or 22 (after pass 1) bits of the quantile; kReportNoKey: count == 0
    uint32_t pad;
};

// Workspace of stac_report_errors (byte offsets, all multiples of 8): keys uint32 [K][stride] (the keys, one row per keypoint),
// psum double [K][tiles] and pmax uint64 [K][tiles] (per-tile partials), hist1 uint64 [K][Q][2048], hist2 uint64 [K][Q][1024],
// sel ReportSel [K][Q].  bytes < 0: bad arguments (or a size beyond int64).
struct ReportLayout {
    int64_t tiles, stride, nseg, keys, psum, pmax, hist1, hist2, sel, bytes;
};

STAC_REPORT_HD ReportLayout report_layout(int64_t N, int64_t K, int64_t Q) {
    ReportLayout L = {0, 0, 0, 0, 0, 0, 0, 0, 0, -1};
    if (N < 1 || K < 1 || Q < 1 || Q > kReportMaxQuant) return L;
    L.tiles = (N - 1) / kReportTileFrames + 1;
    L.stride = L.tiles * kReportTileFrames;
    L.nseg = (N - 1) / kReportSegFrames + 1;
    const int64_t per_kp = L.tiles * (4 * kReportTileFrames + 16) + Q * (8 * (kReportBins1 + kReportBins2) + 16);
    if (per_kp > ((int64_t)1 << 60) / K) return L;
    L.keys = 0;
    L.psum = L.keys + 4 * K * L.stride;
    L.pmax = L.psum + 8 * K * L.tiles;
    L.hist1 = L.pmax + 8 * K * L.tiles;
    L.hist2 = L.hist1 + 8 * K * Q * kReportBins1;
    L.sel = L.hist2 + 8 * K * Q * kReportBins2;
    L.bytes = L.sel + 16 * K * Q;
    return L;
}

}  // namespace stac
