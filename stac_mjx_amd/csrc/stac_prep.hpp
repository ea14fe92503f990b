// Filling missing keypoints along time before the fit (stac_prep.hip).  DESIGN.md "Filling missing keypoints".
//
// The three things the kernels, a CPU statement of the same staged scan (tests/test_prep_host.py) and the numpy reference share:
// the missing test, the value / gap rule, and the combine of two tile summaries.  Host + device inline functions; every float64
// operation is a single IEEE operation in a stated order (the library is built with -ffp-contract=off).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define STAC_PREP_HD __host__ __device__ inline
#else
#define STAC_PREP_HD inline
#endif

namespace stac {

enum { kPrepLinear = 0, kPrepHold = 1 };  // the `mode` of stac_prep_fill

constexpr int kPrepTileFrames = 64;   // frames of a tile of the kernels: one wavefront ballot is a keypoint's validity mask of a tile
constexpr int kPrepMaxBlocks = 1024;  // 256 CUs x 4 workgroups: the grid strides over the tiles beyond that

STAC_PREP_HD int64_t prep_tiles(int64_t T, int64_t tile) { return (T + tile - 1) / tile; }

// Workspace of stac_prep_fill: four int64 arrays [K][tiles] (first, last: the tile summaries; prev, next: the carries).
// -1: bad arguments (or a size beyond int64).
STAC_PREP_HD int64_t prep_workspace_bytes(int64_t T, int64_t K) {
    if (T < 1 || K < 1) return -1;
    const int64_t tiles = prep_tiles(T, kPrepTileFrames);
    if (tiles > ((int64_t)1 << 57) / K) return -1;
    return 32 * K * tiles;
}

// finite: the exponent bits are not all ones (a bit test: no compiler flag can fold it away)
STAC_PREP_HD bool prep_finite(float v) {
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return (b & 0x7F800000u) != 0x7F800000u;
}

// A keypoint is missing in a frame iff any of its three coordinates is NaN, +inf or -inf
STAC_PREP_HD bool prep_missing(float x, float y, float z) { return !(prep_finite(x) && prep_finite(y) && prep_finite(z)); }

// Summary of one keypoint over a range of frames: its first and last valid frame index (absolute), -1 = the range has none
struct PrepSummary {
    int64_t first, last;
};

STAC_PREP_HD PrepSummary prep_none() { return PrepSummary{-1, -1}; }

// Summary of the range a followed by the range b (a lies before b in time).  Associative; prep_none() is its identity.
STAC_PREP_HD PrepSummary prep_combine(PrepSummary a, PrepSummary b) {
    return PrepSummary{a.first >= 0 ? a.first : b.first, b.last >= 0 ? b.last : a.last};
}

// One coordinate of a MISSING keypoint in frame t.  p: the largest valid frame < t (-1: none), with value a there;
// n: the smallest valid frame > t (-1: none), with value b.  At least one of p, n exists (an empty track is not filled).
STAC_PREP_HD float prep_fill(int32_t mode, int64_t t, int64_t p, int64_t n, float a, float b) {
    if (p < 0) return b;  // leading run
    if (n < 0) return a;  // trailing run
    if (mode == kPrepHold) return (t - p) <= (n - t) ? a : b;  // the nearer one, a tie to p
    const double w = (double)(t - p) / (double)(n - p);
    const double d = (double)b - (double)a;
    const double s = d * w;
    return (float)((double)a + s);
}

// Length of the missing run that frame t of a track of T frames belongs to (p, n as above), saturated to int32
STAC_PREP_HD int32_t prep_gap(int64_t p, int64_t n, int64_t T) {
    const int64_t g = (p < 0 && n < 0) ? T : (p < 0 ? n : (n < 0 ? T - 1 - p : n - p - 1));
    return g > 2147483647 ? 2147483647 : (int32_t)g;
}

}  // namespace stac
