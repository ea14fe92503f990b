// Rejecting keypoint outliers along time before the fit (stac_outlier.hip).  DESIGN.md "Rejecting keypoint outliers".
//
// The Hampel identifier per track and coordinate: a sliding median and median absolute deviation over the frames
// max(0, t-h) .. min(T-1, t+h) in which the keypoint is not missing (missing as in stac_prep.hpp: a coordinate that is not finite).
//   n < 3: the coordinate decides nothing.         s = the n window values (float32) in ascending order,
//   med = 0.5 * ((double)s[(n-1)/2] + (double)s[n/2])         d_j = fabs((double)x_j - med),  D = the d_j in ascending order,
//   mad = 0.5 * (D[(n-1)/2] + D[n/2])             outlier iff d_centre > thr * mad  AND  d_centre > min_dev   (both strict).
// A keypoint that is not missing is REJECTED in a frame iff one of its coordinates is an outlier; its three coordinates leave as
// the quiet NaN 0x7FC00000 and its flag as 1; everything else passes bit for bit.  Every decision reads input values only.
//
// What the kernel, the CPU program of tests/test_outlier_host.py and the numpy reference share is outlier_coord below.  It selects
// by RANK COUNTING: the value v is s[r] iff #{x_i < v} <= r < #{x_i <= v}, so nothing is sorted and no array is kept; ties are
// selected by value (+0.0 and -0.0 may fall either way; d does not depend on which).  It works on a SANITIZED series: all three
// coordinates of a missing keypoint, and every frame outside the series, hold NaN, and since every comparison with a NaN is false
// such an entry counts for nothing.  Every float64 operation is a single IEEE operation in a stated order (the library is built with
// -ffp-contract=off -fno-fast-math).
#pragma once

#include <stdint.h>

#include "stac_prep.hpp"

#if defined(__HIPCC__)
#define STAC_OUTLIER_HD __host__ __device__ inline
#else
#define STAC_OUTLIER_HD inline
#endif

namespace stac {

constexpr int kOutlierMaxHalf = 16;  // largest half-width h of the window (2 h + 1 = 33 frames)

// the value a rejected coordinate leaves as, and the value a missing keypoint / a frame outside the series holds in a sanitized series
STAC_OUTLIER_HD float outlier_nan() {
    const uint32_t b = 0x7FC00000u;
    float v;
    __builtin_memcpy(&v, &b, 4);
    return v;
}

STAC_OUTLIER_HD double outlier_abs(double v) { return __builtin_fabs(v); }  // (clears the sign bit; a NaN stays a NaN)

// One coordinate of one keypoint in one frame.  x points at the centre value in a sanitized series (see above) whose frames lie
// `stride` floats apart; the frames -h .. +h around the centre are readable.  The centre is not missing (not NaN).
STAC_OUTLIER_HD bool outlier_coord(const float *x, int64_t stride, int32_t h, double thr, double min_dev) {
    int32_t n = 0;
    for (int32_t i = -h; i <= h; ++i) {
        const float xi = x[i * stride];
        n += xi == xi ? 1 : 0;
    }
    if (n < 3) return false;
    const int32_t r0 = (n - 1) / 2, r1 = n / 2;
    float s0 = 0.0f, s1 = 0.0f;
    for (int32_t j = -h; j <= h; ++j) {
        const float xj = x[j * stride];
        int32_t lt = 0, le = 0;
        for (int32_t i = -h; i <= h; ++i) {
            const float xi = x[i * stride];
            lt += xi < xj ? 1 : 0;
            le += xi <= xj ? 1 : 0;
        }
        if (lt <= r0 && r0 < le) s0 = xj;  // (a NaN x_j has lt = le = 0 and is never selected)
        if (lt <= r1 && r1 < le) s1 = xj;
    }
    const double sum = (double)s0 + (double)s1;
    const double med = 0.5 * sum;
    const double dc = outlier_abs((double)x[0] - med);
    if (!(dc > min_dev)) return false;  // (decided already: the deviations need no ranking)
    double D0 = 0.0, D1 = 0.0;
    for (int32_t j = -h; j <= h; ++j) {
        const double dj = outlier_abs((double)x[j * stride] - med);
        int32_t lt = 0, le = 0;
        for (int32_t i = -h; i <= h; ++i) {
            const double di = outlier_abs((double)x[i * stride] - med);
            lt += di < dj ? 1 : 0;
            le += di <= dj ? 1 : 0;
        }
        if (lt <= r0 && r0 < le) D0 = dj;
        if (lt <= r1 && r1 < le) D1 = dj;
    }
    const double dsum = D0 + D1;
    const double mad = 0.5 * dsum;
    const double bound = thr * mad;
    return dc > bound;
}

}  // namespace stac
