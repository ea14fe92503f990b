// Filling long keypoint gaps from rigid neighbours (stac_donor.hip).  DESIGN.md "Filling gaps from donor keypoints".
//
// The rule as host + device inline functions: what the kernel, a CPU statement of it (tests/test_donor_host.py) and the numpy
// reference (tests/donor_cases.py) share.  Everything is double arithmetic on exactly converted floats, every operation one of
// + - * / in a stated order (the library is built with -ffp-contract=off), no square root anywhere, and one rounding to float32 at
// the end.  p, n and the missing test are those of stac_prep.hpp.
#pragma once

#include <stdint.h>

#include "stac_prep.hpp"

namespace stac {

constexpr int kDonorMaxKp = 64;      // keypoints of stac_prep_donor at most (one chunk of the tile walk holds every keypoint's mask)
constexpr int kDonorMaxTriples = 8;  // donor triples per keypoint at most: the D of don [K][D][3]

enum { kDonorObserved = 0, kDonorLeft = 255 };  // src: 0 observed, d + 1 filled by triple d, 255 missing and left so

STAC_PREP_HD double donor_dot(const double *x, const double *y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

// The frame of a donor triple in one frame of the series: origin a, the axes u = b - a, w = (c - a) less its part along u, and
// m = u x w, none of them normalised, with their squared lengths
struct DonorFrame {
    double a[3], u[3], w[3], m[3], uu, ww, mm;
};

// Row d of a keypoint's donor list is a triple iff it names three different keypoints of 0 .. K - 1, all different from k; the first
// row that is not ends the list (and is never used as an address)
STAC_PREP_HD bool donor_row(int32_t k, int32_t K, int32_t a, int32_t b, int32_t c) {
    return a >= 0 && a < K && b >= 0 && b < K && c >= 0 && c < K && a != b && a != c && b != c && a != k && b != k && c != k;
}

// -> whether the three donors at pa, pb, pc (three floats each, none missing) span a frame: uu > 0, ww > 0, mm > 0
STAC_PREP_HD bool donor_frame(const float *pa, const float *pb, const float *pc, DonorFrame &F) {
    double v[3];
    for (int i = 0; i < 3; ++i) {
        F.a[i] = (double)pa[i];
        F.u[i] = (double)pb[i] - F.a[i];
        v[i] = (double)pc[i] - F.a[i];
    }
    F.uu = donor_dot(F.u, F.u);
    const double s = donor_dot(v, F.u) / F.uu;
    for (int i = 0; i < 3; ++i) F.w[i] = v[i] - s * F.u[i];
    F.ww = donor_dot(F.w, F.w);
    F.m[0] = F.u[1] * F.w[2] - F.u[2] * F.w[1];
    F.m[1] = F.u[2] * F.w[0] - F.u[0] * F.w[2];
    F.m[2] = F.u[0] * F.w[1] - F.u[1] * F.w[0];
    F.mm = donor_dot(F.m, F.m);
    return F.uu > 0.0 && F.ww > 0.0 && F.mm > 0.0;
}

// The local coordinates L = (alpha, beta, gamma) of keypoint k in the frame of the donors (a, b, c), all in the row `row` [3K] of the
// series, in which k is valid -> false if a donor is missing there or the donors span no frame (L is then not to be used).  Written
// without an early return: on the device every lane of a wavefront runs the same instructions.
STAC_PREP_HD bool donor_local(const float *row, int32_t k, int32_t a, int32_t b, int32_t c, double *L) {
    const float *pa = row + 3 * a, *pb = row + 3 * b, *pc = row + 3 * c, *x = row + 3 * k;
    const bool present = !(prep_missing(pa[0], pa[1], pa[2]) || prep_missing(pb[0], pb[1], pb[2]) || prep_missing(pc[0], pc[1], pc[2]));
    DonorFrame F;
    const bool spans = donor_frame(pa, pb, pc, F);
    double r[3];
    for (int i = 0; i < 3; ++i) r[i] = (double)x[i] - F.a[i];
    L[0] = donor_dot(r, F.u) / F.uu;
    L[1] = donor_dot(r, F.w) / F.ww;
    L[2] = donor_dot(r, F.m) / F.mm;
    return present && spans;
}

// One triple (a, b, c), a row by donor_row, for the MISSING keypoint k of frame t of kp [T][K3].  p: the largest valid frame < t of
// track k (-1: none), n: the smallest valid one > t (-1: none), at least one of them exists; the caller has seen that no donor is
// missing in frame t itself.  -> whether the triple is usable, and then o[3], the value.  (A run with one neighbour reads that
// neighbour for both ends and selects its coordinates: nothing is interpolated.)
STAC_PREP_HD bool donor_try(const float *kp, int64_t K3, int64_t t, int64_t p, int64_t n, int32_t k, int32_t a, int32_t b, int32_t c,
                            float *o) {
    const float *rt = kp + t * K3;
    const bool both = p >= 0 && n >= 0;
    DonorFrame F;
    bool ok = donor_frame(rt + 3 * a, rt + 3 * b, rt + 3 * c, F);
    double Lp[3], Ln[3], L[3];
    ok = donor_local(kp + (p >= 0 ? p : n) * K3, k, a, b, c, Lp) && ok;
    ok = donor_local(kp + (n >= 0 ? n : p) * K3, k, a, b, c, Ln) && ok;
    const double wgt = both ? (double)(t - p) / (double)(n - p) : 0.0;
    for (int i = 0; i < 3; ++i) {
        const double d = Ln[i] - Lp[i];
        const double s = d * wgt;
        const double v = Lp[i] + s;
        L[i] = both ? v : Lp[i];  // (one neighbour: Lp and Ln are the same, held in the donors' frame)
    }
    for (int i = 0; i < 3; ++i) o[i] = (float)(((F.a[i] + L[0] * F.u[i]) + L[1] * F.w[i]) + L[2] * F.m[i]);
    return ok && prep_finite(o[0]) && prep_finite(o[1]) && prep_finite(o[2]);
}

}  // namespace stac
