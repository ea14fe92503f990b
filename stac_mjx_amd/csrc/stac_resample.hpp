// Resampling fitted poses to another frame rate (stac_resample.hip): a polyphase Kaiser-windowed sinc filter of x[N, C] per clip,
// up by U and down by D, with the quaternion blocks aligned to the nearest earlier input row, summed and renormalised and the scalar
// columns clamped to the joint bounds.  DESIGN.md "Resampling fitted poses".
//
// Everything here is the index rule, the per-element arithmetic and the tile choice of the kernel, as host + device inline
// functions: a CPU build of this header (tests/test_resample_host.py) runs exactly what the kernel runs.  Every float32 operation
// is a single IEEE operation in a stated order (the library is built with -ffp-contract=off), so the results are those of numpy's.
#pragma once

#include <math.h>
#include <stdint.h>

#include "stac_smooth.hpp"  // smooth_clamp, smooth_quat: the arithmetic of a bounded column and of a quaternion block is smoothing's

#if defined(__HIPCC__)
#define STAC_RESAMPLE_HD __host__ __device__ inline
#else
#define STAC_RESAMPLE_HD inline
#endif

namespace stac {

constexpr int kResampleMaxUp = 32;     // U at most
constexpr int kResampleMaxDown = 64;   // D at most
constexpr int kResampleMaxWin = 256;   // taps W = 2 H of a phase at most
constexpr int kResampleMaxQuat = kSmoothMaxQuat;
// Columns of a band at most: a workgroup stages a band of columns of its rows, not whole rows, so that the tile does not depend
// on C.  The image of a band carries kResampleOverhang more columns (as far as the row has them): a quaternion block belongs to the
// band of its first column and finds its other three there.
constexpr int kResampleMaxBand = 64;
constexpr int kResampleOverhang = 3;
// LDS of a workgroup in floats (80 KiB): the phase rows of the tile, two bounds per column of the band and the staged rows.  Two
// workgroups fit the 160 KiB of a compute unit.  One output of the widest window (256 rows of 67 floats) takes 17 536 of them.
constexpr int kResampleLdsFloats = 20480;
constexpr int kResampleMaxTile = 128;  // outputs of a tile at most

// Output rows of a clip of L >= 1 input rows: the outputs m with m D / U <= L - 1, none beyond the last sample.
STAC_RESAMPLE_HD int64_t resample_rows(int64_t L, int32_t U, int32_t D) { return ((L - 1) * U) / D + 1; }

// Output m sits at input position m D / U = n + r / U
STAC_RESAMPLE_HD void resample_index(int64_t m, int32_t U, int32_t D, int64_t *n, int32_t *r) {
    const int64_t p = m * D;
    *n = p / U;
    *r = (int32_t)(p - *n * U);
}

// The nearest input row of output m (a tie goes down), inside the clip: what a per-frame mark of the output is gathered from.
STAC_RESAMPLE_HD int64_t resample_source_row(int64_t m, int64_t L, int32_t U, int32_t D) {
    int64_t n;
    int32_t r;
    resample_index(m, U, D, &n, &r);
    const int64_t s = n + (2 * r > U ? 1 : 0);
    return s > L - 1 ? L - 1 : s;
}

// Taps on each side of an output: tap j of a phase row belongs to input row n + (j - H + 1), j = 0 .. 2 H - 1
STAC_RESAMPLE_HD int32_t resample_half_rows(int32_t half, int32_t U) { return half / U + 1; }

// Columns of a band for rows of C floats: the row in the fewest bands of at most kResampleMaxBand, all but the last equally wide.
STAC_RESAMPLE_HD int32_t resample_band_cols(int32_t C) {
    const int32_t nb = (C + kResampleMaxBand - 1) / kResampleMaxBand;
    return (C + nb - 1) / nb;
}

// Input rows that T consecutive outputs reach at most, the clamped halo included: n of the last less n of the first, and a window.
STAC_RESAMPLE_HD int32_t resample_staged_rows(int32_t T, int32_t U, int32_t D, int32_t H) { return ((T - 1) * D + U - 1) / U + 2 * H; }

// LDS floats of a tile of T outputs of a band of bw columns: min(T, U) phase rows, the bounds, the image.
STAC_RESAMPLE_HD int32_t resample_lds_floats(int32_t T, int32_t bw, int32_t U, int32_t D, int32_t H) {
    return (T < U ? T : U) * 2 * H + 2 * bw + resample_staged_rows(T, U, D, H) * (bw + kResampleOverhang);
}

// Outputs T of a tile: as many as the LDS holds, kResampleMaxTile at most, and from U on a multiple of U (every tile of a clip then
// starts at phase 0 and the phase rows are staged once per workgroup).  At least 1 for every bw <= 64 and H <= 128.
STAC_RESAMPLE_HD int32_t resample_tile_rows(int32_t bw, int32_t U, int32_t D, int32_t H) {
    int32_t T = kResampleMaxTile;
    while (T > 1 && resample_lds_floats(T, bw, U, D, H) > kResampleLdsFloats) --T;
    return T >= U ? T - T % U : T;
}

// A scalar column: taps[0] * x[0], then + taps[j] * x[j * stride] for j = 1 .. W - 1, one rounding per operation (the arithmetic of
// smooth_scalar, for an even W: four taps at a time so that the reads of a step are in flight together, then the rest one by one).
STAC_RESAMPLE_HD float resample_scalar(const float *taps, const float *x, int32_t stride, int32_t W) {
    float acc = taps[0] * x[0];
    int32_t j = 1;
    for (; j + 3 < W; j += 4) {
        const float *y = x + j * stride;
        const float t0 = taps[j], t1 = taps[j + 1], t2 = taps[j + 2], t3 = taps[j + 3];
        const float x0 = y[0], x1 = y[stride], x2 = y[2 * stride], x3 = y[3 * stride];
        acc = acc + t0 * x0;
        acc = acc + t1 * x1;
        acc = acc + t2 * x2;
        acc = acc + t3 * x3;
    }
    for (; j < W; ++j) acc = acc + taps[j] * x[j * stride];
    return acc;
}

}  // namespace stac
