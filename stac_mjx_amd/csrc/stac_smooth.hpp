// Smoothing of fitted poses along time (stac_smooth.hip): a table-driven low-pass filter of qpos[N, nq] per clip, with the
// quaternion blocks aligned to the centre frame, summed and renormalised and the scalar columns clamped to the joint bounds.
// DESIGN.md "Smoothing fitted poses".
//
// Everything here is the window rule, the per-element arithmetic and the tile choice of the kernel, as host + device inline
// functions: a CPU build of this header (tests/test_smooth_host.py) runs exactly what the kernel runs.  Every float32 operation
// is a single IEEE operation in a stated order (the library is built with -ffp-contract=off), so the results are those of numpy's.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define STAC_SMOOTH_HD __host__ __device__ inline
#else
#define STAC_SMOOTH_HD inline
#endif

namespace stac {

constexpr int kSmoothMaxHalf = 16;                        // half-width H; the window is W = 2 H + 1 <= 33 frames
constexpr int kSmoothMaxWin = 2 * kSmoothMaxHalf + 1;
// Quaternion blocks of a row at most (their start columns travel in the kernel's arguments).  The models of tests/golden/
// (rodent, mouse, fly, synth) have one each, the free joint's: jnt_type holds no ball joint in any of them.  64 leaves room for
// a body of ball joints.
constexpr int kSmoothMaxQuat = 64;
// LDS of a workgroup in floats (64 KiB): the tap table, two words per column and the staged rows.  Two workgroups fit the 160 KiB
// of a compute unit with room to spare.
constexpr int kSmoothLdsFloats = 16384;
constexpr int kSmoothMaxTile = 128;                       // frames of a tile at most

// Frames T of a tile for rows of nq floats and half-width H: as many as the LDS holds beside the halo of 2 H rows, 128 at most.
// 0: not even one frame fits (nq beyond 437 at H = 16, beyond 3 275 at H = 1): the entry point refuses.
STAC_SMOOTH_HD int32_t smooth_tile_frames(int32_t nq, int32_t H) {
    const int32_t W = 2 * H + 1;
    const int32_t rows = (kSmoothLdsFloats - W * W) / nq - 2;  // (- 2: the two bounds per column)
    const int32_t T = rows - 2 * H;
    return T < 1 ? 0 : (T > kSmoothMaxTile ? kSmoothMaxTile : T);
}

// First frame s of the window of frame t in a clip of L >= W frames: clamp(t - H, 0, L - W).  The frame stands at position
// p = t - s of its window: H in the interior, less at the head of the clip, more at its tail.
STAC_SMOOTH_HD int32_t smooth_window_start(int32_t t, int32_t L, int32_t H) {
    const int32_t s = t - H, last = L - (2 * H + 1);
    return s < 0 ? 0 : (s > last ? last : s);
}

// A scalar column: taps[0] * x[0], then + taps[j] * x[j * stride] for j = 1 .. W-1, one rounding per operation.
// taps: row p of the table; x: the column's value in the first row of the window; stride: floats between rows.  W is odd.
// The loop is written four taps at a time (and the W - 1 = 2 H taps behind the first leave a rest of two or none): the eight reads
// of a step do not depend on each other, so on the device they are in flight together instead of one LDS round trip per tap;
// the sums are the same operations in the same order.
STAC_SMOOTH_HD float smooth_scalar(const float *taps, const float *x, int32_t stride, int32_t W) {
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
    if (j < W) {
        const float *y = x + j * stride;
        const float t0 = taps[j], t1 = taps[j + 1];
        const float x0 = y[0], x1 = y[stride];
        acc = acc + t0 * x0;
        acc = acc + t1 * x1;
    }
    return acc;
}

// np.clip(x, lb, ub) with comparisons that keep a NaN (post_clip of stac_post.hpp with two bounds)
STAC_SMOOTH_HD float smooth_clamp(float x, float lb, float ub) { return x < lb ? lb : (x > ub ? ub : x); }

// A quaternion block: every frame of the window is brought into the hemisphere of the centre frame's block c (sign of the dot
// product, a zero or NaN dot product counts as +), weighted and summed per component like a scalar column, then divided by the
// float32 norm.  Where the norm is not > 0 (zero or NaN) the output is c as it came.
// x: component 0 of the block in the first row of the window; c: the block of the frame itself.
STAC_SMOOTH_HD void smooth_quat(const float *taps, const float *x, int32_t stride, int32_t W, const float *c, float out[4]) {
    const float c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    for (int32_t j = 0; j < W; ++j) {
        const float *y = x + (int64_t)j * stride;
        const float y0 = y[0], y1 = y[1], y2 = y[2], y3 = y[3];
        const float d = ((c0 * y0 + c1 * y1) + c2 * y2) + c3 * y3;
        const float sg = d < 0.0f ? -1.0f : 1.0f;
        const float w = taps[j];
        const float p0 = w * (sg * y0), p1 = w * (sg * y1), p2 = w * (sg * y2), p3 = w * (sg * y3);
        if (j == 0) {
            a0 = p0; a1 = p1; a2 = p2; a3 = p3;
        } else {
            a0 = a0 + p0; a1 = a1 + p1; a2 = a2 + p2; a3 = a3 + p3;
        }
    }
    const float n = sqrtf(((a0 * a0 + a1 * a1) + a2 * a2) + a3 * a3);
    if (n > 0.0f) {
        out[0] = a0 / n; out[1] = a1 / n; out[2] = a2 / n; out[3] = a3 / n;
    } else {
        out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
    }
}

}  // namespace stac
