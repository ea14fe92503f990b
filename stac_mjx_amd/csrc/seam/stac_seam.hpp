// Pose steps of a fitted series (stac_seam.hip).  DESIGN.md "Warm-started clips and pose steps".
//
// qpos [N][nq] holds the poses of N / clip_len clips of clip_len rows each.  A row's STEP is how far the pose moved since the row
// before it; a step across a clip border (t % clip_len == 0, t > 0) is a SEAM.  Every column j of a row is one of
//   translation   j < n_lin (n_lin is 0, or 3: the free joint's position)
//   block         c <= j < c + 4 for a quaternion block that starts at c = quat_cols[b]; j == c is the block's FIRST column
//   scalar        every other column (hinges and slides)
// and, with a = row t - 1 and b = row t (t > 0), its MEASURE is
//   scalar, translation   d_j = |b[j] - a[j]|
//   first of a block      r = 1 - |dot|, dot = ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3 over the block's four columns
//   rest of a block       +0
// Per row t > 0:
//   step_joint   the largest d_j over the scalar columns and step_col the smallest j that attains it; +0 and -1 without a scalar
//                column; the quiet NaN 0x7FC00000 and -1 if any scalar d_j is not finite
//   step_rot     the largest r over the blocks (it is negative where every |dot| exceeds 1), +0 without blocks, the quiet NaN if any
//                r is not finite.  No square root or arc cosine here: the host turns it into an angle (2 acos(1 - r))
//   step_lin2    (d0 * d0 + d1 * d1) + d2 * d2 over the translation columns, +0 without them, the quiet NaN if that is not finite
// Row 0 has no row before it: step_joint, step_rot and step_lin2 are +0 and step_col is -1.
// Per column j: col_max_in[j] is the maximum of the measure over the rows with t % clip_len != 0, col_max_seam[j] over the rows with
// t % clip_len == 0 and t > 0.  Both start from +0 and a measure that is not finite is skipped, so they are never negative and never
// NaN: a maximum has no order, its bits do not depend on how it is reduced, and the kernel may merge partial maxima with an integer
// atomic maximum on the bit pattern (the order of non-negative floats is the order of their bits).
// Everything is float32 with one rounding per operation (-ffp-contract=off).
//
// What the kernel and the CPU build of tests/seam_cases.py share is below; seam_reference is the rule on the host, serial.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define STAC_SEAM_HD __host__ __device__ inline
#else
#define STAC_SEAM_HD inline
#endif

namespace stac {

constexpr int32_t kSeamMaxQuat = 64;        // quaternion blocks of a row at most (they travel to the kernel by value)
constexpr int32_t kSeamMaxNq = 4096;        // columns of a row at most (a workgroup keeps three words per column in LDS)
constexpr int64_t kSeamMaxRows = 1ll << 32;  // rows at most (the grid is rows / kSeamRowsPerGroup workgroups of 64 threads, below 2^32 threads)
constexpr int32_t kSeamRowsPerGroup = 128;  // consecutive rows of one workgroup (one wavefront)

enum SeamKind : int32_t { kSeamScalar = 0, kSeamLin = 1, kSeamQuatFirst = 2, kSeamQuatRest = 3 };

STAC_SEAM_HD float seam_quiet_nan() {
    union { uint32_t u; float f; } v;
    v.u = 0x7FC00000u;
    return v.f;
}
STAC_SEAM_HD uint32_t seam_bits(float x) {
    union { uint32_t u; float f; } v;
    v.f = x;
    return v.u;
}
STAC_SEAM_HD float seam_abs(float x) {  // clears the sign bit: no arithmetic, the same bits on host and device
    union { uint32_t u; float f; } v;
    v.f = x;
    v.u &= 0x7FFFFFFFu;
    return v.f;
}
// Finite: neither an infinity nor a NaN, told from the exponent bits (no compiler may fold it away under any flag)
STAC_SEAM_HD bool seam_finite(float x) { return (seam_bits(x) & 0x7F800000u) != 0x7F800000u; }

STAC_SEAM_HD int32_t seam_kind(int32_t j, const int32_t *quat_cols, int32_t n_quat, int32_t n_lin) {
    if (j < n_lin) return kSeamLin;
    for (int32_t b = 0; b < n_quat; ++b) {
        if (j == quat_cols[b]) return kSeamQuatFirst;
        if (j > quat_cols[b] && j < quat_cols[b] + 4) return kSeamQuatRest;
    }
    return kSeamScalar;
}

STAC_SEAM_HD float seam_diff(const float *a, const float *b, int32_t j) { return seam_abs(b[j] - a[j]); }

// r of the block whose first column is c
STAC_SEAM_HD float seam_rot(const float *a, const float *b, int32_t c) {
    const float dot = ((a[c] * b[c] + a[c + 1] * b[c + 1]) + a[c + 2] * b[c + 2]) + a[c + 3] * b[c + 3];
    return 1.0f - seam_abs(dot);
}

// step_lin2 of a row (n_lin is 0 or 3)
STAC_SEAM_HD float seam_lin2(const float *a, const float *b, int32_t n_lin) {
    if (n_lin != 3) return 0.0f;
    const float d0 = seam_diff(a, b, 0), d1 = seam_diff(a, b, 1), d2 = seam_diff(a, b, 2);
    const float s = (d0 * d0 + d1 * d1) + d2 * d2;
    return seam_finite(s) ? s : seam_quiet_nan();
}

// The layout of a row: 0, or the number of the first rule it breaks (the entry point turns it into a text)
//   1 nq outside 1 .. kSeamMaxNq   2 n_quat outside 0 .. kSeamMaxQuat   3 n_lin not 0 or 3, or beyond nq
//   4 a block that is not inside n_lin .. nq   5 two blocks that overlap
inline int seam_check_layout(int32_t nq, const int32_t *quat_cols, int32_t n_quat, int32_t n_lin) {
    if (nq < 1 || nq > kSeamMaxNq) return 1;
    if (n_quat < 0 || n_quat > kSeamMaxQuat) return 2;
    if ((n_lin != 0 && n_lin != 3) || n_lin > nq) return 3;
    for (int32_t b = 0; b < n_quat; ++b)
        if (quat_cols[b] < n_lin || quat_cols[b] > nq - 4) return 4;
    for (int32_t b = 0; b < n_quat; ++b)
        for (int32_t c = b + 1; c < n_quat; ++c)
            if (quat_cols[b] - quat_cols[c] < 4 && quat_cols[c] - quat_cols[b] < 4) return 5;
    return 0;
}

// The rule on the host, one serial pass.  Every output is written.
inline void seam_reference(const float *qpos, int64_t N, int32_t nq, int64_t clip_len, const int32_t *quat_cols, int32_t n_quat,
                           int32_t n_lin, float *step_joint, int32_t *step_col, float *step_rot, float *step_lin2, float *col_max_in,
                           float *col_max_seam) {
    for (int32_t j = 0; j < nq; ++j) col_max_in[j] = col_max_seam[j] = 0.0f;
    for (int64_t t = 0; t < N; ++t) {
        if (t == 0) {
            step_joint[0] = step_rot[0] = step_lin2[0] = 0.0f;
            step_col[0] = -1;
            continue;
        }
        const float *a = qpos + (t - 1) * nq, *b = qpos + t * nq;
        float *col_max = t % clip_len == 0 ? col_max_seam : col_max_in;
        float best = 0.0f, rot = 0.0f;
        int32_t col = -1;
        bool bad = false, rbad = false, any_rot = false;
        for (int32_t j = 0; j < nq; ++j) {
            const int32_t kind = seam_kind(j, quat_cols, n_quat, n_lin);
            if (kind == kSeamQuatRest) continue;
            const float m = kind == kSeamQuatFirst ? seam_rot(a, b, j) : seam_diff(a, b, j);
            const bool fin = seam_finite(m);
            if (kind == kSeamScalar) {
                bad |= !fin;
                if (fin && (col < 0 || m > best)) best = m, col = j;
            } else if (kind == kSeamQuatFirst) {
                rbad |= !fin;
                if (fin && (!any_rot || m > rot)) rot = m, any_rot = true;
            }
            if (fin && m > col_max[j]) col_max[j] = m;
        }
        step_joint[t] = bad ? seam_quiet_nan() : best;
        step_col[t] = bad ? -1 : col;
        step_rot[t] = rbad ? seam_quiet_nan() : rot;
        step_lin2[t] = seam_lin2(a, b, n_lin);
    }
}

}  // namespace stac
