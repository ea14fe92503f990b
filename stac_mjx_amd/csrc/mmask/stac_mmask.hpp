// The offset phase on observed keypoints only (stac_mmask.hip).  DESIGN.md "Offsets from observed keypoints".
//
// The closed form of the offset phase (csrc/stac_kernels.hip, "offset phase") fits every keypoint value it is given.  Here a mask
// valid [T][K] (uint8, non-zero = observed) says which values are observations, and a value that is none takes no part:
//   contribution of (t, k)   b = site_bodyid[k]; z = kp[t][k] - xpos[t][b]; r = R(xquat[t][b])^T z; e = |z|^2 -- the float32
//                            operations of m_contrib_kernel in its order (mmask_contrib).  Where (t, k) is not OBSERVED -- valid[t][k]
//                            is 0, or b is outside 0 .. nbody - 1 -- r = (+0, +0, +0) and e = +0 by a select: the three floats of that
//                            keypoint are never read into arithmetic, a NaN or an infinity there reaches no output
//   partial [4 K + 2]        s [K][3]: the sum of r over t ascending from +0;  n [K]: the observed count, as float (T <= 2^24, so
//                            it is exact);  z2: per frame the subtotal of e over k ascending from +0, the subtotals summed over t
//                            ascending from +0;  T.  Every word is additive across shards of the frames.
//   finish                   per coordinate i of keypoint k (d = dreg[3 k + i], m0 = m0[3 k + i], s = s[k][i]):
//                            denom = n_k + lam * d; numer = s + lam * d * m0; v = denom == 0 ? m0 : numer / denom;
//                            err = ((z2 - 2 * sum v s) + sum n_k * (v * v)) + lam * sum (d (v - m0))^2, the three sums over 3 k + i
//                            ascending from +0.  Outputs: offsets [K][3], err, n [K] as int32.
// Everything is float32 with one rounding per operation (-ffp-contract=off).  A sum that starts at +0 is never -0, so adding the +0
// of a masked entry changes no sum: with every entry observed s, z2, T and the offsets are the bits of stac_m_phase_partial /
// stac_m_phase_finish; err may differ by the rounding of its n (v v) term (there: T * sum v v).
//
// What the kernels and the CPU build of tests/mmask_cases.py share is below; mmask_reference / mmask_finish are the rule on the host.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define STAC_MMASK_HD __host__ __device__ inline
#else
#define STAC_MMASK_HD inline
#endif

namespace stac {

constexpr int64_t kMmaskMaxFrames = 1ll << 24;  // n_k is exact as a float
constexpr int32_t kMmaskMaxKp = 4096;           // keypoints of one call at most (the finish is one serial pass over 3 K words)
constexpr int32_t kMmaskMaxBodies = 1 << 16;    // bodies of a model at most

STAC_MMASK_HD int64_t mmask_partial_words(int64_t K) { return 4 * K + 2; }
STAC_MMASK_HD int64_t mmask_row_words(int64_t K) { return 3 * K + 1; }  // a frame's row of the workspace: r of every keypoint, then the subtotal of e
// Bytes of the workspace of T frames (a multiple of 8, at least 8: an empty series still hands a buffer over)
STAC_MMASK_HD int64_t mmask_workspace_bytes(int64_t T, int64_t K) { return T > 0 ? (4 * T * mmask_row_words(K) + 7) / 8 * 8 : 8; }

STAC_MMASK_HD bool mmask_observed(uint8_t valid, int32_t body, int32_t nbody) { return valid != 0 && body >= 0 && body < nbody; }

// r[3] = R(q)^T (y - p) and e = |y - p|^2: the operations of m_contrib_kernel, in its order
STAC_MMASK_HD void mmask_contrib(const float *q, const float *p, const float *y, float *r, float *e) {
    const float q00 = q[0] * q[0], q11 = q[1] * q[1], q22 = q[2] * q[2], q33 = q[3] * q[3];
    const float q01 = q[0] * q[1], q02 = q[0] * q[2], q03 = q[0] * q[3];
    const float q12 = q[1] * q[2], q13 = q[1] * q[3], q23 = q[2] * q[3];
    const float m0 = q00 + q11 - q22 - q33, m1 = 2.0f * (q12 - q03), m2 = 2.0f * (q13 + q02);
    const float m3 = 2.0f * (q12 + q03), m4 = q00 - q11 + q22 - q33, m5 = 2.0f * (q23 - q01);
    const float m6 = 2.0f * (q13 - q02), m7 = 2.0f * (q23 + q01), m8 = q00 - q11 - q22 + q33;
    const float z0 = y[0] - p[0], z1 = y[1] - p[1], z2 = y[2] - p[2];
    r[0] = m0 * z0 + m3 * z1 + m6 * z2;
    r[1] = m1 * z0 + m4 * z1 + m7 * z2;
    r[2] = m2 * z0 + m5 * z1 + m8 * z2;
    *e = z0 * z0 + z1 * z1 + z2 * z2;
}

// The row of frame t: row[3 k + i] = r_i of keypoint k, row[3 K] = the subtotal of e in the order of k
STAC_MMASK_HD void mmask_frame(const float *kp, const float *xpos, const float *xquat, int32_t nbody, const int32_t *site_bodyid,
                               const uint8_t *valid, int64_t t, int32_t K, float *row) {
    float z2t = 0.0f;
    for (int32_t k = 0; k < K; ++k) {
        const int32_t b = site_bodyid[k];
        float r[3] = {0.0f, 0.0f, 0.0f}, e = 0.0f;
        if (mmask_observed(valid[t * K + k], b, nbody))
            mmask_contrib(xquat + (t * nbody + b) * 4, xpos + (t * nbody + b) * 3, kp + (t * K + k) * 3, r, &e);
        row[3 * k + 0] = r[0];
        row[3 * k + 1] = r[1];
        row[3 * k + 2] = r[2];
        z2t += e;
    }
    row[3 * K] = z2t;
}

// The closed form, one serial pass (the kernel runs it in one thread).  err and n_out may be null.
STAC_MMASK_HD void mmask_finish(const float *partial, int32_t K, const float *m0, const float *dreg, float lam, float *offsets, float *err,
                                int32_t *n_out) {
    const float *n = partial + 3 * K;
    const float z2 = partial[4 * K];
    float ms = 0.0f, mm = 0.0f, reg = 0.0f;
    for (int32_t k = 0; k < K; ++k) {
        const float nk = n[k];
        for (int32_t i = 3 * k; i < 3 * k + 3; ++i) {
            const float d = dreg[i], s = partial[i], m0i = m0[i];
            const float denom = nk + lam * d;
            const float numer = s + lam * d * m0i;
            // never observed and an unregularised coordinate: nothing determines it -- keep the previous offset
            const float v = denom == 0.0f ? m0i : numer / denom;
            offsets[i] = v;
            ms += v * s;
            mm += nk * (v * v);
            const float dr = d * (v - m0i);
            reg += dr * dr;
        }
        if (n_out) n_out[k] = (int32_t)nk;
    }
    if (err) *err = ((z2 - 2.0f * ms) + mm) + lam * reg;
}

// The rule on the host: partial [4 K + 2] of the T frames.  row [3 K + 1] is the caller's scratch (no allocation here).
inline void mmask_reference(const float *kp, const float *xpos, const float *xquat, int32_t nbody, const int32_t *site_bodyid,
                            const uint8_t *valid, int64_t T, int32_t K, float *row, float *partial) {
    for (int64_t c = 0; c < mmask_partial_words(K); ++c) partial[c] = 0.0f;
    for (int64_t t = 0; t < T; ++t) {  // (n is summed as the float it is stored as: exact up to 2^24)
        mmask_frame(kp, xpos, xquat, nbody, site_bodyid, valid, t, K, row);
        for (int32_t c = 0; c < 3 * K; ++c) partial[c] += row[c];
        for (int32_t k = 0; k < K; ++k) partial[3 * K + k] += mmask_observed(valid[t * K + k], site_bodyid[k], nbody) ? 1.0f : 0.0f;
        partial[4 * K] += row[3 * K];
    }
    partial[4 * K + 1] = (float)T;
}

}  // namespace stac
