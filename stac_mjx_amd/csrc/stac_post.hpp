// Post-processing of a continuous ik_only run (stac_post.hip): the cross-fade stitch of overlapping clip windows
// (stac_mjx/utils.py:393-461) and the finite-difference qvel (utils.py:302-347).  DESIGN.md "Post-processing on the GPU".
//
// Everything here is the per-row / per-element arithmetic of the two kernels, as host + device inline functions: a CPU build
// of this header (tests/test_post_host.py) runs exactly what the kernels run.  Every float32 and float64 operation is a single
// IEEE operation in a stated order (the library is built with -ffp-contract=off), so the results are those of numpy's.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define STAC_POST_HD __host__ __device__ inline
#else
#define STAC_POST_HD inline
#endif

namespace stac {

constexpr int kPostMaxOverlap = 32;

// m[overlap] of the cross-fade, by value in the kernel's arguments (computed on the host with numpy's expression)
struct PostMask {
    double m[kPostMaxOverlap];
};

// Rows of the stitched array: clip 0 whole, clips 1 .. C-2 without their head, clip C-1 without head and tail (for C == 1
// that is clip 0 again: the reference's slicing).  -1: bad arguments.
STAC_POST_HD int64_t post_stitch_rows(int64_t C, int64_t F, int64_t ov) {
    if (C < 0 || F < 1 || ov < 1 || ov > kPostMaxOverlap) return -1;
    if (C == 0) return 0;
    return F + ov + (C > 2 ? C - 2 : 0) * F + (F > ov ? F - ov : 0);
}

// Output row r -> its source row (clip c, frame t).  Returns true when the row is a cross-fade of (c, t) with (c + 1, t - F).
// (The one 64-bit division per ROW; elements never divide.)
STAC_POST_HD bool post_stitch_source(int64_t r, int64_t C, int32_t F, int32_t ov, int64_t *c, int32_t *t) {
    const int64_t head = (int64_t)F + ov;
    int64_t cc = 0;
    int32_t tt = (int32_t)r;
    if (r >= head) {
        const int64_t k = (r - head) / F;
        cc = 1 + k;
        tt = ov + (int32_t)((r - head) - k * F);
        if (cc > C - 1) cc = C - 1;  // C == 1: the "last clip" is clip 0
    }
    *c = cc;
    *t = tt;
    return tt >= F && cc < C - 1;
}

// (1 - m) * a + m * b in double, two products and one sum, rounded once to float32
STAC_POST_HD float post_fade(float a, float b, double m) {
    const double pa = (1.0 - m) * (double)a;
    const double pb = m * (double)b;
    return (float)(pa + pb);
}

// np.clip(x, -m, m): a NaN stays a NaN
STAC_POST_HD float post_clip(float x, float m) { return x < -m ? -m : (x > m ? m : x); }

// Row that row r of qpos[N, nq] differences against: the next one, or itself on the last row of its clip of F rows
STAC_POST_HD int64_t post_qvel_next(int64_t r, int32_t F) { return (r % F == F - 1) ? r : r + 1; }

// Root gyro (before the division by dt): quat_to_axisangle(normalise(conj(q0) * q1)) of utils.py, operation by operation.
// q0, q1: the root quaternions w, x, y, z of the two rows.
STAC_POST_HD void post_gyro(const float *q0, const float *q1, float out[3]) {
    const float aw = q0[0], ax = -q0[1], ay = -q0[2], az = -q0[3];
    const float bw = q1[0], bx = q1[1], by = q1[2], bz = q1[3];
    // utils.quat_mul(a, b), its operand order
    const float w = aw * bw - ax * bx - ay * by - az * bz;
    const float x = aw * bx + ax * bw + ay * bz - az * by;
    const float y = aw * by - ax * bz + ay * bw + az * bx;
    const float z = aw * bz + ax * by - ay * bx + az * bw;
    // np.linalg.norm over four float32 values: squares summed left to right, one float32 square root
    const float n = sqrtf(w * w + x * x + y * y + z * z);
    const float nw = w / n, nx = x / n, ny = y / n, nz = z / n;
    const double wd = (double)nw;
    const double wc = wd < -1.0 ? -1.0 : (wd > 1.0 ? 1.0 : wd);
    const double angle = 2.0 * acos(wc);
    if (angle < 1e-10) {
        out[0] = out[1] = out[2] = 0.0f;
        return;
    }
    const double s = sin(angle / 2.0);  // the device library's double sin needs no scratch here
    const double pi = 3.141592653589793;
    const double wrapped = fmod(angle + pi, 2.0 * pi) - pi;
    out[0] = (float)((double)nx / s * wrapped);
    out[1] = (float)((double)ny / s * wrapped);
    out[2] = (float)((double)nz / s * wrapped);
}

// Element j of a qvel row from the qpos rows q0 (this frame) and q1 (post_qvel_next); nv = nq - 1 columns with a free joint
STAC_POST_HD float post_qvel_elem(const float *q0, const float *q1, int32_t j, int32_t freejoint, float dt, float max_qvel) {
    if (!freejoint) return post_clip((q1[j] - q0[j]) / dt, max_qvel);
    if (j < 3) return (q1[j] - q0[j]) / dt;
    if (j < 6) {
        float g[3];
        post_gyro(q0 + 3, q1 + 3, g);
        return (j == 3 ? g[0] : (j == 4 ? g[1] : g[2])) / dt;
    }
    return post_clip((q1[j + 1] - q0[j + 1]) / dt, max_qvel);
}

}  // namespace stac
