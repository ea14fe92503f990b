// Pose steps of a fitted series (rule: stac_seam.hpp; entry point: below the kernel; C ABI: stac_seam.h).
//
// One kernel, one wavefront per workgroup, kSeamRowsPerGroup consecutive rows per workgroup:
//   seam_steps_kernel   lane l owns the columns j = l, l + 64, ... of every row of its workgroup.  Three LDS words per column -- its
//                       kind and its two running maxima (within clips, across a border) -- are read and written by the owning lane
//                       alone, so nothing in the kernel needs a barrier.  Per row the lanes take the measure of their columns
//                       (row t - 1 was row t of the iteration before: it comes out of the cache), then the wavefront reduces
//                       (largest scalar step, smallest column among equals), the largest r and the two not-finite flags with
//                       __shfl_xor, and lane 0 writes the row's four words.  After its rows a lane merges its column maxima into
//                       col_max_in / col_max_seam with an integer atomic maximum on the bit pattern, and only where its maximum
//                       exceeds what a plain read of the word shows: the maxima saturate after a few workgroups.
// Offsets are 64-bit element offsets.  Nothing returns to the host, no workgroup waits for another, no scratch.
#include <hip/hip_runtime.h>

#include <string>

#include "stac_seam.h"
#include "stac_seam.hpp"

using namespace stac;

namespace {

constexpr int kSeamThreads = 64;

struct SeamQuatCols { int32_t c[kSeamMaxQuat]; };

__device__ inline void seam_merge(uint32_t *dst, float v) {
    const uint32_t bits = seam_bits(v);  // (v >= +0 and finite: the order of the bits is the order of the floats)
    if (bits > __atomic_load_n(dst, __ATOMIC_RELAXED)) atomicMax(dst, bits);
}

__global__ __launch_bounds__(kSeamThreads) void seam_steps_kernel(const float *__restrict__ qpos, int64_t N, int32_t nq, int64_t clip_len,
                                                                  SeamQuatCols quat, int32_t n_quat, int32_t n_lin,
                                                                  float *__restrict__ step_joint, int32_t *__restrict__ step_col,
                                                                  float *__restrict__ step_rot, float *__restrict__ step_lin2,
                                                                  uint32_t *__restrict__ col_max_in, uint32_t *__restrict__ col_max_seam) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int32_t *kind = (int32_t *)smem;          // [nq]
    float *max_in = (float *)smem + nq;       // [nq]
    float *max_seam = (float *)smem + 2 * nq;  // [nq]
    const int lane = threadIdx.x;
    for (int32_t j = lane; j < nq; j += kSeamThreads) {
        kind[j] = seam_kind(j, quat.c, n_quat, n_lin);
        max_in[j] = 0.0f;
        max_seam[j] = 0.0f;
    }
    const int64_t t0 = (int64_t)blockIdx.x * kSeamRowsPerGroup;
    const int64_t t1 = t0 + kSeamRowsPerGroup < N ? t0 + kSeamRowsPerGroup : N;
    for (int64_t t = t0; t < t1; ++t) {
        if (t == 0) {
            if (lane == 0) {
                step_joint[0] = 0.0f;
                step_col[0] = -1;
                step_rot[0] = 0.0f;
                step_lin2[0] = 0.0f;
            }
            continue;
        }
        const float *a = qpos + (t - 1) * nq, *b = qpos + t * nq;
        float *col_max = t % clip_len == 0 ? max_seam : max_in;
        float best = -1.0f, rot = -__builtin_huge_valf();
        int32_t col = INT32_MAX;
        int bad = 0, rbad = 0;
        for (int32_t j = lane; j < nq; j += kSeamThreads) {
            const int32_t k = kind[j];
            if (k == kSeamQuatRest) continue;
            const float m = k == kSeamQuatFirst ? seam_rot(a, b, j) : seam_diff(a, b, j);
            const bool fin = seam_finite(m);
            if (k == kSeamScalar) {
                bad |= !fin;
                if (fin && m > best) best = m, col = j;  // (a lane's columns ascend: the first of equals stays)
            } else if (k == kSeamQuatFirst) {
                rbad |= !fin;
                if (fin && m > rot) rot = m;
            }
            if (fin && m > col_max[j]) col_max[j] = m;
        }
#pragma unroll
        for (int s = 1; s < kSeamThreads; s <<= 1) {
            const float ob = __shfl_xor(best, s, kSeamThreads), orot = __shfl_xor(rot, s, kSeamThreads);
            const int32_t oc = __shfl_xor(col, s, kSeamThreads);
            if (ob > best || (ob == best && oc < col)) best = ob, col = oc;
            if (orot > rot) rot = orot;
        }
        const bool any_bad = __any(bad), any_rbad = __any(rbad);
        if (lane == 0) {
            const bool none = col == INT32_MAX;
            step_joint[t] = any_bad ? seam_quiet_nan() : (none ? 0.0f : best);
            step_col[t] = any_bad || none ? -1 : col;
            step_rot[t] = any_rbad ? seam_quiet_nan() : (n_quat > 0 ? rot : 0.0f);
            step_lin2[t] = seam_lin2(a, b, n_lin);
        }
    }
    for (int32_t j = lane; j < nq; j += kSeamThreads) {
        if (max_in[j] > 0.0f) seam_merge(col_max_in + j, max_in[j]);
        if (max_seam[j] > 0.0f) seam_merge(col_max_seam + j, max_seam[j]);
    }
}

// ---- error state of the calling thread (this library's own: it does not link against libstac_hip.so) ------------------------------
thread_local std::string g_err;
thread_local int32_t g_err_code = 0;
int fail(int code, const std::string &msg) {
    g_err = msg;
    g_err_code = code;
    return code;
}

struct Buf { const char *name; uintptr_t lo; int64_t bytes; };

// Null, then alignment, then overlap, one text each
int check_buffers(const char *who, const Buf *buf, int n) {
    for (int i = 0; i < n; ++i)
        if (!buf[i].lo) return fail(STAC_ERR_INVALID, std::string(who) + ": null " + buf[i].name);
    for (int i = 0; i < n; ++i)
        if (buf[i].lo % 4 != 0) return fail(STAC_ERR_INVALID, std::string(who) + ": " + buf[i].name + " must be 4-byte aligned");
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (buf[i].lo < buf[j].lo + (uintptr_t)buf[j].bytes && buf[j].lo < buf[i].lo + (uintptr_t)buf[i].bytes)
                return fail(STAC_ERR_INVALID, std::string(who) + ": " + buf[i].name + " and " + buf[j].name +
                                                  " overlap: the input and the six outputs are distinct buffers");
    return STAC_OK;
}

}  // namespace

// ---- C ABI entry points (stac_seam.h): every argument is checked before the device is touched -------------------------------------
extern "C" const char *stac_seam_last_error(void) { return g_err.c_str(); }
extern "C" int32_t stac_seam_last_error_code(void) { return g_err_code; }

extern "C" int32_t stac_seam_steps(const float *qpos, int64_t n_rows, int32_t nq, int64_t clip_len, const int32_t *quat_cols, int32_t n_quat,
                                   int32_t n_lin, float *step_joint, int32_t *step_col, float *step_rot, float *step_lin2, float *col_max_in,
                                   float *col_max_seam, void *stream) {
    const std::string who = "stac_seam_steps";
    if (n_rows < 1 || n_rows > kSeamMaxRows)
        return fail(STAC_ERR_INVALID, who + ": n_rows = " + std::to_string(n_rows) + " is outside 1 .. 2^32");
    if (nq < 1) return fail(STAC_ERR_INVALID, who + ": nq >= 1, got " + std::to_string(nq));
    if (nq > kSeamMaxNq)
        return fail(STAC_ERR_CAPACITY, who + ": nq = " + std::to_string(nq) + " exceeds the " + std::to_string(kSeamMaxNq) + " columns of a call");
    if (clip_len < 1) return fail(STAC_ERR_INVALID, who + ": clip_len >= 1, got " + std::to_string(clip_len));
    if (n_rows % clip_len != 0)
        return fail(STAC_ERR_INVALID, who + ": " + std::to_string(n_rows) + " rows are not whole clips of clip_len = " + std::to_string(clip_len));
    if (n_quat < 0 || n_quat > kSeamMaxQuat)
        return fail(STAC_ERR_INVALID, who + ": n_quat = " + std::to_string(n_quat) + " is outside 0 .. " + std::to_string(kSeamMaxQuat));
    if (n_quat > 0 && !quat_cols) return fail(STAC_ERR_INVALID, who + ": null quat_cols (host memory) with n_quat = " + std::to_string(n_quat));
    switch (seam_check_layout(nq, quat_cols, n_quat, n_lin)) {
        case 0: break;
        case 3: return fail(STAC_ERR_INVALID, who + ": n_lin = " + std::to_string(n_lin) + " must be 0 or 3 and at most nq = " + std::to_string(nq));
        case 4: return fail(STAC_ERR_INVALID, who + ": a quaternion block lies outside the columns n_lin .. nq - 1 of a row");
        case 5: return fail(STAC_ERR_INVALID, who + ": two quaternion blocks overlap");
        default: return fail(STAC_ERR_INVALID, who + ": bad row layout");
    }
    const Buf buf[7] = {{"qpos", (uintptr_t)qpos, n_rows * nq * 4},         {"step_joint", (uintptr_t)step_joint, n_rows * 4},
                        {"step_col", (uintptr_t)step_col, n_rows * 4},       {"step_rot", (uintptr_t)step_rot, n_rows * 4},
                        {"step_lin2", (uintptr_t)step_lin2, n_rows * 4},     {"col_max_in", (uintptr_t)col_max_in, (int64_t)nq * 4},
                        {"col_max_seam", (uintptr_t)col_max_seam, (int64_t)nq * 4}};
    if (const int rc = check_buffers(who.c_str(), buf, 7)) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(col_max_in, 0, (size_t)nq * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(col_max_seam, 0, (size_t)nq * 4, s);
    if (e != hipSuccess) return fail(STAC_ERR_HIP, who + ": " + hipGetErrorString(e));
    SeamQuatCols quat = {};
    for (int32_t b = 0; b < n_quat; ++b) quat.c[b] = quat_cols[b];
    const unsigned groups = (unsigned)((n_rows + kSeamRowsPerGroup - 1) / kSeamRowsPerGroup);
    hipLaunchKernelGGL(seam_steps_kernel, dim3(groups), dim3(kSeamThreads), (size_t)nq * 12, s, qpos, n_rows, nq, clip_len, quat, n_quat, n_lin,
                       step_joint, step_col, step_rot, step_lin2, (uint32_t *)col_max_in, (uint32_t *)col_max_seam);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(STAC_ERR_HIP, who + ": " + hipGetErrorString(e));
    return fail(STAC_OK, "");
}
