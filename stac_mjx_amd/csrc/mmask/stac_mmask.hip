// The offset phase on observed keypoints only (rule: stac_mmask.hpp; entry points: below the kernels; C ABI: stac_mmask.h).
//
// Three kernels, the shapes of the offset phase of stac_kernels.hip, whose serial sums they keep on purpose (the bits of a sum are
// its order; the phase is a fraction of a percent of a fit):
//   mmask_contrib_kernel  one lane per frame: the frame's row of the workspace, r of every keypoint and the subtotal of e in the
//                         order of k (mmask_frame); an entry that is not observed is three +0 and adds +0, its kp is not read
//   mmask_reduce_kernel   one thread per word of partial: the sum of its column over the frames in ascending order; the counts
//                         come from valid itself
//   mmask_finish_kernel   one thread: the closed form (mmask_finish)
// Offsets are 64-bit element offsets.  Nothing returns to the host, no workgroup waits for another, no atomics.
#include <hip/hip_runtime.h>

#include <string>

#include "stac_mmask.h"
#include "stac_mmask.hpp"

using namespace stac;

namespace {

constexpr int kMmaskContribThreads = 64;
constexpr int kMmaskReduceThreads = 128;

__global__ __launch_bounds__(kMmaskContribThreads) void mmask_contrib_kernel(const float *__restrict__ kp, const float *__restrict__ xpos,
                                                                             const float *__restrict__ xquat, int32_t nbody,
                                                                             const int32_t *__restrict__ site_bodyid,
                                                                             const uint8_t *__restrict__ valid, int64_t T, int32_t K,
                                                                             float *__restrict__ contrib) {
    const int64_t t = (int64_t)blockIdx.x * kMmaskContribThreads + threadIdx.x;
    if (t >= T) return;
    mmask_frame(kp, xpos, xquat, nbody, site_bodyid, valid, t, K, contrib + t * mmask_row_words(K));
}

__global__ __launch_bounds__(kMmaskReduceThreads) void mmask_reduce_kernel(const float *__restrict__ contrib, const uint8_t *__restrict__ valid,
                                                                           const int32_t *__restrict__ site_bodyid, int32_t nbody, int64_t T,
                                                                           int32_t K, float *__restrict__ partial) {
    const int32_t c = blockIdx.x * kMmaskReduceThreads + threadIdx.x;
    const int64_t W = mmask_row_words(K);
    if (c < 3 * K || c == 4 * K) {
        const float *col = contrib + (c == 4 * K ? 3 * K : c);
        float s = 0.0f;
#pragma unroll 8
        for (int64_t t = 0; t < T; ++t) s += col[t * W];
        partial[c] = s;
    } else if (c < 4 * K) {
        const int32_t k = c - 3 * K, b = site_bodyid[k];
        float n = 0.0f;
#pragma unroll 8
        for (int64_t t = 0; t < T; ++t) n += mmask_observed(valid[t * K + k], b, nbody) ? 1.0f : 0.0f;
        partial[c] = n;
    } else if (c == 4 * K + 1) {
        partial[c] = (float)T;
    }
}

__global__ void mmask_finish_kernel(const float *__restrict__ partial, int32_t K, const float *__restrict__ m0, const float *__restrict__ dreg,
                                    float lam, float *__restrict__ offsets, float *__restrict__ err, int32_t *__restrict__ n_out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    mmask_finish(partial, K, m0, dreg, lam, offsets, err, n_out);
}

// ---- error state of the calling thread (this library's own: it does not link against libstac_hip.so) ------------------------------
thread_local std::string g_err;
thread_local int32_t g_err_code = 0;
int fail(int code, const std::string &msg) {
    g_err = msg;
    g_err_code = code;
    return code;
}

struct Buf { const char *name; uintptr_t lo; int64_t bytes; int align; bool required; };

// Null, then alignment, then overlap, one text each; a buffer of 0 bytes is not looked at
int check_buffers(const char *who, const Buf *buf, int n) {
    for (int i = 0; i < n; ++i)
        if (buf[i].bytes && buf[i].required && !buf[i].lo) return fail(STAC_ERR_INVALID, std::string(who) + ": null " + buf[i].name);
    for (int i = 0; i < n; ++i)
        if (buf[i].bytes && buf[i].lo % buf[i].align != 0)
            return fail(STAC_ERR_INVALID, std::string(who) + ": " + buf[i].name + " must be " + std::to_string(buf[i].align) + "-byte aligned");
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (buf[i].bytes && buf[j].bytes && buf[i].lo && buf[j].lo && buf[i].lo < buf[j].lo + (uintptr_t)buf[j].bytes &&
                buf[j].lo < buf[i].lo + (uintptr_t)buf[i].bytes)
                return fail(STAC_ERR_INVALID, std::string(who) + ": " + buf[i].name + " and " + buf[j].name +
                                                  " overlap: inputs, outputs and workspace are distinct buffers");
    return STAC_OK;
}

int check_kp(const char *who, int32_t n_kp) {
    if (n_kp < 1) return fail(STAC_ERR_INVALID, std::string(who) + ": n_kp >= 1, got " + std::to_string(n_kp));
    if (n_kp > kMmaskMaxKp)
        return fail(STAC_ERR_CAPACITY, std::string(who) + ": n_kp = " + std::to_string(n_kp) + " exceeds the " + std::to_string(kMmaskMaxKp) + " keypoints of a call");
    return STAC_OK;
}

int64_t mmask_bytes(const char *who, int64_t n_frames, int32_t n_kp) {
    if (n_frames < 0 || n_frames > kMmaskMaxFrames)
        return fail(STAC_ERR_INVALID, std::string(who) + ": n_frames = " + std::to_string(n_frames) + " is outside 0 .. 2^24 (the observed counts are exact floats)");
    if (const int rc = check_kp(who, n_kp)) return rc;
    return mmask_workspace_bytes(n_frames, n_kp);
}

}  // namespace

// ---- C ABI entry points (stac_mmask.h): every argument is checked before the device is touched -----------------------------------
extern "C" const char *stac_mmask_last_error(void) { return g_err.c_str(); }
extern "C" int32_t stac_mmask_last_error_code(void) { return g_err_code; }

extern "C" int64_t stac_mmask_workspace(int64_t n_frames, int32_t n_kp) {
    const int64_t need = mmask_bytes("stac_mmask_workspace", n_frames, n_kp);
    if (need >= 0) fail(STAC_OK, "");
    return need;
}

extern "C" int32_t stac_mmask_partial(const float *kp, const float *xpos, const float *xquat, int32_t nbody, const int32_t *site_bodyid,
                                      const uint8_t *valid, int64_t n_frames, int32_t n_kp, void *workspace, int64_t workspace_bytes,
                                      float *partial, void *stream) {
    const char *who = "stac_mmask_partial";
    const int64_t need = mmask_bytes(who, n_frames, n_kp);
    if (need < 0) return (int32_t)need;
    if (nbody < 1 || nbody > kMmaskMaxBodies)
        return fail(STAC_ERR_INVALID, std::string(who) + ": nbody = " + std::to_string(nbody) + " is outside 1 .. " + std::to_string(kMmaskMaxBodies));
    if (workspace_bytes < need)
        return fail(STAC_ERR_INVALID, std::string(who) + ": workspace_bytes = " + std::to_string(workspace_bytes) + ", " + std::to_string(need) +
                                          " are needed (stac_mmask_workspace)");
    const int64_t T = n_frames, K = n_kp;
    const Buf buf[7] = {{"kp", (uintptr_t)kp, T * K * 12, 4, true},
                        {"xpos", (uintptr_t)xpos, T * nbody * 12, 4, true},
                        {"xquat", (uintptr_t)xquat, T * nbody * 16, 4, true},
                        {"site_bodyid", (uintptr_t)site_bodyid, K * 4, 4, true},
                        {"valid", (uintptr_t)valid, T * K, 1, true},
                        {"workspace", (uintptr_t)workspace, need, 4, true},
                        {"partial", (uintptr_t)partial, mmask_partial_words(K) * 4, 4, true}};
    if (const int rc = check_buffers(who, buf, 7)) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *contrib = (float *)workspace;
    if (T > 0) {  // (a zero-block grid would be an invalid launch; the sums below then come out as zeros)
        hipLaunchKernelGGL(mmask_contrib_kernel, dim3((unsigned)((T + kMmaskContribThreads - 1) / kMmaskContribThreads)), dim3(kMmaskContribThreads), 0, s,
                           kp, xpos, xquat, nbody, site_bodyid, valid, T, n_kp, contrib);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(STAC_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    const unsigned words = (unsigned)mmask_partial_words(K);
    hipLaunchKernelGGL(mmask_reduce_kernel, dim3((words + kMmaskReduceThreads - 1) / kMmaskReduceThreads), dim3(kMmaskReduceThreads), 0, s, contrib,
                       valid, site_bodyid, nbody, T, n_kp, partial);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(STAC_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return fail(STAC_OK, "");
}

extern "C" int32_t stac_mmask_finish(const float *partial, int32_t n_kp, const float *m0, const float *dreg, float lam, float *offsets_out,
                                     float *err_out, int32_t *n_out, void *stream) {
    const char *who = "stac_mmask_finish";
    if (const int rc = check_kp(who, n_kp)) return rc;
    const int64_t K = n_kp;
    const Buf buf[6] = {{"partial", (uintptr_t)partial, mmask_partial_words(K) * 4, 4, true}, {"m0", (uintptr_t)m0, K * 12, 4, true},
                        {"dreg", (uintptr_t)dreg, K * 12, 4, true},                           {"offsets_out", (uintptr_t)offsets_out, K * 12, 4, true},
                        {"err_out", (uintptr_t)err_out, 4, 4, false},                         {"n_out", (uintptr_t)n_out, K * 4, 4, false}};
    if (const int rc = check_buffers(who, buf, 6)) return rc;
    // (m0 and dreg are only read, but the offsets are written while they are: nothing may share memory with an output)
    hipLaunchKernelGGL(mmask_finish_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, partial, n_kp, m0, dreg, lam, offsets_out, err_out, n_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(STAC_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return fail(STAC_OK, "");
}
