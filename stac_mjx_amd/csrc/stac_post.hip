// Post-processing kernels of a continuous run: cross-fade stitch and qvel (arithmetic: stac_post.hpp; entry points: below the kernels).
//
// Both are streaming kernels with one wavefront per row: a row's source (clip, frame) is worked out once per row, the 64 lanes
// then walk the row's D (or nv) consecutive floats, so every load and store instruction of a wavefront covers 256 contiguous
// bytes.  Rows are 4-byte aligned only (D is odd for most arrays), hence dword accesses.  Offsets are 64-bit element offsets.
#include <hip/hip_runtime.h>

#include "stac_host.hpp"
#include "stac_post.hpp"

namespace stac {

namespace {

constexpr int kPostThreads = 256;                // 4 wavefronts = 4 rows per workgroup and sweep
constexpr int kPostWaves = kPostThreads / 64;
constexpr int kPostMaxBlocks = 2048;             // 256 CUs x 8 workgroups: the grid strides over the rows beyond that

__global__ __launch_bounds__(kPostThreads) void post_stitch_kernel(const float *__restrict__ src, float *__restrict__ dst, int64_t C,
                                                                   int32_t F, int32_t ov, int32_t D, int64_t R, PostMask M) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kPostWaves;
    const int64_t W = (int64_t)F + ov;  // rows of a clip window
    for (int64_t r = (int64_t)blockIdx.x * kPostWaves + (threadIdx.x >> 6); r < R; r += stride) {
        int64_t c;
        int32_t t;
        const bool fade = post_stitch_source(r, C, F, ov, &c, &t);
        const float *a = src + (c * W + t) * D;
        float *o = dst + r * D;
        if (fade) {
            const float *b = src + ((c + 1) * W + (t - F)) * D;
            const double m = M.m[t - F];
            for (int32_t j = lane; j < D; j += 64) o[j] = post_fade(a[j], b[j], m);
        } else {
            for (int32_t j = lane; j < D; j += 64) o[j] = a[j];
        }
    }
}

__global__ __launch_bounds__(kPostThreads) void post_qvel_kernel(const float *__restrict__ qpos, float *__restrict__ qvel, int64_t N,
                                                                 int32_t nq, int32_t F, int32_t freejoint, float dt, float max_qvel) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kPostWaves;
    const int32_t nv = nq - (freejoint ? 1 : 0);
    for (int64_t r = (int64_t)blockIdx.x * kPostWaves + (threadIdx.x >> 6); r < N; r += stride) {
        const float *q0 = qpos + r * nq;
        const float *q1 = qpos + post_qvel_next(r, F) * nq;
        float *o = qvel + r * nv;
        for (int32_t j = lane; j < nv; j += 64) o[j] = post_qvel_elem(q0, q1, j, freejoint, dt, max_qvel);
    }
}

unsigned post_grid(int64_t rows) {
    const int64_t b = (rows + kPostWaves - 1) / kPostWaves;
    return (unsigned)(b < kPostMaxBlocks ? b : kPostMaxBlocks);
}

}  // namespace

static hipError_t launch_post_stitch(const float *src, float *dst, int64_t C, int32_t F, int32_t ov, int32_t D, int64_t R, const PostMask &M,
                              hipStream_t s) {
    if (R <= 0) return hipSuccess;
    hipLaunchKernelGGL(post_stitch_kernel, dim3(post_grid(R)), dim3(kPostThreads), 0, s, src, dst, C, F, ov, D, R, M);
    return hipGetLastError();
}

static hipError_t launch_post_qvel(const float *qpos, float *qvel, int64_t N, int32_t nq, int32_t F, int32_t freejoint, float dt,
                            float max_qvel, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    hipLaunchKernelGGL(post_qvel_kernel, dim3(post_grid(N)), dim3(kPostThreads), 0, s, qpos, qvel, N, nq, F, freejoint, dt, max_qvel);
    return hipGetLastError();
}

}  // namespace stac

// ---- C ABI entry points (include/stac_hip.h): every argument is checked before the device is touched ------------------------------
extern "C" int64_t stac_post_stitch_rows(int64_t C, int32_t F, int32_t overlap) {
    const int64_t R = post_stitch_rows(C, F, overlap);
    if (R < 0) return fail(STAC_ERR_INVALID, "stac_post_stitch_rows: C >= 0, F >= 1, overlap 1..32");
    return R;
}

extern "C" int32_t stac_post_stitch(const float *src, int64_t C, int32_t F, int32_t overlap, int32_t D, const double *mask_host,
                                    float *dst, int64_t dst_rows, void *stream) {
    const int64_t R = post_stitch_rows(C, F, overlap);
    if (R < 0 || D < 1) return fail(STAC_ERR_INVALID, "stac_post_stitch: C >= 0, F >= 1, overlap 1..32, D >= 1");
    if (dst_rows != R)
        return fail(STAC_ERR_INVALID, "stac_post_stitch: dst_rows = " + std::to_string(dst_rows) + ", the stitched array has " +
                                          std::to_string(R) + " rows (stac_post_stitch_rows)");
    if (C == 0) return STAC_OK;
    if (!src || !dst || !mask_host) return fail(STAC_ERR_INVALID, "stac_post_stitch: null src / dst / mask_host");
    PostMask M{};
    for (int k = 0; k < overlap; ++k) M.m[k] = mask_host[k];
    return launch_result("stac_post_stitch", launch_post_stitch(src, dst, C, F, overlap, D, R, M, (hipStream_t)stream));
}

extern "C" int32_t stac_post_qvel(const float *qpos, int64_t N, int32_t nq, int32_t F, double dt, int32_t freejoint, double max_qvel,
                                  float *qvel, void *stream) {
    if (N < 0 || F < 1 || nq < 1 || (freejoint && nq < 7))
        return fail(STAC_ERR_INVALID, "stac_post_qvel: N >= 0, F >= 1, nq >= 1 (nq >= 7 with a free joint)");
    if (N % F != 0)
        return fail(STAC_ERR_INVALID, "stac_post_qvel: " + std::to_string(N) + " rows are not whole clips of " + std::to_string(F));
    if (dt == 0.0) return fail(STAC_ERR_INVALID, "stac_post_qvel: dt == 0");
    if (N == 0) return STAC_OK;
    if (!qpos || !qvel) return fail(STAC_ERR_INVALID, "stac_post_qvel: null qpos / qvel");
    return launch_result("stac_post_qvel", launch_post_qvel(qpos, qvel, N, nq, F, freejoint ? 1 : 0, (float)dt, (float)max_qvel, (hipStream_t)stream));
}
