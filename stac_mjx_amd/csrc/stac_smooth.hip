// Smoothing fitted poses along time (rule and shared functions: stac_smooth.hpp; entry point: below the kernels).
//
// The job is bound by memory traffic: every output is a weighted sum of W = 2 H + 1 inputs of its column, so a kernel that reads
// them from global memory reads qpos W times.  A workgroup therefore works on one tile of T consecutive frames of one clip at a
// time (T: smooth_tile_frames, from nq and H; 512 threads) and strides over the tiles with at most kSmoothMaxBlocks workgroups:
//   1. the rows that the tile's clamped windows reach -- at most T + 2 H, contiguous in memory -- go to LDS as one dense image;
//      thread i stages floats i, i + 512, ..., so every load instruction of a wavefront covers 256 contiguous bytes (rows are
//      4-byte aligned only, hence dword accesses; 64-bit element offsets).  The tap table (W x W floats) and two words per column
//      (its bounds; a NaN lower bound marks a column of a quaternion block) stand in LDS as well, written once per workgroup;
//   2. scalar pass: thread i computes elements i, i + 512, ... of the tile's own rows in the order of memory (smooth_scalar over
//      the image, then the clamp), so the stores coalesce like the loads; the (frame, column) of an element is stepped, not
//      divided.  Lanes on a column of a quaternion block sit this pass out;
//   3. quaternion pass: thread i computes whole blocks i, i + 512, ... of the tile (frame-major), smooth_quat over the image, and
//      stores their four floats.  A pass of its own keeps the longer quaternion loop from stalling the wavefronts of pass 2.
// Taps and rows are read through LDS addresses; nothing is kept in a per-lane array with run-time indices (no scratch).
// The tap table is a host table of up to 4 356 bytes, more than kernel arguments carry: it is written to a stream-ordered device
// buffer by smooth_upload_kernel, whose arguments hold it in pieces (copied at launch, so the caller's table may go at once).
#include <hip/hip_runtime.h>

#include "stac_host.hpp"
#include "stac_smooth.hpp"

namespace stac {

namespace {

constexpr int kSmoothThreads = 512;  // 8 wavefronts: with two or three workgroups per compute unit (LDS) 16 .. 24 wavefronts hide the LDS latency
constexpr int kSmoothMaxBlocks = 1024;  // 256 CUs x 4 workgroups (LDS admits 2 .. 3 of them at a time): the grid strides over the tiles beyond that
constexpr int kSmoothChunk = 768;       // floats of the tap table per upload launch (3 KiB of kernel arguments)

struct SmoothChunk {
    float v[kSmoothChunk];
};

// start columns of the quaternion blocks, by value in the kernel's arguments
struct SmoothQuat {
    int32_t n;
    int32_t col[kSmoothMaxQuat];
};

__global__ __launch_bounds__(kSmoothThreads) void smooth_upload_kernel(float *__restrict__ dst, int32_t n, SmoothChunk c) {
    for (int32_t i = threadIdx.x; i < n; i += kSmoothThreads) dst[i] = c.v[i];
}

__global__ __launch_bounds__(kSmoothThreads) void smooth_kernel(const float *__restrict__ qpos, float *__restrict__ out,
                                                                const float *__restrict__ taps_dev, const float *__restrict__ lb,
                                                                const float *__restrict__ ub, int32_t nq, int32_t L, int32_t H, int32_t T,
                                                                int32_t tiles_per_clip, int64_t tiles, SmoothQuat Q) {
    extern __shared__ float smooth_lds[];
    const int32_t W = 2 * H + 1;
    float *taps = smooth_lds;                  // [W * W]
    float *lo_col = smooth_lds + W * W;        // [nq] lower bound of a scalar column (-inf without one); NaN: a quaternion column
    float *hi_col = lo_col + nq;               // [nq] upper bound (+inf without one)
    float *img = hi_col + nq;                  // [<= T + 2 H][nq]
    const int32_t tid = threadIdx.x;
    for (int32_t i = tid; i < W * W; i += kSmoothThreads) taps[i] = taps_dev[i];
    for (int32_t j = tid; j < nq; j += kSmoothThreads) {
        // a NaN bound clamps nothing (smooth_clamp compares), like an infinite one: the image keeps NaN for the quaternion columns
        const float lo = lb ? lb[j] : -INFINITY, hi = ub ? ub[j] : INFINITY;
        lo_col[j] = lo == lo ? lo : -INFINITY;
        hi_col[j] = hi == hi ? hi : INFINITY;
    }
    __syncthreads();
    for (int32_t b = tid; b < Q.n; b += kSmoothThreads) {
        const int32_t col = Q.col[b];
        lo_col[col] = lo_col[col + 1] = lo_col[col + 2] = lo_col[col + 3] = __builtin_nanf("");
    }
    // (the barrier behind the first tile's staging orders these writes before their reads)
    const int32_t df = kSmoothThreads / nq, dj = kSmoothThreads - df * nq;  // the (frame, column) step of 512 elements
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t c = tile / tiles_per_clip;
        const int32_t t0 = (int32_t)(tile - c * tiles_per_clip) * T;
        const int32_t nT = L - t0 < T ? L - t0 : T;
        // 1: the image, rows s_lo .. s_hi - 1 of the clip
        const int32_t s_lo = smooth_window_start(t0, L, H);
        const int32_t s_hi = smooth_window_start(t0 + nT - 1, L, H) + W;
        const float *src = qpos + (c * L + s_lo) * nq;
        const int32_t staged = (s_hi - s_lo) * nq;  // <= (T + 2 H) nq
        for (int32_t i = tid; i < staged; i += kSmoothThreads) img[i] = src[i];
        __syncthreads();
        // 2: the scalar columns of the tile's own rows
        float *dst = out + (c * L + t0) * nq;
        const int32_t own = nT * nq;
        int32_t f = tid / nq, j = tid - f * nq;
        for (int32_t e = tid; e < own; e += kSmoothThreads) {
            // (bounds from LDS: a global load in this loop would make every element wait for the store of the one before it,
            // loads and stores share a counter)
            const float lo = lo_col[j], hi = hi_col[j];
            if (lo == lo) {
                const int32_t t = t0 + f, s = smooth_window_start(t, L, H);
                const float v = smooth_scalar(taps + (t - s) * W, img + (s - s_lo) * nq + j, nq, W);
                dst[e] = smooth_clamp(v, lo, hi);
            }
            f += df;
            j += dj;
            if (j >= nq) {
                j -= nq;
                ++f;
            }
        }
        // 3: the quaternion blocks
        const int32_t blocks = nT * Q.n;
        for (int32_t e = tid; e < blocks; e += kSmoothThreads) {
            const int32_t fq = e / Q.n, col = Q.col[e - fq * Q.n];
            const int32_t t = t0 + fq, s = smooth_window_start(t, L, H);
            float o[4];
            smooth_quat(taps + (t - s) * W, img + (s - s_lo) * nq + col, nq, W, img + (t - s_lo) * nq + col, o);
            float *d = dst + fq * nq + col;
            d[0] = o[0];
            d[1] = o[1];
            d[2] = o[2];
            d[3] = o[3];
        }
        __syncthreads();  // img is written again in the next sweep
    }
}

}  // namespace

static hipError_t launch_post_smooth(const float *qpos, int64_t N, int32_t nq, int32_t L, int32_t H, const float *taps_host,
                                     const SmoothQuat &Q, const float *lb, const float *ub, float *out, hipStream_t s) {
    const int32_t W = 2 * H + 1, T = smooth_tile_frames(nq, H);
    const int32_t tiles_per_clip = (L + T - 1) / T;
    const int64_t tiles = (N / L) * tiles_per_clip;
    float *taps_dev = nullptr;
    hipError_t e = hipMallocAsync(reinterpret_cast<void **>(&taps_dev), (size_t)W * W * sizeof(float), s);
    if (e != hipSuccess) return e;
    for (int32_t at = 0; at < W * W && e == hipSuccess; at += kSmoothChunk) {
        SmoothChunk chunk;
        const int32_t n = W * W - at < kSmoothChunk ? W * W - at : kSmoothChunk;
        for (int32_t i = 0; i < kSmoothChunk; ++i) chunk.v[i] = i < n ? taps_host[at + i] : 0.0f;
        hipLaunchKernelGGL(smooth_upload_kernel, dim3(1), dim3(kSmoothThreads), 0, s, taps_dev + at, n, chunk);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        const size_t lds = (size_t)(W * W + 2 * nq + (T + 2 * H) * nq) * sizeof(float);  // <= kSmoothLdsFloats floats (smooth_tile_frames)
        const unsigned grid = (unsigned)(tiles < kSmoothMaxBlocks ? tiles : kSmoothMaxBlocks);
        hipLaunchKernelGGL(smooth_kernel, dim3(grid), dim3(kSmoothThreads), lds, s, qpos, out, taps_dev, lb, ub, nq, L, H, T, tiles_per_clip,
                           tiles, Q);
        e = hipGetLastError();
    }
    const hipError_t ef = hipFreeAsync(taps_dev, s);  // stream-ordered: behind the kernel that reads it
    return e != hipSuccess ? e : ef;
}

}  // namespace stac

// ---- C ABI entry point (include/stac_hip.h): every argument is checked before the device is touched -------------------------------
extern "C" int32_t stac_post_smooth(const float *qpos, int64_t N, int32_t nq, int32_t clip_len, int32_t half_window, const float *taps,
                                    const int32_t *quat_cols, int32_t n_quat, const float *lb, const float *ub, float *out, void *stream) {
    if (N < 0 || nq < 1 || N > (((int64_t)1 << 59) / nq))
        return fail(STAC_ERR_INVALID, "stac_post_smooth: N >= 0, nq >= 1 (and array sizes within int64)");
    if (half_window < 1 || half_window > kSmoothMaxHalf)
        return fail(STAC_ERR_INVALID, "stac_post_smooth: half_window " + std::to_string(half_window) + " is outside 1 .. " +
                                          std::to_string(kSmoothMaxHalf));
    const int32_t W = 2 * half_window + 1;
    if (clip_len < W)
        return fail(STAC_ERR_INVALID, "stac_post_smooth: clips of " + std::to_string(clip_len) + " frames are shorter than the window of " +
                                          std::to_string(W));
    if (N % clip_len != 0)
        return fail(STAC_ERR_INVALID, "stac_post_smooth: " + std::to_string(N) + " rows are not whole clips of " + std::to_string(clip_len));
    if (n_quat < 0 || n_quat > kSmoothMaxQuat)
        return fail(STAC_ERR_INVALID, "stac_post_smooth: " + std::to_string(n_quat) + " quaternion blocks, at most " +
                                          std::to_string(kSmoothMaxQuat) + " (kSmoothMaxQuat)");
    if (n_quat > 0 && !quat_cols) return fail(STAC_ERR_INVALID, "stac_post_smooth: null quat_cols");
    SmoothQuat Q{};
    Q.n = n_quat;
    for (int32_t b = 0; b < n_quat; ++b) {
        const int32_t col = quat_cols[b];
        if (col < 0 || col > nq - 4)
            return fail(STAC_ERR_INVALID, "stac_post_smooth: the quaternion block at column " + std::to_string(col) + " leaves the row of " +
                                              std::to_string(nq));
        for (int32_t a = 0; a < b; ++a)
            if (col - Q.col[a] < 4 && Q.col[a] - col < 4)
                return fail(STAC_ERR_INVALID, "stac_post_smooth: the quaternion blocks at columns " + std::to_string(Q.col[a]) + " and " +
                                                  std::to_string(col) + " overlap");
        Q.col[b] = col;
    }
    if (smooth_tile_frames(nq, half_window) < 1)
        return fail(STAC_ERR_INVALID, "stac_post_smooth: rows of " + std::to_string(nq) + " floats leave no room for a window of " +
                                          std::to_string(W) + " of them in a workgroup's LDS");
    if (!taps) return fail(STAC_ERR_INVALID, "stac_post_smooth: null taps");
    if ((lb == nullptr) != (ub == nullptr)) return fail(STAC_ERR_INVALID, "stac_post_smooth: lb and ub must be given together");
    if (N == 0) return STAC_OK;
    if (!qpos || !out) return fail(STAC_ERR_INVALID, "stac_post_smooth: null qpos / out");
    if ((uintptr_t)qpos % 4 != 0 || (uintptr_t)out % 4 != 0 || (uintptr_t)lb % 4 != 0 || (uintptr_t)ub % 4 != 0)
        return fail(STAC_ERR_INVALID, "stac_post_smooth: qpos / out / lb / ub must be 4-byte aligned");
    const int64_t bytes = N * nq * 4, bb = lb ? (int64_t)nq * 4 : 0;
    const HostBuf read[3] = {{"qpos", (uintptr_t)qpos, bytes}, {"lb", (uintptr_t)lb, bb}, {"ub", (uintptr_t)ub, bb}};
    for (const HostBuf &r : read) {  // (the inputs may share memory with each other; none may be written)
        const HostBuf pair[2] = {{"out", (uintptr_t)out, bytes}, r};
        const HostBuf *a, *b;
        if (find_overlap(pair, 2, &a, &b))
            return fail(STAC_ERR_INVALID, std::string("stac_post_smooth: ") + a->name + " and " + b->name +
                                              " overlap: windows read raw values, so in place is not possible");
    }
    return launch_result("stac_post_smooth",
                         launch_post_smooth(qpos, N, nq, clip_len, half_window, taps, Q, lb, ub, out, (hipStream_t)stream));
}
