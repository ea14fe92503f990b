// Rejecting keypoint outliers along time (rule and shared function: stac_outlier.hpp; entry point: below the kernel).
//
// One launch, no workspace, no workgroup ever waits for another.  A workgroup works on one (tile of 64 frames, chunk of up to 32
// keypoints) at a time and strides over the work with at most kPrepMaxBlocks workgroups:
//   1. the tile and a halo of h frames on each side -- 64 + 2 h rows of 3 kc floats -- go to LDS as one dense image, SANITIZED: the
//      three coordinates of a missing keypoint and every row outside the series are NaN, so the clipping of the window at both ends
//      of the series and the validity of a neighbour are both "a NaN counts for nothing" (stac_outlier.hpp).  A thread stages
//      (row, keypoint) pairs in the order of memory, so consecutive lanes read consecutive keypoints of a frame row in whole lines
//      (rows are 4-byte aligned only, hence dword accesses; 64-bit element offsets);
//   2. a thread decides (frame, keypoint) pairs of the tile in the same order: outlier_coord per coordinate by rank counting over
//      the LDS image (the image is dense, so pair e lies at dword 3 e and every lane of a wavefront reads the same row offset:
//      consecutive lanes are 3 dwords apart, and 3 is coprime to the 32 banks of a ds_read_b32 -- no conflicts at any kc), and
//      writes its three floats of out and its byte of flag.
// Nothing is kept in a per-lane array (no scratch): the centre value is read back from the image, and only a MISSING keypoint,
// whose image holds NaN, reads its raw coordinates again from global memory to pass them on bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>

#include "stac_host.hpp"
#include "stac_outlier.hpp"

namespace stac {

namespace {

constexpr int kOutlierThreads = 256;
constexpr int kOutlierChunk = 32;                                  // keypoints of a chunk
constexpr int kOutlierRows = kPrepTileFrames + 2 * kOutlierMaxHalf;  // rows of the LDS image at most: 96
constexpr int kOutlierImage = kOutlierRows * 3 * kOutlierChunk;     // floats: 9 216 = 36 864 bytes

__global__ __launch_bounds__(kOutlierThreads) void outlier_reject_kernel(const float *__restrict__ kp, int64_t T, int32_t K, int32_t h,
                                                                         double thr, double min_dev, int64_t tiles, int32_t chunks,
                                                                         float *__restrict__ out, uint8_t *__restrict__ flag) {
    __shared__ float img[kOutlierImage];
    const int64_t K3 = 3 * (int64_t)K, work = tiles * chunks;
    const float nan = outlier_nan();
    for (int64_t wk = blockIdx.x; wk < work; wk += gridDim.x) {
        const int64_t tile = wk / chunks;
        const int32_t k0 = (int32_t)(wk - tile * chunks) * kOutlierChunk;
        const int32_t kc = K - k0 < kOutlierChunk ? K - k0 : kOutlierChunk;
        const int64_t t0 = tile * kPrepTileFrames;
        const int32_t stride = 3 * kc;
        // 1: the image, rows t0 - h .. t0 + 63 + h
        const int32_t staged = (kPrepTileFrames + 2 * h) * kc;  // <= 96 * 32 pairs
        for (int32_t e = threadIdx.x; e < staged; e += kOutlierThreads) {
            const int32_t r = e / kc, k = e - r * kc;
            const int64_t t = t0 - h + r;
            float x = nan, y = nan, z = nan;
            if (t >= 0 && t < T) {
                const float *s = kp + t * K3 + 3 * (int64_t)(k0 + k);
                x = s[0];
                y = s[1];
                z = s[2];
                if (prep_missing(x, y, z)) x = y = z = nan;
            }
            float *d = img + 3 * e;
            d[0] = x;
            d[1] = y;
            d[2] = z;
        }
        __syncthreads();
        // 2: the decisions of the tile's own rows
        const int32_t own = kPrepTileFrames * kc;
        for (int32_t e = threadIdx.x; e < own; e += kOutlierThreads) {
            const int32_t f = e / kc, k = e - f * kc;
            const int64_t t = t0 + f;
            if (t >= T) break;  // (e grows with f: the rest of this thread's pairs lie past the series as well)
            const float *c = img + 3 * (h * kc + e);  // the centre: row h + f of the image
            float x = c[0], y = c[1], z = c[2];
            const int64_t at = t * K3 + 3 * (int64_t)(k0 + k);
            uint8_t rejected = 0;
            if (x != x) {  // missing (sanitized): its raw coordinates pass as they came
                x = kp[at];
                y = kp[at + 1];
                z = kp[at + 2];
            } else if (outlier_coord(c, stride, h, thr, min_dev) || outlier_coord(c + 1, stride, h, thr, min_dev) ||
                       outlier_coord(c + 2, stride, h, thr, min_dev)) {
                x = y = z = nan;
                rejected = 1;
            }
            out[at] = x;
            out[at + 1] = y;
            out[at + 2] = z;
            flag[t * K + (k0 + k)] = rejected;
        }
        __syncthreads();  // img is written again in the next sweep
    }
}

}  // namespace

static hipError_t launch_outlier_reject(const float *kp, int64_t T, int32_t K, int32_t h, double thr, double min_dev, float *out, uint8_t *flag,
                                 hipStream_t s) {
    const int64_t tiles = prep_tiles(T, kPrepTileFrames);
    const int32_t chunks = (K + kOutlierChunk - 1) / kOutlierChunk;
    const int64_t work = tiles * chunks;
    const unsigned grid = (unsigned)(work < kPrepMaxBlocks ? work : kPrepMaxBlocks);
    hipLaunchKernelGGL(outlier_reject_kernel, dim3(grid), dim3(kOutlierThreads), 0, s, kp, T, K, h, thr, min_dev, tiles, chunks, out, flag);
    return hipGetLastError();
}

}  // namespace stac

// ---- C ABI entry point (include/stac_hip.h): every argument is checked before the device is touched -------------------------------
extern "C" int32_t stac_prep_reject(const float *kp, int64_t n_frames, int32_t n_kp, int32_t half_window, double thr, double min_dev,
                                    float *out, uint8_t *flag, void *stream) {
    if (n_frames < 1 || n_kp < 1 || n_frames > (((int64_t)1 << 59) / n_kp))
        return fail(STAC_ERR_INVALID, "stac_prep_reject: n_frames >= 1, n_kp >= 1 (and array sizes within int64)");
    if (half_window < 1 || half_window > kOutlierMaxHalf)
        return fail(STAC_ERR_INVALID, "stac_prep_reject: half_window " + std::to_string(half_window) + " is outside 1 .. " +
                                          std::to_string(kOutlierMaxHalf));
    if (!std::isfinite(thr) || thr < 0.0 || !std::isfinite(min_dev) || min_dev < 0.0)
        return fail(STAC_ERR_INVALID, "stac_prep_reject: thr and min_dev must be finite and >= 0");
    if (!kp || !out || !flag) return fail(STAC_ERR_INVALID, "stac_prep_reject: null kp / out / flag");
    if ((uintptr_t)kp % 4 != 0 || (uintptr_t)out % 4 != 0) return fail(STAC_ERR_INVALID, "stac_prep_reject: kp / out must be 4-byte aligned");
    const int64_t kp_bytes = n_frames * n_kp * 12, flag_bytes = n_frames * n_kp;
    const HostBuf buf[3] = {{"kp", (uintptr_t)kp, kp_bytes}, {"out", (uintptr_t)out, kp_bytes}, {"flag", (uintptr_t)flag, flag_bytes}};
    const HostBuf *a, *b;
    if (find_overlap(buf, 3, &a, &b))
        return fail(STAC_ERR_INVALID, std::string("stac_prep_reject: ") + a->name + " and " + b->name +
                                          " overlap: neighbours read raw values, so in place is not possible");
    return launch_result("stac_prep_reject", launch_outlier_reject(kp, n_frames, n_kp, half_window, thr, min_dev, out, flag, (hipStream_t)stream));
}
