// Resampling fitted poses to another frame rate (rule and shared functions: stac_resample.hpp; entry points: below the kernel).
//
// Every output is a weighted sum of W = 2 H input rows of its column, so a kernel that reads them from global memory reads x many
// times over.  A workgroup therefore works on one tile of T consecutive outputs of one clip and one band of bw columns at a time
// (T: resample_tile_rows, bw: resample_band_cols; 512 threads; blockIdx.y is the band) and strides over the tiles with at most
// kResampleMaxBlocks workgroups per band:
//   1. the input rows that the tile's windows reach go to LDS as an image [rows][bw + 3]: row i of it is input row
//      n(first output) - H + 1 + i of the clip with the index clamped to 0 .. L - 1, so the held edges of a clip are materialised
//      and no window reads another clip.  Lanes run along the columns of a row (and on into the next row), so a load instruction of
//      a wavefront covers contiguous runs of a row; the three columns beyond the band's own belong to a quaternion block that
//      starts in it.  The phase rows of the tile (min(T, U) of them, slot f mod U holds the row of output f of the tile) and two
//      words per column (its bounds; a NaN lower bound marks a column of a quaternion block) stand in LDS as well.  Where T is a
//      multiple of U every tile starts at phase 0 and the phase rows are staged once per workgroup, else once per tile;
//   2. scalar pass: thread i computes elements i, i + 512, ... of the tile's outputs in the order of memory (resample_scalar over the
//      image, then the clamp), so the stores coalesce; the (output, column) of an element is stepped, not divided.  Lanes on a
//      column of a quaternion block sit this pass out;
//   3. quaternion pass: thread i computes whole blocks i, i + 512, ... of the tile (smooth_quat over the image with the block of
//      input row n as the centre) if the block starts in this band, and stores their four floats.
// With an odd row pitch of the image consecutive lanes of a row read consecutive banks.  Taps and rows are read through LDS
// addresses; nothing is kept in a per-lane array with run-time indices (no scratch).  The tap table is DEVICE memory (up to
// 32 KiB, more than kernel arguments carry).
#include <hip/hip_runtime.h>

#include "stac_host.hpp"
#include "stac_resample.hpp"

namespace stac {

namespace {

constexpr int kResampleThreads = 512;
constexpr int kResampleMaxBlocks = 1024;  // per band: 256 CUs x 4 workgroups; the grid strides over the tiles beyond that

// start columns of the quaternion blocks, by value in the kernel's arguments
struct ResampleQuat {
    int32_t n;
    int32_t col[kResampleMaxQuat];
};

__global__ __launch_bounds__(kResampleThreads) void resample_kernel(const float *__restrict__ x, float *__restrict__ out,
                                                                    const float *__restrict__ taps_dev, const float *__restrict__ lb,
                                                                    const float *__restrict__ ub, int32_t C, int64_t L, int64_t Lo, int32_t U,
                                                                    int32_t D, int32_t H, int32_t T, int32_t bw, int64_t tiles_per_clip,
                                                                    int64_t tiles, ResampleQuat Q) {
    extern __shared__ float resample_lds[];
    const int32_t W = 2 * H, slots = T < U ? T : U, pitch = bw + kResampleOverhang;
    float *taps = resample_lds;        // [slots][W]
    float *lo_col = taps + slots * W;  // [bw] lower bound of a scalar column (-inf without one); NaN: a quaternion column
    float *hi_col = lo_col + bw;       // [bw] upper bound (+inf without one)
    float *img = hi_col + bw;          // [<= resample_staged_rows(T)][pitch]
    const int32_t tid = threadIdx.x;
    const int32_t c0 = (int32_t)blockIdx.y * bw;                 // the band's first column
    const int32_t own = C - c0 < bw ? C - c0 : bw;               // its own columns
    const int32_t sw = C - c0 < pitch ? C - c0 : pitch;          // the columns of its image
    for (int32_t j = tid; j < own; j += kResampleThreads) {
        // a NaN bound clamps nothing (smooth_clamp compares), like an infinite one
        const float lo = lb ? lb[c0 + j] : -INFINITY, hi = ub ? ub[c0 + j] : INFINITY;
        lo_col[j] = lo == lo ? lo : -INFINITY;
        hi_col[j] = hi == hi ? hi : INFINITY;
    }
    __syncthreads();
    for (int32_t b = tid; b < 4 * Q.n; b += kResampleThreads) {
        const int32_t col = Q.col[b >> 2] + (b & 3) - c0;
        if (col >= 0 && col < own) lo_col[col] = __builtin_nanf("");
    }
    const bool fixed = T % U == 0;  // every tile of a clip starts at phase 0
    if (fixed)
        for (int32_t i = tid; i < U * W; i += kResampleThreads) {
            const int32_t f = i / W;
            taps[i] = taps_dev[((f * D) % U) * W + (i - f * W)];
        }
    // (the barrier behind the first tile's staging orders these writes before their reads)
    const int32_t ds = kResampleThreads / sw, djs = kResampleThreads - ds * sw;     // the (row, column) step of 512 elements of the image
    const int32_t df = kResampleThreads / own, dj = kResampleThreads - df * own;    // ... and of the outputs
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t clip = tile / tiles_per_clip;
        const int64_t m0 = (tile - clip * tiles_per_clip) * T;
        const int32_t nT = Lo - m0 < T ? (int32_t)(Lo - m0) : T;
        int64_t n0, n1;
        int32_t r0, r1;
        resample_index(m0, U, D, &n0, &r0);
        resample_index(m0 + nT - 1, U, D, &n1, &r1);
        if (!fixed)
            for (int32_t i = tid; i < (nT < U ? nT : U) * W; i += kResampleThreads) {
                const int32_t f = i / W;
                taps[i] = taps_dev[((r0 + f * D) % U) * W + (i - f * W)];
            }
        // 1: the image, input rows n0 - H + 1 .. n1 + H of the clip, clamped
        const int32_t rows = (int32_t)(n1 - n0) + W;  // <= resample_staged_rows(T)
        const float *src = x + clip * L * C + c0;
        const int64_t first = n0 - H + 1;
        {
            const int32_t staged = rows * sw;
            int32_t i = tid / sw, j = tid - i * sw;
            for (int32_t e = tid; e < staged; e += kResampleThreads) {
                int64_t row = first + i;
                row = row < 0 ? 0 : (row > L - 1 ? L - 1 : row);
                img[i * pitch + j] = src[row * C + j];
                i += ds;
                j += djs;
                if (j >= sw) {
                    j -= sw;
                    ++i;
                }
            }
        }
        __syncthreads();
        // 2: the scalar columns of the tile's outputs
        float *dst = out + (clip * Lo + m0) * C + c0;
        {
            const int32_t count = nT * own;
            int32_t f = tid / own, j = tid - f * own;
            for (int32_t e = tid; e < count; e += kResampleThreads) {
                const float lo = lo_col[j], hi = hi_col[j];
                if (lo == lo) {
                    const int32_t dn = (r0 + f * D) / U;  // n of the output less n0
                    const float v = resample_scalar(taps + (f % U) * W, img + dn * pitch + j, pitch, W);
                    dst[(int64_t)f * C + j] = smooth_clamp(v, lo, hi);
                }
                f += df;
                j += dj;
                if (j >= own) {
                    j -= own;
                    ++f;
                }
            }
        }
        // 3: the quaternion blocks that start in this band
        const int32_t blocks = nT * Q.n;
        for (int32_t e = tid; e < blocks; e += kResampleThreads) {
            const int32_t f = e / Q.n, col = Q.col[e - f * Q.n] - c0;
            if (col < 0 || col >= own) continue;
            const int32_t dn = (r0 + f * D) / U;
            float o[4];
            smooth_quat(taps + (f % U) * W, img + dn * pitch + col, pitch, W, img + (dn + H - 1) * pitch + col, o);
            float *d = dst + (int64_t)f * C + col;
            d[0] = o[0];
            d[1] = o[1];
            d[2] = o[2];
            d[3] = o[3];
        }
        __syncthreads();  // img (and, where they move, the phase rows) are written again in the next sweep
    }
}

hipError_t launch_post_resample(const float *x, int64_t N, int32_t C, int64_t L, int32_t U, int32_t D, int32_t H, const float *taps_dev,
                                const ResampleQuat &Q, const float *lb, const float *ub, float *out, hipStream_t s) {
    const int32_t bw = resample_band_cols(C), bands = (C + bw - 1) / bw, T = resample_tile_rows(bw, U, D, H);
    const int64_t Lo = resample_rows(L, U, D);
    const int64_t tiles_per_clip = (Lo + T - 1) / T, tiles = (N / L) * tiles_per_clip;
    const size_t lds = (size_t)resample_lds_floats(T, bw, U, D, H) * sizeof(float);  // <= kResampleLdsFloats floats (resample_tile_rows)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&resample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(kResampleLdsFloats * sizeof(float)));
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)(tiles < kResampleMaxBlocks ? tiles : kResampleMaxBlocks);
    hipLaunchKernelGGL(resample_kernel, dim3(grid, (unsigned)bands), dim3(kResampleThreads), lds, s, x, out, taps_dev, lb, ub, C, L, Lo, U, D, H,
                       T, bw, tiles_per_clip, tiles, Q);
    return hipGetLastError();
}

// The sizes that both entry points refuse: nullptr, or the text
const char *bad_ratio(int64_t L, int32_t U, int32_t D) {
    if (L < 1 || L > ((int64_t)1 << 56)) return "clip_len >= 1 (and row counts within int64)";
    if (U < 1 || U > kResampleMaxUp) return "up is outside 1 .. 32 (kResampleMaxUp)";
    if (D < 1 || D > kResampleMaxDown) return "down is outside 1 .. 64 (kResampleMaxDown)";
    return nullptr;
}

}  // namespace

}  // namespace stac

// ---- C ABI entry points (include/stac_hip.h): every argument is checked before the device is touched ------------------------
extern "C" int64_t stac_post_resample_rows(int64_t clip_len, int32_t up, int32_t down) {
    if (const char *bad = bad_ratio(clip_len, up, down)) return fail(STAC_ERR_INVALID, std::string("stac_post_resample_rows: ") + bad);
    return resample_rows(clip_len, up, down);
}

extern "C" int32_t stac_post_resample(const float *x, int64_t n_rows, int32_t n_cols, int64_t clip_len, int32_t up, int32_t down, int32_t half,
                                      const float *taps_dev, const int32_t *quat_cols, int32_t n_quat, const float *lb, const float *ub, float *out,
                                      int64_t out_rows, void *stream) {
    const std::string who = "stac_post_resample: ";
    if (n_rows < 0 || n_cols < 1 || n_rows > (((int64_t)1 << 54) / n_cols))
        return fail(STAC_ERR_INVALID, who + "n_rows >= 0, n_cols >= 1 (and array sizes within int64)");
    if (const char *bad = bad_ratio(clip_len, up, down)) return fail(STAC_ERR_INVALID, who + bad);
    if (half < 0 || half / up + 1 > kResampleMaxWin / 2)
        return fail(STAC_ERR_INVALID, who + "half = " + std::to_string(half) + " with up = " + std::to_string(up) + " makes a window of more than " +
                                          std::to_string(kResampleMaxWin) + " taps (kResampleMaxWin), or is negative");
    const int32_t H = resample_half_rows(half, up), W = 2 * H;
    if (n_rows % clip_len != 0)
        return fail(STAC_ERR_INVALID, who + std::to_string(n_rows) + " rows are not whole clips of " + std::to_string(clip_len));
    const int64_t want_rows = (n_rows / clip_len) * resample_rows(clip_len, up, down);
    if (out_rows != want_rows)
        return fail(STAC_ERR_INVALID, who + "out_rows = " + std::to_string(out_rows) + ", but " + std::to_string(n_rows / clip_len) + " clips of " +
                                          std::to_string(clip_len) + " rows give " + std::to_string(want_rows) + " (stac_post_resample_rows)");
    if (n_quat < 0 || n_quat > kResampleMaxQuat)
        return fail(STAC_ERR_INVALID, who + std::to_string(n_quat) + " quaternion blocks, at most " + std::to_string(kResampleMaxQuat) +
                                          " (kResampleMaxQuat)");
    if (n_quat > 0 && !quat_cols) return fail(STAC_ERR_INVALID, who + "null quat_cols");
    ResampleQuat Q{};
    Q.n = n_quat;
    for (int32_t b = 0; b < n_quat; ++b) {
        const int32_t col = quat_cols[b];
        if (col < 0 || col > n_cols - 4)
            return fail(STAC_ERR_INVALID, who + "the quaternion block at column " + std::to_string(col) + " leaves the row of " + std::to_string(n_cols));
        for (int32_t a = 0; a < b; ++a)
            if (col - Q.col[a] < 4 && Q.col[a] - col < 4)
                return fail(STAC_ERR_INVALID, who + "the quaternion blocks at columns " + std::to_string(Q.col[a]) + " and " + std::to_string(col) + " overlap");
        Q.col[b] = col;
    }
    if (!taps_dev) return fail(STAC_ERR_INVALID, who + "null taps_dev");
    if ((lb == nullptr) != (ub == nullptr)) return fail(STAC_ERR_INVALID, who + "lb and ub must be given together");
    if (n_rows == 0) return STAC_OK;
    if (!x || !out) return fail(STAC_ERR_INVALID, who + "null x / out");
    const int64_t bb = lb ? (int64_t)n_cols * 4 : 0;
    const HostBuf buf[5] = {{"x", (uintptr_t)x, n_rows * n_cols * 4, 4},
                            {"taps_dev", (uintptr_t)taps_dev, (int64_t)up * W * 4, 4},
                            {"lb", (uintptr_t)lb, bb, 4},
                            {"ub", (uintptr_t)ub, bb, 4},
                            {"out", (uintptr_t)out, out_rows * n_cols * 4, 4}};
    if (const int rc = check_buffers("stac_post_resample", buf, 5, " (in place is not possible)")) return rc;
    return launch_result("stac_post_resample",
                         launch_post_resample(x, n_rows, n_cols, clip_len, up, down, H, taps_dev, Q, lb, ub, out, (hipStream_t)stream));
}
