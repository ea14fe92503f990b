// Filling missing keypoints along time (rule and shared functions: stac_prep.hpp; entry points: below the kernels).
//
// A staged scan over tiles of 64 frames, three launches on the caller's stream, no workgroup ever waits for another:
//   1. prep_summary_kernel: per tile and keypoint the first and last valid frame of the tile          -> first, last [K][tiles]
//   2. prep_carry_kernel:   per keypoint an exclusive prefix (last valid frame before the tile) and an
//                           exclusive suffix (first valid frame after it) over the tile summaries       -> prev, next  [K][tiles]
//   3. prep_fill_kernel:    re-reads the tile, finishes p / n inside it from the tile's validity masks,
//                           gathers the two source values and writes out and gap
// Kernels 1 and 3 work on one (tile, chunk of up to 64 keypoints) at a time.  A thread owns (frame, keypoint) pairs in the
// order of memory -- consecutive lanes read the three floats of consecutive keypoints of a frame row, then of the next row --
// so with K <= 64 a tile is one contiguous block of 64 * 3K floats, read and written in whole lines.  The validity of a
// pair goes to LDS as a byte; a wavefront whose lane l reads the byte of frame l then has the keypoint's 64-bit validity mask
// of the tile in one ballot.  Rows are 4-byte aligned only, hence dword accesses; offsets are 64-bit element offsets.
#include <hip/hip_runtime.h>

#include "stac_host.hpp"
#include "stac_prep.hpp"
#include "stac_prep_tile.hpp"

namespace stac {

namespace {

constexpr int kCarryThreads = 1024;  // (the tile walk, the masks and the other constants: stac_prep_tile.hpp)

__global__ __launch_bounds__(kPrepThreads) void prep_summary_kernel(const float *__restrict__ kp, int64_t T, int32_t K, int64_t tiles,
                                                                   int32_t chunks, int64_t *__restrict__ first,
                                                                   int64_t *__restrict__ last) {
    __shared__ PrepShared sh;
    const int64_t K3 = 3 * (int64_t)K, work = tiles * chunks;
    for (int64_t wk = blockIdx.x; wk < work; wk += gridDim.x) {
        const int64_t tile = wk / chunks;
        const int32_t k0 = (int32_t)(wk - tile * chunks) * kPrepChunk;
        const int32_t kc = K - k0 < kPrepChunk ? K - k0 : kPrepChunk;
        const int64_t t0 = tile * kPrepTileFrames;
        float v[kPrepPairs][3];
        prep_tile_masks(kp, T, K3, t0, k0, kc, v, sh);
        if ((int)threadIdx.x < kc) {
            const unsigned long long m = sh.mask[threadIdx.x];
            const int64_t at = (int64_t)(k0 + (int)threadIdx.x) * tiles + tile;
            first[at] = m ? t0 + (__ffsll(m) - 1) : -1;
            last[at] = m ? t0 + 63 - __clzll(m) : -1;
        }
        __syncthreads();  // sh is written again in the next sweep
    }
}

// One workgroup per keypoint, the tiles cut into one contiguous segment per thread: a combine over the segment, a scan over the
// 1024 segment summaries in LDS (forwards and backwards at once), then the segment again with the carried value.
__global__ __launch_bounds__(kCarryThreads) void prep_carry_kernel(const int64_t *__restrict__ first, const int64_t *__restrict__ last,
                                                                  int64_t *__restrict__ prev, int64_t *__restrict__ next,
                                                                  int64_t tiles) {
    __shared__ PrepSummary fwd[kCarryThreads], bwd[kCarryThreads];
    const int i = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * tiles;
    const int64_t S = (tiles + kCarryThreads - 1) / kCarryThreads;
    const int64_t lo = i * S < tiles ? i * S : tiles, hi = lo + S < tiles ? lo + S : tiles;
    PrepSummary s = prep_none();
    for (int64_t j = lo; j < hi; ++j) s = prep_combine(s, PrepSummary{first[base + j], last[base + j]});
    fwd[i] = s;  // -> combine of the segments 0 .. i
    bwd[i] = s;  // -> combine of the segments i .. 1023
    __syncthreads();
    for (int off = 1; off < kCarryThreads; off <<= 1) {
        const PrepSummary a = i >= off ? prep_combine(fwd[i - off], fwd[i]) : fwd[i];
        const PrepSummary b = i + off < kCarryThreads ? prep_combine(bwd[i], bwd[i + off]) : bwd[i];
        __syncthreads();
        fwd[i] = a;
        bwd[i] = b;
        __syncthreads();
    }
    PrepSummary run = i > 0 ? fwd[i - 1] : prep_none();
    for (int64_t j = lo; j < hi; ++j) {
        prev[base + j] = run.last;
        run = prep_combine(run, PrepSummary{first[base + j], last[base + j]});
    }
    run = i + 1 < kCarryThreads ? bwd[i + 1] : prep_none();
    for (int64_t j = hi - 1; j >= lo; --j) {
        next[base + j] = run.first;
        run = prep_combine(PrepSummary{first[base + j], last[base + j]}, run);
    }
}

__global__ __launch_bounds__(kPrepThreads) void prep_fill_kernel(const float *__restrict__ kp, int64_t T, int32_t K, int32_t mode,
                                                                int64_t tiles, int32_t chunks, const int64_t *__restrict__ prev,
                                                                const int64_t *__restrict__ next, float *__restrict__ out,
                                                                int32_t *__restrict__ gap) {
    __shared__ PrepShared sh;
    const int64_t K3 = 3 * (int64_t)K, work = tiles * chunks;
    for (int64_t wk = blockIdx.x; wk < work; wk += gridDim.x) {
        const int64_t tile = wk / chunks;
        const int32_t k0 = (int32_t)(wk - tile * chunks) * kPrepChunk;
        const int32_t kc = K - k0 < kPrepChunk ? K - k0 : kPrepChunk;
        const int64_t t0 = tile * kPrepTileFrames;
        float v[kPrepPairs][3];
        prep_tile_masks(kp, T, K3, t0, k0, kc, v, sh);
        PrepWalk w((uint32_t)kc);
#pragma unroll
        for (int i = 0; i < kPrepPairs; ++i) {
            const int64_t t = t0 + w.f;
            if (w.f < (uint32_t)kPrepTileFrames && t < T) {
                const int64_t kk = k0 + (int32_t)w.k;
                const unsigned long long m = sh.mask[w.k];
                float x = v[i][0], y = v[i][1], z = v[i][2];
                int32_t g = 0;
                if (!((m >> w.f) & 1ull)) {
                    const unsigned long long below = m & ((1ull << w.f) - 1ull);
                    const unsigned long long above = w.f == 63u ? 0ull : m >> (w.f + 1u);
                    const int64_t p = below ? t0 + 63 - __clzll(below) : prev[kk * tiles + tile];
                    const int64_t n = above ? t + 1 + (__ffsll(above) - 1) : next[kk * tiles + tile];
                    g = prep_gap(p, n, T);
                    if (p >= 0 || n >= 0) {  // (an empty track stays as it is)
                        const float *a = kp + (p >= 0 ? p : n) * K3 + 3 * kk;
                        const float *b = kp + (n >= 0 ? n : p) * K3 + 3 * kk;
                        x = prep_fill(mode, t, p, n, a[0], b[0]);
                        y = prep_fill(mode, t, p, n, a[1], b[1]);
                        z = prep_fill(mode, t, p, n, a[2], b[2]);
                    }
                }
                float *o = out + t * K3 + 3 * kk;
                o[0] = x;
                o[1] = y;
                o[2] = z;
                gap[t * K + kk] = g;
            }
            w.next();
        }
        __syncthreads();  // sh is written again in the next sweep
    }
}

}  // namespace

// Stages 1 and 2 (declared in stac_prep_tile.hpp: the donor fill of stac_donor.hip starts with the same two launches)
hipError_t launch_prep_scan(const float *kp, int64_t T, int32_t K, void *workspace, hipStream_t s) {
    const int64_t tiles = prep_tiles(T, kPrepTileFrames);
    const int32_t chunks = (K + kPrepChunk - 1) / kPrepChunk;
    int64_t *first = (int64_t *)workspace, *last = first + (int64_t)K * tiles, *prev = last + (int64_t)K * tiles,
            *next = prev + (int64_t)K * tiles;
    const int64_t work = tiles * chunks;
    const unsigned grid = (unsigned)(work < kPrepMaxBlocks ? work : kPrepMaxBlocks);
    hipLaunchKernelGGL(prep_summary_kernel, dim3(grid), dim3(kPrepThreads), 0, s, kp, T, K, tiles, chunks, first, last);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(prep_carry_kernel, dim3((unsigned)K), dim3(kCarryThreads), 0, s, first, last, prev, next, tiles);
    return hipGetLastError();
}

static hipError_t launch_prep_fill(const float *kp, int64_t T, int32_t K, int32_t mode, float *out, int32_t *gap, void *workspace,
                            hipStream_t s) {
    const int64_t tiles = prep_tiles(T, kPrepTileFrames);
    const int32_t chunks = (K + kPrepChunk - 1) / kPrepChunk;
    const int64_t *prev = (const int64_t *)workspace + 2 * (int64_t)K * tiles, *next = prev + (int64_t)K * tiles;
    const int64_t work = tiles * chunks;
    const unsigned grid = (unsigned)(work < kPrepMaxBlocks ? work : kPrepMaxBlocks);
    const hipError_t e = launch_prep_scan(kp, T, K, workspace, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(prep_fill_kernel, dim3(grid), dim3(kPrepThreads), 0, s, kp, T, K, mode, tiles, chunks, prev, next, out, gap);
    return hipGetLastError();
}

}  // namespace stac

// ---- C ABI entry points (include/stac_hip.h): every argument is checked before the device is touched ------------------------------
extern "C" int64_t stac_prep_fill_workspace(int64_t n_frames, int32_t n_kp) {
    const int64_t b = prep_workspace_bytes(n_frames, n_kp);
    if (b < 0) return fail(STAC_ERR_INVALID, "stac_prep_fill_workspace: n_frames >= 1, n_kp >= 1 (and a workspace size within int64)");
    return b;
}

extern "C" int32_t stac_prep_fill(const float *kp, int64_t n_frames, int32_t n_kp, int32_t mode, float *out, int32_t *gap,
                                  void *workspace, int64_t workspace_bytes, void *stream) {
    const int64_t need = prep_workspace_bytes(n_frames, n_kp);
    if (need < 0 || n_frames > (((int64_t)1 << 59) / n_kp))
        return fail(STAC_ERR_INVALID, "stac_prep_fill: n_frames >= 1, n_kp >= 1 (and array sizes within int64)");
    if (mode != STAC_PREP_LINEAR && mode != STAC_PREP_HOLD)
        return fail(STAC_ERR_INVALID, "stac_prep_fill: mode " + std::to_string(mode) + " is neither STAC_PREP_LINEAR nor STAC_PREP_HOLD");
    if (!kp || !out || !gap || !workspace) return fail(STAC_ERR_INVALID, "stac_prep_fill: null kp / out / gap / workspace");
    if (workspace_bytes < need)
        return fail(STAC_ERR_INVALID, "stac_prep_fill: workspace_bytes = " + std::to_string(workspace_bytes) + ", " +
                                          std::to_string(need) + " are needed (stac_prep_fill_workspace)");
    if ((uintptr_t)workspace % 8 != 0 || (uintptr_t)kp % 4 != 0 || (uintptr_t)out % 4 != 0 || (uintptr_t)gap % 4 != 0)
        return fail(STAC_ERR_INVALID, "stac_prep_fill: kp / out / gap must be 4-byte aligned, workspace 8-byte aligned");
    const int64_t kp_bytes = n_frames * n_kp * 12, gap_bytes = n_frames * n_kp * 4;
    const HostBuf buf[4] = {{"kp", (uintptr_t)kp, kp_bytes}, {"out", (uintptr_t)out, kp_bytes}, {"gap", (uintptr_t)gap, gap_bytes},
                            {"workspace", (uintptr_t)workspace, need}};
    const HostBuf *a, *b;
    if (find_overlap(buf, 4, &a, &b))
        return fail(STAC_ERR_INVALID, std::string("stac_prep_fill: ") + a->name + " and " + b->name +
                                          " overlap: source, outputs and workspace are distinct buffers");
    return launch_result("stac_prep_fill", launch_prep_fill(kp, n_frames, n_kp, mode, out, gap, workspace, (hipStream_t)stream));
}
