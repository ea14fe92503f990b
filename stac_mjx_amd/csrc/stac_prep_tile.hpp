// What the units that scan keypoint tracks along time share on the device (stac_prep.hip: the fill; stac_donor.hip: the donor fill):
// the walk of a workgroup over a tile of 64 frames in the order of memory, the tile's validity masks by ballot, and the launch of
// the first two stages of the staged scan (tile summaries, carries across tiles).  Device code: only .hip units include it.
#pragma once
#include <hip/hip_runtime.h>

#include "stac_prep.hpp"

namespace stac {

// Stages 1 and 2 of DESIGN.md §10 on stream s (prep_summary_kernel, prep_carry_kernel; defined in stac_prep.hip): leaves, in the
// four int64 arrays [K][tiles] of a workspace of prep_workspace_bytes(T, K) bytes (first, last, prev, next, in that order), per tile
// and keypoint the last valid frame before the tile in `prev` and the first valid frame after it in `next` (-1: none).
__attribute__((visibility("hidden"))) hipError_t launch_prep_scan(const float *kp, int64_t T, int32_t K, void *workspace, hipStream_t s);

namespace {

constexpr int kPrepThreads = 256;
constexpr int kPrepWaves = kPrepThreads / 64;
constexpr int kPrepChunk = 64;                                            // keypoints of a chunk
constexpr int kPrepPairs = kPrepTileFrames * kPrepChunk / kPrepThreads;  // (frame, keypoint) pairs of a thread: 16
constexpr int kPrepFlagRow = kPrepChunk + 4;  // bytes of a frame's flags in LDS: 17 dwords, so the 64 rows a ballot reads differ in bank

static_assert(kPrepTileFrames == 64, "a tile is what one 64-lane ballot covers");

struct PrepShared {
    uint8_t flags[kPrepTileFrames][kPrepFlagRow];
    unsigned long long mask[kPrepChunk];
};

// Walks the pairs of this thread in (tile, chunk): pair e = i * 256 + threadIdx.x is frame e / kc, keypoint e % kc of the chunk
struct PrepWalk {
    uint32_t f, k, qf, qk, kc;
    __device__ PrepWalk(uint32_t kc_) : kc(kc_) {
        f = threadIdx.x / kc;
        k = threadIdx.x - f * kc;
        qf = kPrepThreads / kc;
        qk = kPrepThreads - qf * kc;
    }
    __device__ void next() {
        f += qf;
        k += qk;
        if (k >= kc) {
            k -= kc;
            ++f;
        }
    }
};

// Stage A + B of kernels 1 and 3: loads the pairs of (tile at frame t0, keypoints k0 .. k0 + kc - 1) into v and leaves the
// validity mask of every keypoint of the chunk (bit f = frame t0 + f is valid; frames >= T are not) in sh.mask.
__device__ __forceinline__ void prep_tile_masks(const float *__restrict__ kp, int64_t T, int64_t K3, int64_t t0, int32_t k0, int32_t kc,
                                                float (&v)[kPrepPairs][3], PrepShared &sh) {
    PrepWalk w((uint32_t)kc);
#pragma unroll
    for (int i = 0; i < kPrepPairs; ++i) {
        v[i][0] = v[i][1] = v[i][2] = 0.0f;
        if (w.f < (uint32_t)kPrepTileFrames) {
            const int64_t t = t0 + w.f;
            bool ok = false;
            if (t < T) {
                const float *s = kp + t * K3 + 3 * (int64_t)(k0 + (int32_t)w.k);
                v[i][0] = s[0];
                v[i][1] = s[1];
                v[i][2] = s[2];
                ok = !prep_missing(v[i][0], v[i][1], v[i][2]);
            }
            sh.flags[w.f][w.k] = ok ? 1 : 0;
        }
        w.next();
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int k = threadIdx.x >> 6; k < kc; k += kPrepWaves) {
        const unsigned long long m = __ballot(sh.flags[lane][k] != 0);
        if (lane == 0) sh.mask[k] = m;
    }
    __syncthreads();
}

}  // namespace

}  // namespace stac
