// Filling long keypoint gaps from rigid neighbours (rule: stac_donor.hpp; entry points: below the kernel).
//
// Three launches on the caller's stream, no workgroup ever waits for another.  The first two are stages 1 and 2 of the staged scan
// of stac_prep.hip (launch_prep_scan: per tile of 64 frames and keypoint the last valid frame before the tile and the first valid one
// after it).  The third is donor_fill_kernel: a workgroup takes a tile, leaves the validity mask of every keypoint of the tile in LDS
// (one ballot per keypoint, stac_prep_tile.hpp), and then walks the tile's (frame, keypoint) pairs in the order of memory.  An observed
// pair passes; a missing one finishes p / n by two bit scans of its mask (a run that leaves the tile reads a carry), tests its donors
// in its own frame in the LDS masks, reads them at p and n from memory and tests them there, and takes the first usable triple of its
// list.  The donor table [K][D][3] sits in LDS, so a lane reads its rows by address and keeps no array of its own.
// K <= 64: one chunk of the tile walk holds all keypoints.  Offsets are 64-bit element offsets; rows are 4-byte aligned only.
#include <hip/hip_runtime.h>

#include "stac_donor.hpp"
#include "stac_host.hpp"
#include "stac_prep_tile.hpp"

namespace stac {

namespace {

struct DonorShared {
    PrepShared tile;
    int32_t don[kDonorMaxKp * kDonorMaxTriples * 3];
};

__global__ __launch_bounds__(kPrepThreads) void donor_fill_kernel(const float *__restrict__ kp, int64_t T, int32_t K, int64_t tiles,
                                                                 const int32_t *__restrict__ don, int32_t D,
                                                                 const int64_t *__restrict__ prev, const int64_t *__restrict__ next,
                                                                 float *__restrict__ out, int32_t *__restrict__ gap,
                                                                 uint8_t *__restrict__ src) {
    __shared__ DonorShared sh;
    const int64_t K3 = 3 * (int64_t)K;
    const int32_t rows = K * D * 3;  // <= 64 * 8 * 3: what sh.don holds
    for (int32_t i = threadIdx.x; i < rows; i += kPrepThreads) sh.don[i] = don[i];
    // (prep_tile_masks has two barriers before the table is read)
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t t0 = tile * kPrepTileFrames;
        float v[kPrepPairs][3];  // the masks are all this kernel keeps of the first read: the walk below reads its pair again
        prep_tile_masks(kp, T, K3, t0, 0, K, v, sh.tile);
        PrepWalk w((uint32_t)K);
#pragma unroll 1
        for (int i = 0; i < kPrepPairs; ++i) {
            const int64_t t = t0 + w.f;
            if (w.f < (uint32_t)kPrepTileFrames && t < T) {
                const int32_t k = (int32_t)w.k;
                const float *s = kp + t * K3 + 3 * k;
                float o[3] = {s[0], s[1], s[2]};
                const unsigned long long m = sh.tile.mask[k];
                int32_t g = 0, from = kDonorObserved;
                if (!((m >> w.f) & 1ull)) {
                    const unsigned long long below = m & ((1ull << w.f) - 1ull);
                    const unsigned long long above = w.f == 63u ? 0ull : m >> (w.f + 1u);
                    const int64_t p = below ? t0 + 63 - __clzll(below) : prev[(int64_t)k * tiles + tile];
                    const int64_t n = above ? t + 1 + (__ffsll(above) - 1) : next[(int64_t)k * tiles + tile];
                    g = prep_gap(p, n, T);
                    from = kDonorLeft;
                    if (p >= 0 || n >= 0) {  // (an empty track stays as it is)
                        for (int32_t d = 0; d < D; ++d) {
                            const int32_t *row = sh.don + (k * D + d) * 3;
                            const int32_t a = row[0], b = row[1], c = row[2];
                            if (!donor_row(k, K, a, b, c)) break;  // the end of this keypoint's list
                            const bool here = ((sh.tile.mask[a] >> w.f) & (sh.tile.mask[b] >> w.f) & (sh.tile.mask[c] >> w.f) & 1ull) != 0;
                            float r[3];
                            if (here && donor_try(kp, K3, t, p, n, k, a, b, c, r)) {
                                o[0] = r[0];
                                o[1] = r[1];
                                o[2] = r[2];
                                from = d + 1;
                                break;
                            }
                        }
                    }
                }
                float *q = out + t * K3 + 3 * k;
                q[0] = o[0];
                q[1] = o[1];
                q[2] = o[2];
                gap[t * K + k] = g;
                src[t * K + k] = (uint8_t)from;
            }
            w.next();
        }
        __syncthreads();  // sh.tile is written again in the next sweep
    }
}

hipError_t launch_donor(const float *kp, int64_t T, int32_t K, const int32_t *don, int32_t D, float *out, int32_t *gap, uint8_t *src,
                        void *workspace, hipStream_t s) {
    const int64_t tiles = prep_tiles(T, kPrepTileFrames);
    const int64_t *prev = (const int64_t *)workspace + 2 * (int64_t)K * tiles, *next = prev + (int64_t)K * tiles;
    const hipError_t e = launch_prep_scan(kp, T, K, workspace, s);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)(tiles < kPrepMaxBlocks ? tiles : kPrepMaxBlocks);
    hipLaunchKernelGGL(donor_fill_kernel, dim3(grid), dim3(kPrepThreads), 0, s, kp, T, K, tiles, don, D, prev, next, out, gap, src);
    return hipGetLastError();
}

}  // namespace

}  // namespace stac

// ---- C ABI entry points (include/stac_hip.h): every argument is checked before the device is touched --------------------------
extern "C" int64_t stac_prep_donor_workspace(int64_t n_frames, int32_t n_kp) {
    const int64_t b = prep_workspace_bytes(n_frames, n_kp);
    if (b < 0) return fail(STAC_ERR_INVALID, "stac_prep_donor_workspace: n_frames >= 1, n_kp >= 1 (and a workspace size within int64)");
    if (n_kp > kDonorMaxKp)
        return fail(STAC_ERR_CAPACITY, "stac_prep_donor_workspace: n_kp = " + std::to_string(n_kp) + " exceeds the " +
                                           std::to_string(kDonorMaxKp) + " keypoints whose masks a tile holds");
    return b;
}

extern "C" int32_t stac_prep_donor(const float *kp, int64_t n_frames, int32_t n_kp, const int32_t *don, int32_t n_triples, float *out,
                                   int32_t *gap, uint8_t *src, void *workspace, int64_t workspace_bytes, void *stream) {
    const int64_t need = prep_workspace_bytes(n_frames, n_kp);
    if (need < 0 || n_frames > (((int64_t)1 << 59) / n_kp))
        return fail(STAC_ERR_INVALID, "stac_prep_donor: n_frames >= 1, n_kp >= 1 (and array sizes within int64)");
    if (n_kp > kDonorMaxKp)
        return fail(STAC_ERR_CAPACITY, "stac_prep_donor: n_kp = " + std::to_string(n_kp) + " exceeds the " + std::to_string(kDonorMaxKp) +
                                           " keypoints whose masks a tile holds");
    if (n_triples < 1 || n_triples > kDonorMaxTriples)
        return fail(STAC_ERR_INVALID, "stac_prep_donor: n_triples = " + std::to_string(n_triples) + " is outside 1 .. " +
                                          std::to_string(kDonorMaxTriples));
    if (!kp || !don || !out || !gap || !src || !workspace)
        return fail(STAC_ERR_INVALID, "stac_prep_donor: null kp / don / out / gap / src / workspace");
    if (workspace_bytes < need)
        return fail(STAC_ERR_INVALID, "stac_prep_donor: workspace_bytes = " + std::to_string(workspace_bytes) + ", " +
                                          std::to_string(need) + " are needed (stac_prep_donor_workspace)");
    const int64_t kp_bytes = n_frames * n_kp * 12, gap_bytes = n_frames * n_kp * 4, src_bytes = n_frames * n_kp;
    const HostBuf buf[6] = {{"kp", (uintptr_t)kp, kp_bytes, 4},    {"don", (uintptr_t)don, (int64_t)n_kp * n_triples * 12, 4},
                            {"out", (uintptr_t)out, kp_bytes, 4},  {"gap", (uintptr_t)gap, gap_bytes, 4},
                            {"src", (uintptr_t)src, src_bytes, 1}, {"workspace", (uintptr_t)workspace, need, 8}};
    if (const int rc = check_buffers("stac_prep_donor", buf, 6, " (in place is not possible)")) return rc;
    return launch_result("stac_prep_donor", launch_donor(kp, n_frames, n_kp, don, n_triples, out, gap, src, workspace, (hipStream_t)stream));
}
