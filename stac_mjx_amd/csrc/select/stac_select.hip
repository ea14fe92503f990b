// Choosing calibration frames by pose diversity (rule: stac_select.hpp; entry points: below the kernels; C ABI: stac_select.h).
//
// 1 + 2 n launches on the caller's stream for n picks, no workgroup ever waits for another, nothing returns to the host:
//   select_describe_kernel  a wavefront takes a tile of 64 frames: it stages their rows in LDS with coalesced reads (rows of 3 K
//                           words, padded to an odd length so that the 64 lanes of a column read 64 banks), then one lane per frame
//                           writes the candidate flag, dmin = +inf and the P distances pair-major, dist[p][t]: 64 consecutive
//                           floats per store.
//   select_update_kernel    grid-strided, one frame per lane: the P distances of the last pick stand in LDS (every lane reads the
//                           same word: a broadcast), the lane streams column t of dist in the order of p (coalesced rows), folds
//                           acc into dmin[t] and keeps the largest key it has seen; shuffles reduce the keys of a wavefront, LDS
//                           those of the workgroup, and part[block] takes the result.  The launch in front of the first pick skips
//                           the sums (dmin is +inf everywhere: the largest key is the lowest-index candidate's).
//   select_pick_kernel      one workgroup: the largest of the part[] is pick i; it writes sel[i], radius2[i] and n_selected and
//                           gathers the pick's P distances into vec.  Once select_stops holds it raises state[0], and every later
//                           update returns at once and every later pick only writes its -1 / NaN.
// Offsets are 64-bit element offsets.  No kernel calls a function or keeps an array of its own.
#include <hip/hip_runtime.h>

#include <string>

#include "stac_select.h"
#include "stac_select.hpp"

using namespace stac;

namespace {

__global__ __launch_bounds__(kSelectTileFrames) void select_describe_kernel(const float *__restrict__ kp, int64_t T, int32_t K,
                                                                            const uint8_t *__restrict__ cand, int64_t stride, int64_t tiles,
                                                                            float *__restrict__ dist, float *__restrict__ dmin,
                                                                            uint8_t *__restrict__ flag, int32_t *__restrict__ state) {
    extern __shared__ float rows[];  // [kSelectTileFrames][row]
    const int32_t K3 = 3 * K, row = K3 | 1, lane = threadIdx.x;
    if (blockIdx.x == 0 && lane == 0) {
        state[0] = 0;
        state[1] = 0;
    }
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t t0 = tile * kSelectTileFrames;
        const int32_t nrow = T - t0 < kSelectTileFrames ? (int32_t)(T - t0) : kSelectTileFrames;
        const float *src = kp + t0 * K3;
        for (int32_t i = lane; i < nrow * K3; i += kSelectTileFrames) {
            const int32_t f = i / K3;
            rows[f * row + (i - f * K3)] = src[i];
        }
        __syncthreads();
        const int64_t t = t0 + lane;
        if (lane < nrow) {
            const float *r = rows + lane * row;
            flag[t] = select_candidate(r, K, cand ? cand[t] : (uint8_t)1) ? 1 : 0;
            dmin[t] = report_float(kSelectInfBits);
            float *d = dist + t;
            for (int32_t a = 0; a < K; ++a) {
                const float xa = r[3 * a], ya = r[3 * a + 1], za = r[3 * a + 2];
                for (int32_t b = a + 1; b < K; ++b) {
                    *d = pairwise_dist(xa, ya, za, r[3 * b], r[3 * b + 1], r[3 * b + 2]);
                    d += stride;
                }
            }
        }
        __syncthreads();  // rows is written again in the next sweep
    }
}

// The largest key of a workgroup of kSelectThreads threads, in thread 0 (wbest: one word per wavefront)
__device__ __forceinline__ uint64_t block_max_key(uint64_t best, uint64_t *wbest) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)best, off, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kSelectThreads / 64; ++w) best = wbest[w] > best ? wbest[w] : best;
    return best;
}

__global__ __launch_bounds__(kSelectThreads) void select_update_kernel(const float *__restrict__ dist, int64_t stride, int64_t T, int32_t P,
                                                                       float *__restrict__ dmin, const uint8_t *__restrict__ flag,
                                                                       const float *__restrict__ vec, const int32_t *__restrict__ state,
                                                                       uint64_t *__restrict__ part, int32_t first) {
    __shared__ float sv[kSelectMaxKp * (kSelectMaxKp - 1) / 2];
    __shared__ uint64_t wbest[kSelectThreads / 64];
    if (state[0]) return;  // (the whole grid alike: the selection has stopped)
    if (!first) {
        for (int32_t p = threadIdx.x; p < P; p += kSelectThreads) sv[p] = vec[p];
        __syncthreads();
    }
    uint64_t best = 0;
    for (int64_t t = (int64_t)blockIdx.x * kSelectThreads + threadIdx.x; t < T; t += (int64_t)gridDim.x * kSelectThreads) {
        if (!flag[t]) continue;
        float d = dmin[t];
        if (!first) {
            const float *col = dist + t;
            float acc = 0.0f;
#pragma unroll 8
            for (int32_t p = 0; p < P; ++p) acc = select_term(acc, col[(int64_t)p * stride], sv[p]);
            d = select_min(d, acc);
            dmin[t] = d;
        }
        const uint64_t key = select_key(d, t);
        best = key > best ? key : best;
    }
    best = block_max_key(best, wbest);
    if (threadIdx.x == 0) part[blockIdx.x] = best;
}

__global__ __launch_bounds__(kSelectThreads) void select_pick_kernel(const uint64_t *__restrict__ part, int32_t nblocks, int64_t i,
                                                                     const float *__restrict__ dist, int64_t stride, int32_t P,
                                                                     float *__restrict__ vec, int32_t *__restrict__ state,
                                                                     int64_t *__restrict__ sel, float *__restrict__ radius2,
                                                                     int64_t *__restrict__ n_selected) {
    __shared__ uint64_t wbest[kSelectThreads / 64];
    __shared__ uint64_t sbest;
    if (state[0]) {  // stopped at an earlier pick
        if (threadIdx.x == 0) {
            sel[i] = -1;
            radius2[i] = report_float(kSelectNanBits);
        }
        return;
    }
    uint64_t best = 0;
    for (int32_t b = threadIdx.x; b < nblocks; b += kSelectThreads) best = part[b] > best ? part[b] : best;
    best = block_max_key(best, wbest);  // (its barrier stands between every thread's read of state[0] and the write below)
    if (threadIdx.x == 0) sbest = best;
    __syncthreads();
    best = sbest;
    if (select_stops(best, i)) {
        if (threadIdx.x == 0) {
            state[0] = 1;
            sel[i] = -1;
            radius2[i] = report_float(kSelectNanBits);
            if (i == 0) *n_selected = 0;
        }
        return;
    }
    const int64_t s = select_key_frame(best);
    if (threadIdx.x == 0) {
        sel[i] = s;
        radius2[i] = report_float(select_key_bits(best));
        *n_selected = i + 1;
    }
    for (int32_t p = threadIdx.x; p < P; p += kSelectThreads) vec[p] = dist[(int64_t)p * stride + s];
}

hipError_t launch_select(const float *kp, int64_t T, int32_t K, const uint8_t *cand, int64_t n_select, int64_t *sel, float *radius2,
                         int64_t *n_selected, void *workspace, hipStream_t s) {
    const SelectLayout L = select_layout(T, K);
    char *w = (char *)workspace;
    float *dist = (float *)(w + L.dist), *dmin = (float *)(w + L.dmin), *vec = (float *)(w + L.vec);
    uint8_t *flag = (uint8_t *)(w + L.flag);
    uint64_t *part = (uint64_t *)(w + L.part);
    int32_t *state = (int32_t *)(w + L.state);
    const int64_t tiles = L.stride / kSelectTileFrames;
    const unsigned dgrid = (unsigned)(tiles < kSelectMaxTiles ? tiles : kSelectMaxTiles), ugrid = (unsigned)L.blocks;
    const size_t lds = sizeof(float) * kSelectTileFrames * (size_t)((3 * K) | 1);
    const int32_t P = (int32_t)L.pairs;
    hipLaunchKernelGGL(select_describe_kernel, dim3(dgrid), dim3(kSelectTileFrames), lds, s, kp, T, K, cand, L.stride, tiles, dist, dmin, flag, state);
    for (int64_t i = 0; i < n_select; ++i) {
        hipLaunchKernelGGL(select_update_kernel, dim3(ugrid), dim3(kSelectThreads), 0, s, dist, L.stride, T, P, dmin, flag, vec, state, part,
                           i == 0 ? 1 : 0);
        hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(kSelectThreads), 0, s, part, (int32_t)ugrid, i, dist, L.stride, P, vec, state, sel,
                           radius2, n_selected);
        if ((i & 63) == 63) {  // (a failed launch is reported within 64 picks, not after all of them)
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    return hipGetLastError();
}

// ---- error state of the calling thread (this library's own: it does not link against libstac_hip.so) ------------------------------
thread_local std::string g_err;
thread_local int32_t g_err_code = 0;
int fail(int code, const std::string &msg) {
    g_err = msg;
    g_err_code = code;
    return code;
}

struct Buf { const char *name; uintptr_t lo; int64_t bytes; int align; };

}  // namespace

// ---- C ABI entry points (stac_select.h): every argument is checked before the device is touched ----------------------------------
extern "C" const char *stac_select_last_error(void) { return g_err.c_str(); }
extern "C" int32_t stac_select_last_error_code(void) { return g_err_code; }

static int64_t select_bytes(const char *who, int64_t n_frames, int32_t n_kp) {
    if (n_frames < 1 || n_kp < 2) return fail(STAC_ERR_INVALID, std::string(who) + ": n_frames >= 1, n_kp >= 2 (a frame is described by the distances of its pairs)");
    if (n_kp > kSelectMaxKp)
        return fail(STAC_ERR_CAPACITY, std::string(who) + ": n_kp = " + std::to_string(n_kp) + " exceeds the " + std::to_string(kSelectMaxKp) + " keypoints of a descriptor");
    if (n_frames > kSelectMaxFrames)
        return fail(STAC_ERR_CAPACITY, std::string(who) + ": n_frames = " + std::to_string(n_frames) + " exceeds the 2^32 - 1 frames that the key of a pick can name");
    return select_layout(n_frames, n_kp).bytes;
}

extern "C" int64_t stac_select_workspace(int64_t n_frames, int32_t n_kp) { return select_bytes("stac_select_workspace", n_frames, n_kp); }

extern "C" int32_t stac_select_diverse(const float *kp, int64_t n_frames, int32_t n_kp, const uint8_t *cand, int64_t n_select, int64_t *sel,
                                       float *radius2, int64_t *n_selected, void *workspace, int64_t workspace_bytes, void *stream) {
    const char *who = "stac_select_diverse";
    const int64_t need = select_bytes(who, n_frames, n_kp);
    if (need < 0) return (int32_t)need;
    if (n_select < 1 || n_select > n_frames)
        return fail(STAC_ERR_INVALID, std::string(who) + ": n_select = " + std::to_string(n_select) + " is outside 1 .. n_frames = " + std::to_string(n_frames));
    if (!kp || !sel || !radius2 || !n_selected || !workspace) return fail(STAC_ERR_INVALID, std::string(who) + ": null kp / sel / radius2 / n_selected / workspace");
    if (workspace_bytes < need)
        return fail(STAC_ERR_INVALID, std::string(who) + ": workspace_bytes = " + std::to_string(workspace_bytes) + ", " + std::to_string(need) +
                                          " are needed (stac_select_workspace)");
    const Buf buf[6] = {{"kp", (uintptr_t)kp, n_frames * n_kp * 12, 4}, {"cand", (uintptr_t)cand, cand ? n_frames : 0, 1},
                        {"sel", (uintptr_t)sel, n_select * 8, 8},       {"radius2", (uintptr_t)radius2, n_select * 4, 4},
                        {"n_selected", (uintptr_t)n_selected, 8, 8},    {"workspace", (uintptr_t)workspace, need, 8}};
    for (const Buf &b : buf)
        if (b.lo % b.align != 0) return fail(STAC_ERR_INVALID, std::string(who) + ": " + b.name + " must be " + std::to_string(b.align) + "-byte aligned");
    for (int i = 0; i < 6; ++i)
        for (int j = i + 1; j < 6; ++j)
            if (buf[i].bytes && buf[j].bytes && buf[i].lo < buf[j].lo + (uintptr_t)buf[j].bytes && buf[j].lo < buf[i].lo + (uintptr_t)buf[i].bytes)
                return fail(STAC_ERR_INVALID, std::string(who) + ": " + buf[i].name + " and " + buf[j].name +
                                                  " overlap: inputs, outputs and workspace are distinct buffers");
    const hipError_t e = launch_select(kp, n_frames, n_kp, cand, n_select, sel, radius2, n_selected, workspace, (hipStream_t)stream);
    if (e != hipSuccess) return fail(STAC_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return fail(STAC_OK, "");
}
