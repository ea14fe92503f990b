// Rejecting keypoints that break pairwise distances (rule and shared functions: stac_pairwise.hpp; entry points: below the kernels).
//
// One call, two memsets and 14 launches on the caller's stream, no copy to the host, no workgroup ever waits for another:
//   0. memset of the histograms in the workspace (everything the first selection adds into)
//   1. pairwise_dist_kernel:   reads kp once; leaves, in the workspace, the KEY of every (pair, frame) in pair-major order
//                              (keys [P][stride]: the bits of d_p(t), kReportNoKey where the pair is not valid)
//   2. the selection of the two middle order statistics of d per pair -- the scheme of stac_report.hip, with the two ranks
//      (n - 1) / 2 and n / 2 in the place of its quantiles: pairwise_count_kernel (pass 0: keys -> hist0 [P][1024] by bits >> 21),
//      pairwise_finish_kernel (-> pair_n and, per rank, the bin that holds it and the rank inside the bin), count and finish of
//      pass 1 (the next 11 bits of the keys whose top 11 match) and of pass 2 (the last 10 bits) -> pair_med
//   3. memset of the histograms again, and the same six launches over the keys of e_p(t), which a counting pass computes from the
//      key of d_p(t) and pair_med as it reads (nothing is stored twice) -> pair_mad
//   4. pairwise_decide_kernel: one lane per frame, one wavefront per tile of 64 frames.  A lane reads the keys of its frame (the
//      lanes of a wavefront read 256 contiguous bytes of a pair's row), marks the bad pairs in its column of LDS (K words of 64
//      bits per frame, word k of frame f at [k][f]: the 32 lanes of a half-wavefront read 32 consecutive 8-byte words, one 256-byte
//      bank row of a ds_read_b64, no bank conflict at any K) and
//      blames (pairwise_blame: population counts over the column; no per-lane array, nothing in scratch).  The wavefront then
//      writes the tile's out and flag in the order of memory, whole lines, from kp and the 64 reject words.
// The first pass stages a tile of 64 frames in LDS by whole-line reads (rows are 4-byte aligned only, hence dword accesses; 64-bit
// element offsets) with a row stride of 3 K | 1 words: odd, hence coprime to the 32 banks of a ds_read_b32, so the 32 lanes of each
// half of a wavefront, one frame each, read one coordinate from 32 different banks at any K (3 K itself is even for even K).  Every
// wavefront then takes pairs with a lane per frame and writes 256-byte lines of the key rows.
// The counting passes keep a histogram per workgroup in LDS (integer atomics on per-lane addresses) and add its non-empty bins to
// global memory with 64-bit integer atomics: the counts do not depend on their order.
//
// Repairing swaps (rule: stac_swap.hpp; stac_prep_swaps below) is the same statistics part -- steps 0 to 3, the same launches -- and
//   4'. pairwise_swap_kernel: one lane per frame, one wavefront per tile of 64 frames, like step 4.  The candidate table comes by
//       value as kernel arguments (four candidates per 64-bit word) and goes into LDS by compile-time-indexed stores: no copy from
//       host memory on the stream, no run-time-indexed private array.  Per candidate (the same for every lane) and third keypoint k
//       a lane reads the keys of {a, k} and {b, k} of its frame (256 contiguous bytes of each row per wavefront); n, med and
//       thr * mad of the two pairs are the same for every lane.  b0 and b1 live in registers, the frame's decisions are 32 bits in
//       LDS.  The wavefront then writes the tile's out in the order of memory: element (frame, keypoint) reads kp at its partner if
//       its candidate swaps, else at itself; flag [T][S] likewise.
#include <hip/hip_runtime.h>

#include <cmath>

#include "stac_host.hpp"
#include "stac_pairwise.hpp"
#include "stac_swap.hpp"

namespace stac {

namespace {

constexpr int kPairwiseThreads = 256;
constexpr int kPairwiseWaves = kPairwiseThreads / 64;

static_assert(kPairwiseTileFrames == 64, "a tile is one wavefront lane per frame");
static_assert(kReportBins0 % kPairwiseThreads == 0 && kReportBins1 % kPairwiseThreads == 0 && kReportBins2 % kPairwiseThreads == 0, "bins per thread");

// dynamic LDS: 64 rows of rs = 3 K | 1 floats
__global__ __launch_bounds__(kPairwiseThreads) void pairwise_dist_kernel(const float *__restrict__ kp, int64_t T, int32_t K, int64_t tiles,
                                                                        int64_t stride, uint32_t *__restrict__ keys) {
    extern __shared__ float rows[];
    const int32_t K3 = 3 * K, rs = K3 | 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t t0 = tile * kPairwiseTileFrames;
        const int64_t left = T - t0;
        const int32_t nf = left < kPairwiseTileFrames ? (int32_t)left : kPairwiseTileFrames;
        const float *src = kp + t0 * K3;
        for (int32_t e = threadIdx.x; e < nf * K3; e += kPairwiseThreads) {
            const int32_t f = e / K3, j = e - f * K3;
            rows[f * rs + j] = src[e];
        }
        __syncthreads();
        if (lane < nf) {
            const float *r = rows + lane * rs;
            int32_t p = 0;
            for (int32_t a = 0; a + 1 < K; ++a) {
                const float xa = r[3 * a], ya = r[3 * a + 1], za = r[3 * a + 2];
                for (int32_t b = a + 1; b < K; ++b, ++p) {
                    if ((p & (kPairwiseWaves - 1)) != wave) continue;  // (the same for every lane of a wavefront)
                    keys[(int64_t)p * stride + t0 + lane] = pairwise_key(xa, ya, za, r[3 * b], r[3 * b + 1], r[3 * b + 2]);
                }
            }
        }
        __syncthreads();  // rows is written again in the next sweep
    }
}

// phase 0: the keys of d as they are stored; phase 1: the keys of e, computed from them and pair_med.  lh: slots x bins counters of
// this workgroup.  pass 0: one slot and sel is not read.  A pair with n < 3 is passed over as soon as n is known.
__global__ __launch_bounds__(kPairwiseThreads) void pairwise_count_kernel(const uint32_t *__restrict__ keys, int64_t T, int64_t stride, int64_t P,
                                                                         int64_t nseg, int32_t pass, int32_t phase,
                                                                         const ReportSel *__restrict__ sel, const int64_t *__restrict__ pair_n,
                                                                         const double *__restrict__ pair_med, unsigned long long *__restrict__ dst) {
    __shared__ uint32_t lh[2 * kReportBins1];
    const int32_t slots = pass == 0 ? 1 : 2, bins = report_bins(pass), cells = slots * bins;
    const int64_t work = P * nseg;
    for (int64_t wk = blockIdx.x; wk < work; wk += gridDim.x) {
        const int64_t p = wk / nseg, seg = wk - p * nseg;
        if ((pass > 0 || phase > 0) && pair_n[p] < 3) continue;  // (the whole workgroup)
        for (int32_t i = threadIdx.x; i < cells; i += kPairwiseThreads) lh[i] = 0u;
        __syncthreads();
        const int64_t lo = seg * kReportSegFrames, hi = lo + kReportSegFrames < T ? lo + kReportSegFrames : T;
        const uint32_t *row = keys + p * stride;
        const double med = phase > 0 ? pair_med[p] : 0.0;
        const uint32_t prefix0 = pass > 0 ? sel[2 * p].prefix : 0u, prefix1 = pass > 0 ? sel[2 * p + 1].prefix : 0u;
        for (int64_t t = lo + threadIdx.x; t < hi; t += kPairwiseThreads) {
            uint32_t key = row[t];
            if (phase > 0) key = pairwise_dev_key(key, med);
            if (pass == 0) {
                if (report_match(0, key, 0u)) atomicAdd(&lh[report_digit(0, key)], 1u);
            } else {
                const int32_t d = (int32_t)report_digit(pass, key);
                if (report_match(pass, key, prefix0)) atomicAdd(&lh[d], 1u);
                if (report_match(pass, key, prefix1)) atomicAdd(&lh[bins + d], 1u);
            }
        }
        __syncthreads();
        unsigned long long *d = dst + p * cells;
        for (int32_t i = threadIdx.x; i < cells; i += kPairwiseThreads) {
            const uint32_t c = lh[i];
            if (c) atomicAdd(&d[i], (unsigned long long)c);
        }
        __syncthreads();  // lh is zeroed again in the next sweep
    }
}

// bins[0 .. n) of global memory into LDS and the sums of the n / 256 bins of every thread next to them
__device__ __forceinline__ void pairwise_stage_bins(const unsigned long long *__restrict__ src, int n, unsigned long long *bins,
                                                    unsigned long long *part) {
    const int per = n / kPairwiseThreads;
    unsigned long long s = 0;
    for (int j = 0; j < per; ++j) {
        const unsigned long long c = src[threadIdx.x * per + j];
        bins[threadIdx.x * per + j] = c;
        s += c;
    }
    part[threadIdx.x] = s;
    __syncthreads();
}

// report_select in two levels (one thread): over the threads' sums, then over the bins of the thread that holds the rank
__device__ __forceinline__ void pairwise_select_lds(const unsigned long long *bins, int n, const unsigned long long *part, uint64_t rank,
                                                    uint32_t *digit, uint64_t *rank_in) {
    const int per = n / kPairwiseThreads;
    uint32_t i, j;
    uint64_t inside;
    report_select((const uint64_t *)part, kPairwiseThreads, rank, &i, &inside);
    report_select((const uint64_t *)bins + i * per, per, inside, &j, rank_in);
    *digit = i * per + j;
}

// The finishing launch of a pass: a workgroup takes pairs.  pass 0: hist [P][1024] -> n (phase 0: pair_n, and the quiet NaN into
// pair_med and pair_mad where n < 3) and sel of the two ranks; pass 1: hist [P][2][2048] -> 22 bits of prefix; pass 2: hist
// [P][2][1024] -> the two order statistics -> result[p] (phase 0: pair_med, phase 1: pair_mad).
__global__ __launch_bounds__(kPairwiseThreads) void pairwise_finish_kernel(const unsigned long long *__restrict__ hist, int64_t P, int32_t pass,
                                                                          int32_t phase, ReportSel *__restrict__ sel, int64_t *__restrict__ pair_n,
                                                                          double *__restrict__ pair_med, double *__restrict__ pair_mad) {
    __shared__ unsigned long long bins[kReportBins1], part[kPairwiseThreads];
    __shared__ unsigned long long total;
    const int i = threadIdx.x;
    const int nb = report_bins(pass);
    for (int64_t p = blockIdx.x; p < P; p += gridDim.x) {
        if (pass == 0) {
            pairwise_stage_bins(hist + p * nb, nb, bins, part);
            if (i == 0) {
                unsigned long long c = 0;
                for (int j = 0; j < kPairwiseThreads; ++j) c += part[j];
                total = c;
                if (phase == 0) {
                    pair_n[p] = (int64_t)c;
                    if (c < 3) {
                        pair_med[p] = pairwise_nan64();
                        pair_mad[p] = pairwise_nan64();
                    }
                }
            }
            __syncthreads();
            if (i < 2) {
                const unsigned long long n = total;
                ReportSel r;
                r.rank = 0;
                r.prefix = kReportNoKey;
                r.pad = 0u;
                if (n >= 3) pairwise_select_lds(bins, nb, part, i == 0 ? (n - 1) / 2 : n / 2, &r.prefix, &r.rank);
                sel[2 * p + i] = r;
            }
            __syncthreads();  // bins and part are written again in the next sweep
        } else {
            if (pair_n[p] < 3) continue;  // (the whole workgroup; phase 1 counts the same frames)
            uint32_t v0 = 0u, v1 = 0u;  // thread 0's: the bits of the two order statistics
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const ReportSel r = sel[2 * p + q];
                pairwise_stage_bins(hist + (2 * p + q) * nb, nb, bins, part);
                if (i == 0) {
                    uint32_t d;
                    uint64_t rank_in;
                    pairwise_select_lds(bins, nb, part, r.rank, &d, &rank_in);
                    if (pass == 1) {
                        ReportSel o;
                        o.rank = rank_in;
                        o.prefix = (r.prefix << 11) | d;
                        o.pad = 0u;
                        sel[2 * p + q] = o;
                    } else if (q == 0) {
                        v0 = (r.prefix << 10) | d;
                    } else {
                        v1 = (r.prefix << 10) | d;
                    }
                }
                __syncthreads();  // bins and part are written again
            }
            if (pass == 2 && i == 0) (phase == 0 ? pair_med : pair_mad)[p] = pairwise_median(report_float(v0), report_float(v1));
        }
    }
}

// One wavefront per workgroup, one lane per frame of a tile.  dynamic LDS: (K + 1) x 64 words of 64 bits.
__global__ __launch_bounds__(64) void pairwise_decide_kernel(const float *__restrict__ kp, int64_t T, int32_t K, int64_t tiles, int64_t stride,
                                                             const uint32_t *__restrict__ keys, const int64_t *__restrict__ pair_n,
                                                             const double *__restrict__ pair_med, const double *__restrict__ pair_mad,
                                                             double thr, double min_dev, int32_t votes, float *__restrict__ out,
                                                             uint8_t *__restrict__ flag) {
    extern __shared__ unsigned long long words[];
    unsigned long long *m = words + threadIdx.x;                          // word k of this lane's frame: m[k * 64]
    unsigned long long *rej = words + (int64_t)K * kPairwiseTileFrames;  // the reject word of every frame of the tile
    const float nan = report_float(kPairwiseNanBits);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t t0 = tile * kPairwiseTileFrames, t = t0 + threadIdx.x;
        unsigned long long rejected = 0;
        if (t < T) {
            for (int32_t k = 0; k < K; ++k) m[k * kPairwiseTileFrames] = 0ull;
            int64_t p = 0;
            for (int32_t a = 0; a + 1 < K; ++a) {
                unsigned long long wa = m[a * kPairwiseTileFrames];  // (the bits of the partners below a)
                for (int32_t b = a + 1; b < K; ++b, ++p) {
                    if (pair_n[p] < 3) continue;  // (the same for every lane)
                    const uint32_t key = keys[p * stride + t];
                    if (key == kReportNoKey) continue;
                    const double bound = thr * pair_mad[p];
                    if (pairwise_bad(pairwise_dev(report_float(key), pair_med[p]), bound, min_dev)) {
                        wa |= 1ull << b;
                        m[b * kPairwiseTileFrames] |= 1ull << a;
                    }
                }
                m[a * kPairwiseTileFrames] = wa;
            }
            rejected = pairwise_blame((uint64_t *)m, kPairwiseTileFrames, K, votes);
        }
        rej[threadIdx.x] = rejected;
        __syncthreads();
        const int64_t left = T - t0;
        const int32_t nf = left < kPairwiseTileFrames ? (int32_t)left : kPairwiseTileFrames;
        const int64_t base = t0 * K;
        for (int32_t e = threadIdx.x; e < nf * K; e += kPairwiseTileFrames) {  // (frame, keypoint) pairs in the order of memory
            const int32_t f = e / K, k = e - f * K;
            const bool r = (rej[f] >> k) & 1ull;
            const int64_t at = 3 * (base + e);
            const float x = kp[at], y = kp[at + 1], z = kp[at + 2];
            out[at] = r ? nan : x;
            out[at + 1] = r ? nan : y;
            out[at + 2] = r ? nan : z;
            flag[base + e] = r ? 1 : 0;
        }
        __syncthreads();  // rej is written again in the next sweep
    }
}

// One wavefront per workgroup, one lane per frame of a tile.  LDS: the candidate table, the partner and the candidate of every
// keypoint, the decisions of the tile's frames (bit s: candidate s swaps).
__global__ __launch_bounds__(64) void pairwise_swap_kernel(const uint32_t *__restrict__ kp, int64_t T, int32_t K, int32_t S, SwapCands cands,
                                                           int64_t tiles, int64_t stride, const uint32_t *__restrict__ keys,
                                                           const int64_t *__restrict__ pair_n, const double *__restrict__ pair_med,
                                                           const double *__restrict__ pair_mad, double thr, double min_dev, int32_t min_bad,
                                                           uint32_t *__restrict__ out, uint8_t *__restrict__ flag) {
    __shared__ unsigned long long candw[kSwapCandWords];
    __shared__ uint8_t partner[kPairwiseMaxKp], cand_of[kPairwiseMaxKp];
    __shared__ uint32_t dec[kPairwiseTileFrames];
    const int32_t lane = threadIdx.x;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kSwapCandWords; ++i) candw[i] = cands.w[i];  // (compile-time indices: the arguments stay in registers)
    }
    partner[lane] = (uint8_t)lane;
    cand_of[lane] = (uint8_t)kSwapNoCand;
    __syncthreads();
    const uint16_t *c16 = (const uint16_t *)candw;  // candidate s: a | b << 8
    if (lane < S) {
        const uint32_t c = c16[lane], a = c & 0xFFu, b = c >> 8;
        partner[a] = (uint8_t)b;
        partner[b] = (uint8_t)a;
        cand_of[a] = (uint8_t)lane;
        cand_of[b] = (uint8_t)lane;
    }
    __syncthreads();
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t t0 = tile * kPairwiseTileFrames, t = t0 + lane;
        uint32_t mask = 0u;
        if (t < T) {
            for (int32_t s = 0; s < S; ++s) {
                const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)c16[s]);  // (the same for every lane)
                const int32_t a = (int32_t)(c & 0xFFu), b = (int32_t)(c >> 8);
                int32_t b0 = 0, b1 = 0;
                for (int32_t k = 0; k < K; ++k) {
                    if (k == a || k == b) continue;
                    const int64_t pa = swap_pair(a, k, K), pb = swap_pair(b, k, K);
                    const int64_t na = pair_n[pa], nb = pair_n[pb];
                    if (na < 3 || nb < 3) continue;  // (the same for every lane)
                    swap_count(keys[pa * stride + t], keys[pb * stride + t], na, nb, pair_med[pa], thr * pair_mad[pa], pair_med[pb],
                               thr * pair_mad[pb], min_dev, &b0, &b1);
                }
                if (swap_decide(b0, b1, min_bad)) mask |= 1u << s;
            }
        }
        dec[lane] = mask;
        __syncthreads();
        const int64_t left = T - t0;
        const int32_t nf = left < kPairwiseTileFrames ? (int32_t)left : kPairwiseTileFrames;
        const int64_t base = t0 * K;
        for (int32_t e = lane; e < nf * K; e += kPairwiseTileFrames) {  // (frame, keypoint) pairs in the order of memory
            const int32_t f = e / K, k = e - f * K;
            const uint32_t s = cand_of[k];
            const bool swaps = s != kSwapNoCand && ((dec[f] >> s) & 1u);
            const int64_t to = 3 * (base + e), from = swaps ? 3 * (base + (int64_t)f * K + partner[k]) : to;
            const uint32_t x = kp[from], y = kp[from + 1], z = kp[from + 2];
            out[to] = x;
            out[to + 1] = y;
            out[to + 2] = z;
        }
        const int64_t fbase = t0 * S;
        for (int32_t e = lane; e < nf * S; e += kPairwiseTileFrames) {  // (frame, candidate) pairs in the order of memory
            const int32_t f = e / S, s = e - f * S;
            flag[fbase + e] = (uint8_t)((dec[f] >> s) & 1u);
        }
        __syncthreads();  // dec is written again in the next sweep
    }
}

}  // namespace

// The statistics part of both entry points: the keys of every (pair, frame) into the workspace, pair_n, pair_med, pair_mad.  Two memsets
// and 13 launches (nothing for K == 1).
static hipError_t launch_pairwise_stats(const float *kp, int64_t T, int32_t K, const PairwiseLayout &L, int64_t *pair_n, double *pair_med,
                                        double *pair_mad, void *workspace, hipStream_t s) {
    char *w = (char *)workspace;
    uint32_t *keys = (uint32_t *)(w + L.keys);
    unsigned long long *hist[3] = {(unsigned long long *)(w + L.hist0), (unsigned long long *)(w + L.hist1), (unsigned long long *)(w + L.hist2)};
    ReportSel *sel = (ReportSel *)(w + L.sel);
    const int64_t P = L.pairs;
    hipError_t e;
    if (P > 0) {
        const unsigned grid1 = (unsigned)(L.tiles < kPairwiseMaxBlocks ? L.tiles : kPairwiseMaxBlocks);
        hipLaunchKernelGGL(pairwise_dist_kernel, dim3(grid1), dim3(kPairwiseThreads), (size_t)kPairwiseTileFrames * ((3 * K) | 1) * 4, s, kp, T, K,
                           L.tiles, L.stride, keys);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        const int64_t work = P * L.nseg;
        const unsigned gridc = (unsigned)(work < kPairwiseMaxBlocks ? work : kPairwiseMaxBlocks);
        const unsigned gridf = (unsigned)(P < kPairwiseMaxBlocks ? P : kPairwiseMaxBlocks);
        for (int phase = 0; phase < 2; ++phase) {
            if ((e = hipMemsetAsync(hist[0], 0, (size_t)(L.sel - L.hist0), s)) != hipSuccess) return e;
            for (int pass = 0; pass < 3; ++pass) {
                hipLaunchKernelGGL(pairwise_count_kernel, dim3(gridc), dim3(kPairwiseThreads), 0, s, keys, T, L.stride, P, L.nseg, pass, phase, sel,
                                   pair_n, pair_med, hist[pass]);
                if ((e = hipGetLastError()) != hipSuccess) return e;
                hipLaunchKernelGGL(pairwise_finish_kernel, dim3(gridf), dim3(kPairwiseThreads), 0, s, hist[pass], P, pass, phase, sel, pair_n,
                                   pair_med, pair_mad);
                if ((e = hipGetLastError()) != hipSuccess) return e;
            }
        }
    }
    return hipSuccess;
}

static hipError_t launch_pairwise(const float *kp, int64_t T, int32_t K, double thr, double min_dev, int32_t votes, float *out, uint8_t *flag,
                                  int64_t *pair_n, double *pair_med, double *pair_mad, void *workspace, hipStream_t s) {
    const PairwiseLayout L = pairwise_layout(T, K);
    const hipError_t e = launch_pairwise_stats(kp, T, K, L, pair_n, pair_med, pair_mad, workspace, s);
    if (e != hipSuccess) return e;
    const uint32_t *keys = (const uint32_t *)((const char *)workspace + L.keys);
    const unsigned gridd = (unsigned)(L.tiles < kPairwiseMaxWaves ? L.tiles : kPairwiseMaxWaves);
    hipLaunchKernelGGL(pairwise_decide_kernel, dim3(gridd), dim3(kPairwiseTileFrames), (size_t)(K + 1) * kPairwiseTileFrames * 8, s, kp, T, K, L.tiles,
                       L.stride, keys, pair_n, pair_med, pair_mad, thr, min_dev, votes, out, flag);
    return hipGetLastError();
}

static hipError_t launch_swaps(const float *kp, int64_t T, int32_t K, const SwapCands &cands, int32_t S, double thr, double min_dev,
                               int32_t min_bad, float *out, uint8_t *flag, int64_t *pair_n, double *pair_med, double *pair_mad, void *workspace,
                               hipStream_t s) {
    const PairwiseLayout L = pairwise_layout(T, K);
    const hipError_t e = launch_pairwise_stats(kp, T, K, L, pair_n, pair_med, pair_mad, workspace, s);
    if (e != hipSuccess) return e;
    const uint32_t *keys = (const uint32_t *)((const char *)workspace + L.keys);
    const unsigned grid = (unsigned)(L.tiles < kPairwiseMaxWaves ? L.tiles : kPairwiseMaxWaves);
    hipLaunchKernelGGL(pairwise_swap_kernel, dim3(grid), dim3(kPairwiseTileFrames), 0, s, (const uint32_t *)kp, T, K, S, cands, L.tiles, L.stride,
                       keys, pair_n, pair_med, pair_mad, thr, min_dev, min_bad, (uint32_t *)out, flag);
    return hipGetLastError();
}

}  // namespace stac

// ---- C ABI entry points of stac.reject_pairwise (include/stac_hip.h): every argument is checked before the device is touched -----
extern "C" int64_t stac_prep_pairwise_workspace(int64_t n_frames, int32_t n_kp) {
    if (n_frames >= 1 && n_kp > kPairwiseMaxKp)
        return fail(STAC_ERR_CAPACITY, "stac_prep_pairwise_workspace: n_kp = " + std::to_string(n_kp) + " is above the " +
                                           std::to_string(kPairwiseMaxKp) + " keypoints that a frame's words of 64 bits hold");
    const PairwiseLayout L = pairwise_layout(n_frames, n_kp);
    if (L.bytes < 0) return fail(STAC_ERR_INVALID, "stac_prep_pairwise_workspace: n_frames >= 1, n_kp >= 1 (and a workspace size within int64)");
    return L.bytes;
}

// The argument checks that stac_prep_pairwise and stac_prep_swaps share, in the order both make them: sizes, capacity (`holds`: what
// the message says the keypoints are limited by), layout, then `own()`, the entry point's checks of what it alone takes, then thr /
// min_dev, the count (votes / min_bad), null pointers, workspace size, and alignment and overlap of the buffers (flag: flag_cols bytes
// per frame).  STAC_OK, or the status of the first check that fails.
template <class Own>
static int32_t check_pairwise_args(const std::string &fn, const char *holds, const float *kp, int64_t n_frames, int32_t n_kp, double thr,
                                   double min_dev, const char *count_name, int32_t count, const float *out, const uint8_t *flag,
                                   int64_t flag_cols, const int64_t *pair_n, const double *pair_med, const double *pair_mad,
                                   const void *workspace, int64_t workspace_bytes, Own own) {
    if (n_frames < 1 || n_kp < 1) return fail(STAC_ERR_INVALID, fn + ": n_frames >= 1, n_kp >= 1");
    if (n_kp > kPairwiseMaxKp)
        return fail(STAC_ERR_CAPACITY, fn + ": n_kp = " + std::to_string(n_kp) + " is above the " + std::to_string(kPairwiseMaxKp) + " keypoints " +
                                           holds);
    const PairwiseLayout L = pairwise_layout(n_frames, n_kp);
    if (L.bytes < 0) return fail(STAC_ERR_INVALID, fn + ": array sizes beyond int64");
    if (const int32_t rc = own()) return rc;
    if (!std::isfinite(thr) || thr < 0.0 || !std::isfinite(min_dev) || min_dev < 0.0)
        return fail(STAC_ERR_INVALID, fn + ": thr and min_dev must be finite and >= 0");
    if (count < 1) return fail(STAC_ERR_INVALID, fn + ": " + count_name + " = " + std::to_string(count) + " must be >= 1");
    if (!kp || !out || !flag || !pair_n || !pair_med || !pair_mad || !workspace)
        return fail(STAC_ERR_INVALID, fn + ": null kp / out / flag / pair_n / pair_med / pair_mad / workspace");
    if (workspace_bytes < L.bytes)
        return fail(STAC_ERR_INVALID, fn + ": workspace_bytes = " + std::to_string(workspace_bytes) + ", " + std::to_string(L.bytes) +
                                          " are needed (" + fn + "_workspace)");
    const int64_t NK = n_frames * n_kp, P8 = (L.pairs > 0 ? L.pairs : 1) * 8;
    const HostBuf buf[7] = {{"kp", (uintptr_t)kp, NK * 12, 4},
                            {"out", (uintptr_t)out, NK * 12, 4},
                            {"flag", (uintptr_t)flag, n_frames * flag_cols, 1},
                            {"pair_n", (uintptr_t)pair_n, P8, 8},
                            {"pair_med", (uintptr_t)pair_med, P8, 8},
                            {"pair_mad", (uintptr_t)pair_mad, P8, 8},
                            {"workspace", (uintptr_t)workspace, L.bytes, 8}};
    return check_buffers(fn.c_str(), buf, 7, " (in place is not possible)");
}

extern "C" int32_t stac_prep_pairwise(const float *kp, int64_t n_frames, int32_t n_kp, double thr, double min_dev, int32_t votes, float *out,
                                      uint8_t *flag, int64_t *pair_n, double *pair_med, double *pair_mad, void *workspace,
                                      int64_t workspace_bytes, void *stream) {
    if (const int32_t rc = check_pairwise_args("stac_prep_pairwise", "that a frame's words of 64 bits hold", kp, n_frames, n_kp, thr, min_dev,
                                               "votes", votes, out, flag, n_kp, pair_n, pair_med, pair_mad, workspace, workspace_bytes,
                                               [] { return (int32_t)STAC_OK; }))
        return rc;
    return launch_result("stac_prep_pairwise", launch_pairwise(kp, n_frames, n_kp, thr, min_dev, votes, out, flag, pair_n, pair_med, pair_mad,
                                                               workspace, (hipStream_t)stream));
}

// ---- C ABI entry points of stac.repair_swaps (include/stac_hip.h) ----------------------------------------------------------------
extern "C" int64_t stac_prep_swaps_workspace(int64_t n_frames, int32_t n_kp) {
    if (n_frames >= 1 && n_kp > kPairwiseMaxKp)
        return fail(STAC_ERR_CAPACITY, "stac_prep_swaps_workspace: n_kp = " + std::to_string(n_kp) + " is above the " +
                                           std::to_string(kPairwiseMaxKp) + " keypoints of the pairwise statistics");
    const PairwiseLayout L = pairwise_layout(n_frames, n_kp);
    if (L.bytes < 0) return fail(STAC_ERR_INVALID, "stac_prep_swaps_workspace: n_frames >= 1, n_kp >= 1 (and a workspace size within int64)");
    return L.bytes;
}

extern "C" int32_t stac_prep_swaps(const float *kp, int64_t n_frames, int32_t n_kp, const int32_t *cand, int32_t n_cand, double thr,
                                   double min_dev, int32_t min_bad, float *out, uint8_t *flag, int64_t *pair_n, double *pair_med,
                                   double *pair_mad, void *workspace, int64_t workspace_bytes, void *stream) {
    SwapCands cands;
    const auto candidates = [&]() -> int32_t {  // (after the sizes: swap_pack counts on 1 <= n_kp <= kPairwiseMaxKp)
        if (n_cand < 0) return fail(STAC_ERR_INVALID, "stac_prep_swaps: n_cand = " + std::to_string(n_cand) + " must be >= 0");
        if (n_cand > 0 && !cand) return fail(STAC_ERR_INVALID, "stac_prep_swaps: null cand with n_cand > 0");
        int32_t at = 0;
        const int bad = swap_pack(cand, n_cand, n_kp, &cands, &at);  // (cand is host memory)
        if (bad) {
            const char *why[] = {"", "has a keypoint outside 0 .. n_kp - 1", "names one keypoint twice (a == b)",
                                 "has a keypoint that an earlier candidate holds", "is one more than n_kp / 2 candidates can be"};
            return fail(STAC_ERR_INVALID, "stac_prep_swaps: candidate " + std::to_string(at) + " (" + std::to_string(cand[2 * at]) + ", " +
                                              std::to_string(cand[2 * at + 1]) + ") " + why[bad]);
        }
        return STAC_OK;
    };
    if (const int32_t rc = check_pairwise_args("stac_prep_swaps", "of the pairwise statistics", kp, n_frames, n_kp, thr, min_dev, "min_bad",
                                               min_bad, out, flag, n_cand > 0 ? n_cand : 1, pair_n, pair_med, pair_mad, workspace,
                                               workspace_bytes, candidates))
        return rc;
    return launch_result("stac_prep_swaps", launch_swaps(kp, n_frames, n_kp, cands, n_cand, thr, min_dev, min_bad, out, flag, pair_n, pair_med,
                                                         pair_mad, workspace, (hipStream_t)stream));
}
