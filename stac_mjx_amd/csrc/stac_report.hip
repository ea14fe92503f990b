// Fit report: per-keypoint marker errors and exact quantiles (rule and shared functions: stac_report.hpp; entry points: below the kernels).
//
// One call, nine operations on the caller's stream, no copy to the host, no workgroup ever waits for another:
//   0. two memsets: the `hist` output and the histograms of the later passes in the workspace (everything the call adds into)
//   1. report_error_kernel:  reads markers, kp and gap once; writes sqerr, frame_sse, frame_n; leaves, in the workspace, the KEY
//                            of every pair in keypoint-major order (keys [K][stride]: the bits of sqerr, kReportNoKey where the
//                            pair is not counted) and per (keypoint, tile) the sum of e and the packed maximum / argmax
//   2. report_count_kernel (pass 0): keys -> hist[K][1024], bins by bits >> 21
//   3. report_finish0_kernel: per keypoint the tile partials in a fixed order -> sum, max, argmax; hist -> count and, per
//                            quantile, the bin that holds its rank and the rank inside the bin
//   4. report_count_kernel (pass 1): the keys whose top 11 bits equal the chosen bin, by their next 11 bits, per (keypoint, quantile)
//   5. report_finish12_kernel: -> the top 22 bits of every quantile
//   6. report_count_kernel (pass 2): the keys whose top 22 bits match, by their last 10
//   7. report_finish12_kernel: -> quant
// The first pass works on one tile of 64 frames at a time, in chunks of up to 32 keypoints: a thread owns (frame, keypoint) pairs
// in the order of memory, so with K <= 32 a tile is one contiguous block of each input, read in whole lines (rows are 4-byte
// aligned only, hence dword accesses; offsets are 64-bit element offsets).  The pairs' e go to LDS as doubles (-1 = not counted);
// lane f of wavefront 0 then adds frame f's e in ascending keypoint order -- carried in a register over the chunks -- and every
// wavefront takes keypoints of the chunk with a lane per frame: it writes the 64 keys of the keypoint as one 256-byte line of the
// keypoint-major key array and reduces the sum and the maximum over its lanes by a fixed shuffle tree.
// The counting passes read the keys of one keypoint, contiguous, in segments of 8192 frames, into a histogram in LDS that belongs
// to the workgroup (LDS integer atomics), and add its non-empty bins to global memory (64-bit integer atomics: the result does
// not depend on their order).  They read the keys, not sqerr: sqerr is frame-major, and it does not say whether gap was 0.
#include <hip/hip_runtime.h>

#include "stac_host.hpp"
#include "stac_report.hpp"

namespace stac {

namespace {

constexpr int kReportThreads = 256;
constexpr int kReportWaves = kReportThreads / 64;
constexpr int kReportChunk = 32;                 // keypoints of a chunk of the first pass
constexpr int kReportRow = kReportChunk + 1;     // doubles of a frame's row in LDS

static_assert(kReportTileFrames == 64, "a tile is one wavefront lane per frame");
static_assert(kReportBins0 % kReportThreads == 0 && kReportBins1 % kReportThreads == 0 && kReportBins2 % kReportThreads == 0, "bins per thread");

__global__ __launch_bounds__(kReportThreads) void report_error_kernel(const float *__restrict__ markers, const float *__restrict__ kp,
                                                                     const int32_t *__restrict__ gap, int64_t N, int32_t K, int64_t tiles,
                                                                     int64_t stride, float *__restrict__ sqerr, double *__restrict__ frame_sse,
                                                                     int32_t *__restrict__ frame_n, uint32_t *__restrict__ keys,
                                                                     double *__restrict__ psum, unsigned long long *__restrict__ pmax) {
    __shared__ double ed[kReportTileFrames * kReportRow];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t t0 = tile * kReportTileFrames;
        double sse = 0.0;  // of frame t0 + threadIdx.x (threads 0 .. 63)
        int32_t n = 0;
        for (int32_t k0 = 0; k0 < K; k0 += kReportChunk) {
            const int32_t kc = K - k0 < kReportChunk ? K - k0 : kReportChunk;
            for (int32_t e = threadIdx.x; e < kReportTileFrames * kc; e += kReportThreads) {
                const int32_t f = e / kc, k = e - f * kc;
                const int64_t t = t0 + f;
                double v = -1.0;
                if (t < N) {
                    const int64_t at = t * K + (k0 + k);
                    const float *m = markers + 3 * at, *y = kp + 3 * at;
                    const ReportPair p = report_pair(m[0], m[1], m[2], y[0], y[1], y[2], gap ? gap[at] : 0);
                    sqerr[at] = p.sqerr;
                    if (p.counted) v = p.e;
                }
                ed[f * kReportRow + k] = v;
            }
            __syncthreads();
            if (threadIdx.x < kReportTileFrames) {  // frame sums: ascending keypoints, sequentially
                for (int32_t k = 0; k < kc; ++k) {
                    const double v = ed[threadIdx.x * kReportRow + k];
                    if (v >= 0.0) {
                        sse = sse + v;
                        ++n;
                    }
                }
            }
            for (int32_t k = wave; k < kc; k += kReportWaves) {  // keys and tile partials: a lane per frame
                const double v = ed[lane * kReportRow + k];
                const bool counted = v >= 0.0;
                const uint32_t key = counted ? report_bits((float)v) : kReportNoKey;
                if (t0 + lane < N) keys[(int64_t)(k0 + k) * stride + t0 + lane] = key;
                double s = counted ? v : 0.0;
                unsigned long long best = counted ? report_pack(key, lane) : 0ull;
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    s = s + __shfl_xor(s, off);
                    const unsigned long long o = __shfl_xor(best, off);
                    best = o > best ? o : best;
                }
                if (lane == 0) {
                    psum[(int64_t)(k0 + k) * tiles + tile] = s;
                    pmax[(int64_t)(k0 + k) * tiles + tile] = best;
                }
            }
            __syncthreads();  // ed is written again in the next chunk
        }
        if (threadIdx.x < kReportTileFrames && t0 + threadIdx.x < N) {
            frame_sse[t0 + threadIdx.x] = sse;
            frame_n[t0 + threadIdx.x] = n;
        }
    }
}

// lh: slots x bins counters of this workgroup.  pass 0: slots == 1 and sel is not read.
__global__ __launch_bounds__(kReportThreads) void report_count_kernel(const uint32_t *__restrict__ keys, int64_t N, int64_t stride, int32_t K,
                                                                     int64_t nseg, int32_t pass, int32_t slots,
                                                                     const ReportSel *__restrict__ sel, unsigned long long *__restrict__ dst) {
    extern __shared__ uint32_t lh[];
    const int32_t bins = report_bins(pass), cells = slots * bins;
    const int64_t work = (int64_t)K * nseg;
    for (int64_t wk = blockIdx.x; wk < work; wk += gridDim.x) {
        const int64_t k = wk / nseg, seg = wk - k * nseg;
        for (int32_t i = threadIdx.x; i < cells; i += kReportThreads) lh[i] = 0u;
        __syncthreads();
        const int64_t lo = seg * kReportSegFrames, hi = lo + kReportSegFrames < N ? lo + kReportSegFrames : N;
        const uint32_t *row = keys + k * stride;
        const ReportSel *sk = sel + k * slots;
        for (int64_t t = lo + threadIdx.x; t < hi; t += kReportThreads) {
            const uint32_t key = row[t];
            if (pass == 0) {
                if (report_match(0, key, 0u)) atomicAdd(&lh[report_digit(0, key)], 1u);
            } else {
                for (int32_t q = 0; q < slots; ++q)
                    if (report_match(pass, key, sk[q].prefix)) atomicAdd(&lh[q * bins + (int32_t)report_digit(pass, key)], 1u);
            }
        }
        __syncthreads();
        unsigned long long *d = dst + k * cells;
        for (int32_t i = threadIdx.x; i < cells; i += kReportThreads) {
            const uint32_t c = lh[i];
            if (c) atomicAdd(&d[i], (unsigned long long)c);
        }
        __syncthreads();  // lh is zeroed again in the next sweep
    }
}

// bins[0 .. n) of global memory into LDS and the sums of the n / 256 bins of every thread next to them
__device__ __forceinline__ void report_stage_bins(const unsigned long long *__restrict__ src, int n, unsigned long long *bins,
                                                  unsigned long long *part) {
    const int per = n / kReportThreads;
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
__device__ __forceinline__ void report_select_lds(const unsigned long long *bins, int n, const unsigned long long *part, uint64_t rank,
                                                  uint32_t *digit, uint64_t *rank_in) {
    const int per = n / kReportThreads;
    uint32_t i, j;
    uint64_t inside;
    report_select((const uint64_t *)part, kReportThreads, rank, &i, &inside);
    report_select((const uint64_t *)bins + i * per, per, inside, &j, rank_in);
    *digit = i * per + j;
}

// One workgroup per keypoint.  perm_lo / perm_hi: the permille values, 16 bits each (quantiles 0 .. 3 and 4 .. 7).
__global__ __launch_bounds__(kReportThreads) void report_finish0_kernel(const double *__restrict__ psum, const unsigned long long *__restrict__ pmax,
                                                                       int64_t tiles, const unsigned long long *__restrict__ hist, int32_t Q,
                                                                       unsigned long long perm_lo, unsigned long long perm_hi,
                                                                       ReportSel *__restrict__ sel, int64_t *__restrict__ count,
                                                                       double *__restrict__ sum, float *__restrict__ max,
                                                                       int64_t *__restrict__ argmax, float *__restrict__ quant) {
    __shared__ double ss[kReportThreads];
    __shared__ unsigned long long sm[kReportThreads];
    __shared__ long long st[kReportThreads];
    __shared__ unsigned long long bins[kReportBins0], part[kReportThreads];
    __shared__ unsigned long long total;
    const int i = threadIdx.x;
    const int64_t k = blockIdx.x, base = k * tiles;
    // the tile partials: a contiguous segment of tiles per thread, then a tree over the threads -- an order fixed by (N, K)
    const int64_t S = (tiles + kReportThreads - 1) / kReportThreads;
    const int64_t lo = i * S < tiles ? i * S : tiles, hi = lo + S < tiles ? lo + S : tiles;
    double s = 0.0;
    unsigned long long best = 0ull;
    long long best_tile = -1;
    for (int64_t j = lo; j < hi; ++j) {
        s = s + psum[base + j];
        const unsigned long long c = pmax[base + j];
        if (report_tile_wins(best, best_tile, c, j)) {
            best = c;
            best_tile = j;
        }
    }
    ss[i] = s;
    sm[i] = best;
    st[i] = best_tile;
    __syncthreads();
    for (int off = kReportThreads / 2; off >= 1; off >>= 1) {
        if (i < off) {
            ss[i] = ss[i] + ss[i + off];
            if (report_tile_wins(sm[i], st[i], sm[i + off], st[i + off])) {
                sm[i] = sm[i + off];
                st[i] = st[i + off];
            }
        }
        __syncthreads();
    }
    report_stage_bins(hist + k * kReportBins0, kReportBins0, bins, part);
    if (i == 0) {
        unsigned long long c = 0;
        for (int j = 0; j < kReportThreads; ++j) c += part[j];
        total = c;
        count[k] = (int64_t)c;
        sum[k] = ss[0];
        max[k] = report_float(c ? (uint32_t)(sm[0] >> 32) : kReportNanBits);
        argmax[k] = c ? st[0] * kReportTileFrames + (kReportTileFrames - (int64_t)(sm[0] & 0xFFFFFFFFull)) : -1;
    }
    __syncthreads();
    if (i < Q) {
        const int32_t permille = (int32_t)(((i < 4 ? perm_lo : perm_hi) >> (16 * (i & 3))) & 0xFFFFull);
        ReportSel r;
        r.pad = 0u;
        if (total == 0) {
            r.rank = 0;
            r.prefix = kReportNoKey;
            quant[k * Q + i] = report_float(kReportNanBits);
        } else {
            report_select_lds(bins, kReportBins0, part, (uint64_t)report_rank(permille, (int64_t)total), &r.prefix, &r.rank);
        }
        sel[k * Q + i] = r;
    }
}

// One workgroup per (keypoint, quantile).  pass 1: hist of 2048 bins -> 22 bits of prefix; pass 2: 1024 bins -> quant.
__global__ __launch_bounds__(kReportThreads) void report_finish12_kernel(const unsigned long long *__restrict__ hist, int32_t pass,
                                                                        ReportSel *__restrict__ sel, float *__restrict__ quant) {
    __shared__ unsigned long long bins[kReportBins1], part[kReportThreads];
    const int64_t slot = blockIdx.x;
    const ReportSel r = sel[slot];
    if (r.prefix == kReportNoKey) return;  // (the whole workgroup: count == 0)
    const int n = report_bins(pass);
    report_stage_bins(hist + slot * n, n, bins, part);
    if (threadIdx.x == 0) {
        uint32_t d;
        uint64_t rank_in;
        report_select_lds(bins, n, part, r.rank, &d, &rank_in);
        if (pass == 1) {
            ReportSel o;
            o.rank = rank_in;
            o.prefix = (r.prefix << 11) | d;
            o.pad = 0u;
            sel[slot] = o;
        } else {
            quant[slot] = report_float((r.prefix << 10) | d);
        }
    }
}

}  // namespace

static hipError_t launch_report_errors(const float *markers, const float *kp, const int32_t *gap, int64_t N, int32_t K, int32_t Q,
                                const int32_t *permille_host, float *sqerr, double *frame_sse, int32_t *frame_n, int64_t *count, double *sum,
                                float *max, int64_t *argmax, int64_t *hist, float *quant, void *workspace, hipStream_t s) {
    const ReportLayout L = report_layout(N, K, Q);
    char *w = (char *)workspace;
    uint32_t *keys = (uint32_t *)(w + L.keys);
    double *psum = (double *)(w + L.psum);
    unsigned long long *pmax = (unsigned long long *)(w + L.pmax), *hist1 = (unsigned long long *)(w + L.hist1),
                       *hist2 = (unsigned long long *)(w + L.hist2);
    ReportSel *sel = (ReportSel *)(w + L.sel);
    unsigned long long perm[2] = {0ull, 0ull};
    for (int q = 0; q < Q; ++q) perm[q >> 2] |= (unsigned long long)(uint32_t)permille_host[q] << (16 * (q & 3));

    hipError_t e = hipMemsetAsync(hist, 0, (size_t)K * kReportBins0 * 8, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(hist1, 0, (size_t)(L.sel - L.hist1), s);
    if (e != hipSuccess) return e;
    const unsigned grid1 = (unsigned)(L.tiles < kReportMaxBlocks ? L.tiles : kReportMaxBlocks);
    hipLaunchKernelGGL(report_error_kernel, dim3(grid1), dim3(kReportThreads), 0, s, markers, kp, gap, N, K, L.tiles, L.stride, sqerr,
                       frame_sse, frame_n, keys, psum, pmax);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t work = (int64_t)K * L.nseg;
    const unsigned gridc = (unsigned)(work < kReportMaxBlocks ? work : kReportMaxBlocks);
    for (int pass = 0; pass < 3; ++pass) {
        const int32_t slots = pass == 0 ? 1 : Q;
        unsigned long long *dst = pass == 0 ? (unsigned long long *)hist : (pass == 1 ? hist1 : hist2);
        const size_t lds = (size_t)slots * report_bins(pass) * 4;  // <= 8 x 2048 x 4 = 64 KiB
        hipLaunchKernelGGL(report_count_kernel, dim3(gridc), dim3(kReportThreads), lds, s, keys, N, L.stride, K, L.nseg, pass, slots, sel, dst);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (pass == 0)
            hipLaunchKernelGGL(report_finish0_kernel, dim3((unsigned)K), dim3(kReportThreads), 0, s, psum, pmax, L.tiles,
                               (const unsigned long long *)hist, Q, perm[0], perm[1], sel, count, sum, max, argmax, quant);
        else
            hipLaunchKernelGGL(report_finish12_kernel, dim3((unsigned)(K * Q)), dim3(kReportThreads), 0, s, dst, pass, sel, quant);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace stac

// ---- C ABI entry points (include/stac_hip.h): every argument is checked before the device is touched ------------------------------
extern "C" int64_t stac_report_workspace(int64_t n_frames, int32_t n_kp, int32_t n_quant) {
    const ReportLayout L = report_layout(n_frames, n_kp, n_quant);
    if (L.bytes < 0)
        return fail(STAC_ERR_INVALID, "stac_report_workspace: n_frames >= 1, n_kp >= 1, n_quant 1 .. " + std::to_string(kReportMaxQuant) +
                                          " (and a workspace size within int64)");
    return L.bytes;
}

extern "C" int32_t stac_report_errors(const stac_report_params *p) {
    if (!p) return fail(STAC_ERR_INVALID, "stac_report_errors: null parameter struct");
    if (p->n_frames < 1 || p->n_kp < 1) return fail(STAC_ERR_INVALID, "stac_report_errors: n_frames >= 1, n_kp >= 1");
    if (p->n_quant < 1 || p->n_quant > kReportMaxQuant)
        return fail(STAC_ERR_INVALID, "stac_report_errors: n_quant " + std::to_string(p->n_quant) + " is outside 1 .. " +
                                          std::to_string(kReportMaxQuant));
    const ReportLayout L = report_layout(p->n_frames, p->n_kp, p->n_quant);
    if (L.bytes < 0 || p->n_frames > (((int64_t)1 << 58) / p->n_kp))
        return fail(STAC_ERR_INVALID, "stac_report_errors: array sizes beyond int64");
    if (!p->markers || !p->kp || !p->permille || !p->sqerr || !p->frame_sse || !p->frame_n || !p->count || !p->sum || !p->max ||
        !p->argmax || !p->hist || !p->quant || !p->workspace)
        return fail(STAC_ERR_INVALID, "stac_report_errors: null markers / kp / permille / output / workspace (only gap may be null)");
    for (int q = 0; q < p->n_quant; ++q)
        if (p->permille[q] < 0 || p->permille[q] > 1000)
            return fail(STAC_ERR_INVALID, "stac_report_errors: permille[" + std::to_string(q) + "] = " + std::to_string(p->permille[q]) +
                                              " is outside 0 .. 1000");
    if (p->workspace_bytes < L.bytes)
        return fail(STAC_ERR_INVALID, "stac_report_errors: workspace_bytes = " + std::to_string(p->workspace_bytes) + ", " +
                                          std::to_string(L.bytes) + " are needed (stac_report_workspace)");
    const int64_t NK = p->n_frames * p->n_kp, K = p->n_kp, Q = p->n_quant;
    const HostBuf buf[13] = {
        {"markers", (uintptr_t)p->markers, NK * 12, 4}, {"kp", (uintptr_t)p->kp, NK * 12, 4}, {"gap", (uintptr_t)p->gap, p->gap ? NK * 4 : 0, 4},
        {"sqerr", (uintptr_t)p->sqerr, NK * 4, 4}, {"frame_sse", (uintptr_t)p->frame_sse, p->n_frames * 8, 8},
        {"frame_n", (uintptr_t)p->frame_n, p->n_frames * 4, 4}, {"count", (uintptr_t)p->count, K * 8, 8}, {"sum", (uintptr_t)p->sum, K * 8, 8},
        {"max", (uintptr_t)p->max, K * 4, 4}, {"argmax", (uintptr_t)p->argmax, K * 8, 8}, {"hist", (uintptr_t)p->hist, K * kReportBins0 * 8, 8},
        {"quant", (uintptr_t)p->quant, K * Q * 4, 4}, {"workspace", (uintptr_t)p->workspace, L.bytes, 8}};
    if (const int rc = check_buffers("stac_report_errors", buf, 13)) return rc;  // (gap == NULL: zero bytes, overlaps nothing)
    return launch_result("stac_report_errors",
                         launch_report_errors(p->markers, p->kp, p->gap, p->n_frames, p->n_kp, p->n_quant, p->permille, p->sqerr, p->frame_sse,
                                              p->frame_n, p->count, p->sum, p->max, p->argmax, p->hist, p->quant, p->workspace,
                                              (hipStream_t)p->stream));
}
