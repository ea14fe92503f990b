// stac_jpeg.hip -- baseline JPEG encoder for rendered frames (gfx950, wave64): stac_jpeg_encode of include/stac_hip.h.
//
// The restart interval cuts a frame's entropy-coded data into independent, byte-aligned segments; one workgroup codes one
// interval.  Four launches per call (DESIGN.md "JPEG on the GPU"):
//   jpeg_entropy_kernel  one workgroup of 6 wavefronts per interval, one wavefront per 8 x 8 block of the MCU (4 Y, Cb, Cr),
//                        one lane per coefficient: colour conversion, edge replication, chroma downsampling, the integer DCT
//                        (through LDS), quantisation, Huffman codes (a ballot of "nonzero" gives every lane its zero run), a
//                        wavefront prefix sum of code lengths, and the bits of the MCU packed into LDS words, which go to the
//                        interval's staging area un-stuffed; it counts the 0xFF bytes on the way
//   jpeg_tile_sum, jpeg_tile_scan, jpeg_offsets
//                        prefix sum of the interval sizes over the whole call (any number of intervals): where every
//                        interval and every frame starts in the output
//   jpeg_pack_kernel     copies the staged bytes to their place with byte stuffing, adds the header in front of a frame's
//                        first interval and RSTn / EOI behind each; no store at or beyond the output's capacity
#include <hip/hip_runtime.h>

#include "stac_host.hpp"
#include "stac_jpeg.hpp"

namespace stac {
namespace {

constexpr int kEntropyThreads = 384;  // 6 wavefronts
constexpr int kPackThreads = 256;

struct ZigTable {
    uint8_t v[64];
};
constexpr ZigTable make_zig() {
    ZigTable z{};
    for (int k = 0; k < 64; ++k) z.v[k] = kJpegZigzag[k];
    return z;
}
__constant__ ZigTable kZig = make_zig();
// 0: DC luminance, 1: AC luminance, 2: DC chrominance, 3: AC chrominance
__constant__ JpegCodeTable kCodes[4] = {jpeg_code_table(kJpegHuff[0]), jpeg_code_table(kJpegHuff[1]),
                                        jpeg_code_table(kJpegHuff[2]), jpeg_code_table(kJpegHuff[3])};

struct JpegQuantArg {
    uint8_t q[2][64];
};

__device__ __forceinline__ int descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }

// One pass of the Loeffler-Ligtenberg-Moshovitz integer DCT (CONST_BITS 13, PASS1_BITS 2) over 8 values `stride` apart, in
// place.  Modular 32-bit arithmetic: every result fits, intermediate sums may wrap.
template <bool ROWS>
__device__ __forceinline__ void dct_pass(int *p, int stride) {
    const uint32_t d0 = p[0], d1 = p[stride], d2 = p[2 * stride], d3 = p[3 * stride], d4 = p[4 * stride], d5 = p[5 * stride],
                   d6 = p[6 * stride], d7 = p[7 * stride];
    const uint32_t t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = ROWS ? 11 : 15;
    int o0, o4;
    if (ROWS) {
        o0 = (int32_t)((t10 + t11) << 2);
        o4 = (int32_t)((t10 - t11) << 2);
    } else {
        o0 = descale(t10 + t11, 2);
        o4 = descale(t10 - t11, 2);
    }
    uint32_t z1 = (t12 + t13) * 4433u;
    const int o2 = descale(z1 + t13 * 6270u, n), o6 = descale(z1 - t12 * 15137u, n);
    z1 = t4 + t7;
    uint32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const uint32_t z5 = (z3 + z4) * 9633u;
    const uint32_t u4 = t4 * 2446u, u5 = t5 * 16819u, u6 = t6 * 25172u, u7 = t7 * 12299u;
    z1 = 0u - z1 * 7373u;
    z2 = 0u - z2 * 20995u;
    z3 = 0u - z3 * 16069u + z5;
    z4 = 0u - z4 * 3196u + z5;
    p[0] = o0;
    p[stride] = descale(u7 + z1 + z4, n);
    p[2 * stride] = o2;
    p[3 * stride] = descale(u6 + z2 + z3, n);
    p[4 * stride] = o4;
    p[5 * stride] = descale(u5 + z2 + z4, n);
    p[6 * stride] = o6;
    p[7 * stride] = descale(u4 + z1 + z3, n);
}

__device__ __forceinline__ uint32_t count_ff(uint32_t w) {
    return (uint32_t)((w & 0xFFu) == 0xFFu) + (uint32_t)((w & 0xFF00u) == 0xFF00u) + (uint32_t)((w & 0xFF0000u) == 0xFF0000u) +
           (uint32_t)((w & 0xFF000000u) == 0xFF000000u);
}

__device__ __forceinline__ void load_rgb(const uint8_t *rgb, size_t px, int &R, int &G, int &B) {
    R = rgb[3 * px];
    G = rgb[3 * px + 1];
    B = rgb[3 * px + 2];
}

__global__ __launch_bounds__(kEntropyThreads) void jpeg_entropy_kernel(const JpegCall C, const JpegQuantArg Q, const int hdr_len) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    __shared__ uint32_t s_tab[2][256 + 16];  // per table class: AC codes by symbol, then DC codes by category
    __shared__ int s_blk[6][64];
    __shared__ uint32_t s_bits[kJpegMcuWords];
    __shared__ int s_dc[6], s_dummy[6], s_nbits[6], s_pred[3];
    __shared__ uint32_t s_ff[6];  // 0xFF bytes staged by each wavefront

    for (int k = tid; k < 512; k += kEntropyThreads) s_tab[k >> 8][k & 255] = kCodes[(k >> 8) * 2 + 1].e[k & 255];
    if (tid < 32) s_tab[tid >> 4][256 + (tid & 15)] = kCodes[(tid >> 4) * 2].e[tid & 15];

    const int comp = w < 4 ? 0 : w - 3, tc = comp > 0 ? 1 : 0;
    const int qd = 8 * (int)Q.q[tc][lane];
    const int nat = kZig.v[lane];
    const int r = lane >> 3, c = lane & 7;
    const int W = C.W, H = C.H;
    const int yw = (W + 7) >> 3, yh = (H + 7) >> 3;
    const int cw = (((W + 1) >> 1) + 7) >> 3, ch = (((H + 1) >> 1) + 7) >> 3, hc = (H + 1) >> 1;
    const int64_t M = (int64_t)C.mw * C.mh;
    const uint32_t *ac = s_tab[tc], *dc = s_tab[tc] + 256;

    for (int64_t i = blockIdx.x; i < C.T; i += gridDim.x) {
        const int64_t f = i / C.nint;
        const int j = (int)(i - f * C.nint);
        const int64_t m0 = (int64_t)j * C.R, m1 = m0 + C.R < M ? m0 + C.R : M;
        const uint8_t *rgb = C.rgb + (size_t)f * H * W * 3;
        uint32_t *stage = C.stage + i * C.stride_words;
        __syncthreads();  // the previous interval is done with the shared state
        for (int t = tid; t < kJpegMcuWords; t += kEntropyThreads) s_bits[t] = 0;
        if (tid < 3) s_pred[tid] = 0;
        uint32_t ff = 0;
        int cb = 0;         // bits carried in s_bits[0]
        int64_t wbase = 0;  // words already staged
        __syncthreads();
        for (int64_t m = m0; m < m1; ++m) {
            const int my = (int)(m / C.mw), mx = (int)(m - (int64_t)my * C.mw);
            // samples (level-shifted); a dummy block (beyond the component's real blocks) is not transformed
            bool dummy;
            int sample = 0;
            if (comp == 0) {
                const int X = 2 * mx + (w & 1), Yb = 2 * my + (w >> 1);
                dummy = X >= yw || Yb >= yh;
                if (!dummy) {
                    const int px = min(X * 8 + c, W - 1), py = min(Yb * 8 + r, H - 1);
                    int R, G, B;
                    load_rgb(rgb, (size_t)py * W + px, R, G, B);
                    sample = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
                }
            } else {
                dummy = mx >= cw || my >= ch;
                if (!dummy) {
                    const int cx = mx * 8 + c, cy = min(my * 8 + r, hc - 1);
                    const int x0 = min(2 * cx, W - 1), x1 = min(2 * cx + 1, W - 1), y0 = 2 * cy, y1 = min(2 * cy + 1, H - 1);
                    int sum = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        int R, G, B;
                        load_rgb(rgb, (size_t)((k & 2) ? y1 : y0) * W + ((k & 1) ? x1 : x0), R, G, B);
                        sum += comp == 1 ? (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
                                         : (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
                    }
                    sample = ((sum + 1 + (cx & 1)) >> 2) - 128;
                }
            }
            s_blk[w][lane] = sample;
            __syncthreads();
            if (lane < 8 && !dummy) dct_pass<true>(&s_blk[w][lane * 8], 1);
            __syncthreads();
            if (lane < 8 && !dummy) dct_pass<false>(&s_blk[w][lane], 8);
            __syncthreads();
            int v = 0;
            if (!dummy) {
                const int cc = s_blk[w][nat];
                const int t = abs(cc) + (qd >> 1);
                const int qv = t >= qd ? t / qd : 0;
                v = cc < 0 ? -qv : qv;
            }
            if (lane == 0) {
                s_dc[w] = v;
                s_dummy[w] = dummy ? 1 : 0;
            }
            __syncthreads();
            // DC prediction: the last real block of the component before this one (0 at the start of an interval)
            int val = v;
            if (lane == 0) {
                int pred = s_pred[comp];
                if (comp == 0) {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        if (k < w && !s_dummy[k]) pred = s_dc[k];
                }
                val = dummy ? 0 : v - pred;
            }
            const unsigned long long nzmask = __ballot(lane > 0 && v != 0);
            uint64_t bits = 0;
            int n = 0;
            const int a = abs(val);
            const int s = a ? 32 - __clz(a) : 0;
            const uint32_t vb = (uint32_t)(val < 0 ? val - 1 : val) & ((1u << s) - 1u);
            if (lane == 0) {
                const uint32_t e = dc[s];
                bits = ((uint64_t)(e >> 8) << s) | vb;
                n = (int)(e & 255u) + s;
            } else if (val != 0) {
                const unsigned long long prev = nzmask & ((1ull << lane) - 1ull);
                const int run = prev ? lane - 1 - (63 - __clzll((long long)prev)) : lane - 1;
                const uint32_t zrl = ac[0xF0];
                for (int z = run >> 4; z > 0; --z) {
                    bits = (bits << (zrl & 255u)) | (zrl >> 8);
                    n += (int)(zrl & 255u);
                }
                const uint32_t e = ac[((run & 15) << 4) | s];
                bits = (((bits << (e & 255u)) | (e >> 8)) << s) | vb;
                n += (int)(e & 255u) + s;
            } else if (lane == 63) {
                const uint32_t e = ac[0];  // EOB
                bits = e >> 8;
                n = (int)(e & 255u);
            }
            int incl = n;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            if (lane == 63) s_nbits[w] = incl;
            __syncthreads();
            int base = cb, tb = cb;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int nb = s_nbits[k];
                if (k < w) base += nb;
                tb += nb;
            }
            if (n > 0) {
                const int p = base + incl - n, wi = p >> 5, sh = p & 31;
                const uint64_t L = bits << (64 - n);  // left-aligned
                const uint64_t hi = L >> sh;
                const uint32_t w0 = (uint32_t)(hi >> 32), w1 = (uint32_t)hi, w2 = sh ? (uint32_t)((L << (64 - sh)) >> 32) : 0u;
                if (w0) atomicOr(&s_bits[wi], w0);
                if (w1) atomicOr(&s_bits[wi + 1], w1);
                if (w2) atomicOr(&s_bits[wi + 2], w2);
            }
            if (tid == 0) {
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    if (!s_dummy[k]) s_pred[k < 4 ? 0 : k - 3] = s_dc[k];
            }
            __syncthreads();
            const int nfull = tb >> 5;
            const uint32_t carry = s_bits[nfull];
            if (tid < nfull) {
                const uint32_t word = s_bits[tid];
                stage[wbase + tid] = __builtin_bswap32(word);
                ff += count_ff(word);
            }
            __syncthreads();
            if (tid == 0) s_bits[0] = carry;
            else if (tid <= nfull) s_bits[tid] = 0;
            wbase += nfull;
            cb = tb & 31;
            __syncthreads();
        }
        int tail = 0;
        if (tid == 0 && cb > 0) {  // pad the last byte with 1-bits
            tail = (cb + 7) >> 3;
            const int pad = tail * 8 - cb;
            const uint32_t word = s_bits[0] | (((1u << pad) - 1u) << (32 - cb - pad));
            stage[wbase] = __builtin_bswap32(word);
            const uint32_t valid = tail < 4 ? ~(0xFFFFFFFFu >> (8 * tail)) : 0xFFFFFFFFu;
            ff += count_ff(word & valid);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) ff += __shfl_xor(ff, d);
        if (lane == 0) s_ff[w] = ff;
        __syncthreads();
        if (tid == 0) {
            const int64_t len = wbase * 4 + tail;
            C.ilen[i] = (uint32_t)len;
            // stuffed data, then RSTn or EOI; the header goes in front of a frame's first interval
            C.isize[i] = len + (int64_t)(s_ff[0] + s_ff[1] + s_ff[2] + s_ff[3] + s_ff[4] + s_ff[5]) + 2 + (j == 0 ? hdr_len : 0);
        }
    }
}

// ---- prefix sum of the interval sizes -----------------------------------------------------------------------------------
// inclusive sum over the 256 threads of a workgroup; *total: the sum of all
__device__ __forceinline__ int64_t block_scan(int64_t v, int64_t *s_wave, int64_t *total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    __syncthreads();  // s_wave may still be read from a previous call
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    int64_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t t = s_wave[k];
        if (k < wv) before += t;
        all += t;
    }
    *total = all;
    return incl + before;
}

__global__ __launch_bounds__(kPackThreads) void jpeg_tile_sum(const JpegCall C, const int64_t ntile) {
    __shared__ int64_t s_wave[4];
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t i0 = tile * kJpegScanTile + 4 * (int64_t)threadIdx.x;
        int64_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k < C.T) v += C.isize[i0 + k];
        int64_t total;
        block_scan(v, s_wave, &total);
        if (threadIdx.x == 0) C.tile_sum[tile] = total;
    }
}

__global__ __launch_bounds__(kPackThreads) void jpeg_tile_scan(const JpegCall C, const int64_t ntile) {
    __shared__ int64_t s_wave[4];
    int64_t carry = 0;
    for (int64_t t0 = 0; t0 < ntile; t0 += kPackThreads) {
        const int64_t t = t0 + threadIdx.x;
        const int64_t v = t < ntile ? C.tile_sum[t] : 0;
        int64_t total;
        const int64_t incl = block_scan(v, s_wave, &total);
        if (t < ntile) C.tile_off[t] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) C.frame_offset[C.N] = carry;
}

__global__ __launch_bounds__(kPackThreads) void jpeg_offsets(const JpegCall C, const int64_t ntile) {
    __shared__ int64_t s_wave[4];
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t i0 = tile * kJpegScanTile + 4 * (int64_t)threadIdx.x;
        int64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        if (i0 < C.T) a0 = C.isize[i0];
        if (i0 + 1 < C.T) a1 = C.isize[i0 + 1];
        if (i0 + 2 < C.T) a2 = C.isize[i0 + 2];
        if (i0 + 3 < C.T) a3 = C.isize[i0 + 3];
        int64_t total;
        const int64_t incl = block_scan(a0 + a1 + a2 + a3, s_wave, &total);
        int64_t o = C.tile_off[tile] + incl - (a0 + a1 + a2 + a3);
        const int64_t add[4] = {a0, a1, a2, a3};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = i0 + k;
            if (i < C.T) {
                C.ioff[i] = o;
                if (i % C.nint == 0) C.frame_offset[i / C.nint] = o;
            }
            o += add[k];
        }
    }
}

// ---- byte stuffing and compaction ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPackThreads) void jpeg_pack_kernel(const JpegCall C, const JpegHeader Hd) {
    __shared__ int s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint8_t *const out = C.out;
    const int64_t cap = C.cap;
    for (int64_t i = blockIdx.x; i < C.T; i += gridDim.x) {
        const int j = (int)(i % C.nint);
        int64_t off = C.ioff[i];
        const int64_t len = C.ilen[i];
        if (j == 0) {
            for (int t = tid; t < Hd.len; t += kPackThreads)
                if (off + t < cap) out[off + t] = Hd.bytes[t];
            off += Hd.len;
        }
        const uint32_t *src = C.stage + i * C.stride_words;
        for (int64_t base = 0; base < len; base += 4 * kPackThreads) {
            const int64_t at = base + 4 * tid;
            const int nvalid = at >= len ? 0 : (len - at < 4 ? (int)(len - at) : 4);
            const uint32_t word = nvalid ? src[at >> 2] : 0u;  // byte k of the stream in bits 8k .. 8k+7
            const uint32_t b0 = word & 255u, b1 = (word >> 8) & 255u, b2 = (word >> 16) & 255u, b3 = word >> 24;
            const int cnt = nvalid + (nvalid > 0 && b0 == 255u) + (nvalid > 1 && b1 == 255u) + (nvalid > 2 && b2 == 255u) +
                            (nvalid > 3 && b3 == 255u);
            int incl = cnt;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            if (lane == 63) s_wave[wv] = incl;
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = s_wave[k];
                if (k < wv) before += t;
                total += t;
            }
            int64_t p = off + before + incl - cnt;
#define STAC_JPEG_PUT(k, b)                      \
    if (nvalid > k) {                            \
        if (p < cap) out[p] = (uint8_t)(b);      \
        ++p;                                     \
        if ((b) == 255u) {                       \
            if (p < cap) out[p] = 0;             \
            ++p;                                 \
        }                                        \
    }
            STAC_JPEG_PUT(0, b0)
            STAC_JPEG_PUT(1, b1)
            STAC_JPEG_PUT(2, b2)
            STAC_JPEG_PUT(3, b3)
#undef STAC_JPEG_PUT
            off += total;
            __syncthreads();  // s_wave is written again in the next round
        }
        if (tid == 0) {
            if (off < cap) out[off] = 0xFF;
            if (off + 1 < cap) out[off + 1] = (uint8_t)(j == C.nint - 1 ? 0xD9 : 0xD0 + (j & 7));
        }
    }
}

}  // namespace

static hipError_t launch_jpeg_encode(const JpegCall &C, const JpegHeader &Hd, hipStream_t s) {
    if (C.T <= 0) return hipSuccess;
    JpegQuantArg Q;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) Q.q[t][k] = Hd.quant[t][k];
    const int64_t ntile = (C.T + kJpegScanTile - 1) / kJpegScanTile;
    const unsigned grid = (unsigned)(C.T < (1 << 20) ? C.T : (1 << 20));
    const unsigned tgrid = (unsigned)(ntile < 65535 ? ntile : 65535);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(grid), dim3(kEntropyThreads), 0, s, C, Q, (int)Hd.len);
    hipLaunchKernelGGL(jpeg_tile_sum, dim3(tgrid), dim3(kPackThreads), 0, s, C, ntile);
    hipLaunchKernelGGL(jpeg_tile_scan, dim3(1), dim3(kPackThreads), 0, s, C, ntile);
    hipLaunchKernelGGL(jpeg_offsets, dim3(tgrid), dim3(kPackThreads), 0, s, C, ntile);
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3(grid), dim3(kPackThreads), 0, s, C, Hd);
    return hipGetLastError();
}

}  // namespace stac

// ---- C ABI entry points (include/stac_hip.h) ---------------------------------------------------------------------------------------
static bool jpeg_shape_ok(int64_t N, int32_t width, int32_t height, int32_t restart_mcus, int min_restart) {
    return N >= 0 && width >= 1 && height >= 1 && width <= kJpegMaxDim && height <= kJpegMaxDim && restart_mcus >= min_restart &&
           restart_mcus <= 65535;
}

extern "C" int64_t stac_jpeg_header(int32_t width, int32_t height, int32_t quality, int32_t restart_mcus, uint8_t *buf,
                                    int64_t capacity) {
    if (!jpeg_shape_ok(0, width, height, restart_mcus, 0) || quality < 1 || quality > 100 || capacity < 0)
        return fail(STAC_ERR_INVALID, "stac_jpeg_header: width / height 1..65535, quality 1..100, restart_mcus 0..65535");
    JpegHeader h;
    jpeg_make_header(width, height, quality, restart_mcus, &h);
    if (buf) {
        if (capacity < h.len) return fail(STAC_ERR_INVALID, "stac_jpeg_header: buffer smaller than the header");
        memcpy(buf, h.bytes, (size_t)h.len);
    }
    return h.len;
}

extern "C" int64_t stac_jpeg_workspace_bytes(int64_t N, int32_t width, int32_t height, int32_t restart_mcus) {
    if (!jpeg_shape_ok(N, width, height, restart_mcus, 1))
        return fail(STAC_ERR_INVALID, "stac_jpeg_workspace_bytes: N >= 0, width / height 1..65535, restart_mcus 1..65535");
    JpegCall c{};
    c.N = N; c.W = width; c.H = height; c.R = restart_mcus;
    const int64_t per_frame = (int64_t)((width + 15) / 16) * ((height + 15) / 16) * (kJpegMcuBitsMax / 8 + 64);
    if (N > 0 && per_frame > (INT64_MAX >> 4) / N) return fail(STAC_ERR_CAPACITY, "stac_jpeg_workspace_bytes: N x width x height too large");
    return jpeg_layout(&c, nullptr);
}

extern "C" int32_t stac_jpeg_encode(int64_t N, int32_t width, int32_t height, int32_t quality, int32_t restart_mcus,
                                    const uint8_t *rgb, uint8_t *out, int64_t out_capacity, int64_t *frame_offset,
                                    void *workspace, int64_t workspace_bytes, void *stream) {
    if (!jpeg_shape_ok(N, width, height, restart_mcus, 1) || quality < 1 || quality > 100)
        return fail(STAC_ERR_INVALID, "stac_jpeg_encode: N >= 0, width / height 1..65535, quality 1..100, restart_mcus 1..65535");
    if (N == 0) return STAC_OK;
    if (!rgb || !frame_offset || out_capacity < 0 || (out_capacity > 0 && !out) || !workspace || ((uintptr_t)workspace & 7))
        return fail(STAC_ERR_INVALID, "stac_jpeg_encode: null rgb / out / frame_offset / workspace, or workspace not 8-byte aligned");
    const int64_t need = stac_jpeg_workspace_bytes(N, width, height, restart_mcus);
    if (need < 0) return (int32_t)need;
    if (workspace_bytes < need)
        return fail(STAC_ERR_INVALID, "stac_jpeg_encode: workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                          std::to_string(need) + " needed (stac_jpeg_workspace_bytes)");
    JpegCall c{};
    c.N = N; c.W = width; c.H = height; c.R = restart_mcus;
    jpeg_layout(&c, (uint8_t *)workspace);
    c.rgb = rgb; c.out = out; c.cap = out_capacity; c.frame_offset = frame_offset;
    JpegHeader h;
    jpeg_make_header(width, height, quality, restart_mcus, &h);
    return launch_result("stac_jpeg_encode", launch_jpeg_encode(c, h, (hipStream_t)stream));
}
