// Shared tables and layout of the JPEG encoder (stac_jpeg.hip) and its host entry points (below the kernels).
//
// The stream is baseline sequential JPEG as libjpeg writes it (DESIGN.md "JPEG on the GPU"): 8 bit, YCbCr 4:2:0, one
// interleaved scan, the Annex K quantisation and Huffman tables, restart interval counted in MCUs of 16 x 16 pixels.
#pragma once

#include <stdint.h>

namespace stac {

// Annex K base quantisation tables, in zigzag order (the order of a DQT segment and of a coded block).
constexpr uint8_t kJpegBaseQuant[2][64] = {
    {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99},
    {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// zigzag position -> index in the 8 x 8 block (row * 8 + column)
constexpr uint8_t kJpegZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K Huffman tables as a DHT segment carries them: 16 code-length counts, then the symbols in code order.
struct JpegHuffSpec {
    uint8_t bits[16];
    int nvals;
    uint8_t vals[162];
};

constexpr JpegHuffSpec kJpegHuff[4] = {
    // DC luminance
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    // AC luminance
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, 162,
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
      0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
      0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
      0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
      0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
      0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
      0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}},
    // DC chrominance
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    // AC chrominance
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}, 162,
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
      0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
      0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
      0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
      0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
      0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
      0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}},
};

// symbol -> (code << 8) | length of one table; 0 = the table has no code for the symbol
struct JpegCodeTable {
    uint32_t e[256];
};

constexpr JpegCodeTable jpeg_code_table(const JpegHuffSpec &s) {
    JpegCodeTable t{};
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < s.bits[l - 1]; ++i) {
            t.e[s.vals[k]] = (code << 8) | (uint32_t)l;
            ++k;
            ++code;
        }
        code <<= 1;
    }
    return t;
}

constexpr int kJpegHeaderMax = 640;       // SOI .. SOS with a DRI segment: 629 bytes
constexpr int kJpegBlockBitsMax = 1660;   // one coded block: DC 11 + 11 bits, 63 AC coefficients of 16 + 10 bits
constexpr int kJpegMcuBitsMax = 6 * kJpegBlockBitsMax;
constexpr int kJpegMcuWords = 320;        // LDS bit buffer of one MCU: 31 carried bits + kJpegMcuBitsMax, two words of slack
constexpr int kJpegScanTile = 1024;       // intervals per workgroup of the size prefix sum
constexpr int kJpegMaxDim = 65535;

// Everything up to and including SOS, and the scaled quantisation tables (zigzag order): a kernel argument by value.
struct JpegHeader {
    uint8_t bytes[kJpegHeaderMax];
    uint8_t quant[2][64];
    int32_t len;
};

inline void jpeg_quant_tables(int quality, uint8_t q[2][64]) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) {
            int v = (kJpegBaseQuant[t][k] * s + 50) / 100;
            q[t][k] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
}

// restart_mcus == 0: no DRI segment
inline void jpeg_make_header(int W, int H, int quality, int restart_mcus, JpegHeader *h) {
    jpeg_quant_tables(quality, h->quant);
    uint8_t *b = h->bytes;
    int n = 0;
    auto put = [&](int v) { b[n++] = (uint8_t)v; };
    auto put2 = [&](int v) { put(v >> 8); put(v & 255); };
    put2(0xFFD8);
    put2(0xFFE0); put2(16);
    for (int v : {0x4A, 0x46, 0x49, 0x46, 0x00, 1, 1, 0, 0, 1, 0, 1, 0, 0}) put(v);
    for (int t = 0; t < 2; ++t) {
        put2(0xFFDB); put2(67); put(t);
        for (int k = 0; k < 64; ++k) put(h->quant[t][k]);
    }
    put2(0xFFC0); put2(17); put(8); put2(H); put2(W); put(3);
    for (int v : {1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1}) put(v);
    const int cls[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; ++t) {
        const JpegHuffSpec &s = kJpegHuff[t];
        put2(0xFFC4); put2(19 + s.nvals); put(cls[t]);
        for (int i = 0; i < 16; ++i) put(s.bits[i]);
        for (int i = 0; i < s.nvals; ++i) put(s.vals[i]);
    }
    if (restart_mcus > 0) { put2(0xFFDD); put2(4); put2(restart_mcus); }
    put2(0xFFDA); put2(12);
    for (int v : {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0}) put(v);
    h->len = n;
}

struct JpegCall {
    int64_t N;
    int32_t W, H, R;           // R: restart interval in MCUs
    int32_t mw, mh;            // MCUs per row / column
    int32_t nint;              // intervals per frame
    int64_t T;                 // N * nint
    int64_t stride_words;      // staging words per interval
    const uint8_t *rgb;
    uint8_t *out;
    int64_t cap;
    int64_t *frame_offset;
    // workspace
    uint32_t *stage;           // [T, stride_words] unstuffed entropy bytes of every interval
    uint32_t *ilen;            // [T] unstuffed bytes
    int64_t *isize;            // [T] bytes the interval adds to its file (stuffed data, marker, header, EOI)
    int64_t *ioff;             // [T] where they start in `out`
    int64_t *tile_sum;         // [ceil(T / kJpegScanTile)]
    int64_t *tile_off;
};

inline int64_t jpeg_stride_words(int W, int H, int R) {
    const int64_t M = (int64_t)((W + 15) / 16) * ((H + 15) / 16);
    const int64_t r = R < M ? R : M;
    return (r * kJpegMcuBitsMax + 31) / 32 + 2;
}

inline int64_t jpeg_align(int64_t v) { return (v + 255) & ~(int64_t)255; }

// Fills the workspace pointers of `c` (N, W, H, R set) from `base`; returns the bytes needed.
inline int64_t jpeg_layout(JpegCall *c, uint8_t *base) {
    c->mw = (c->W + 15) / 16;
    c->mh = (c->H + 15) / 16;
    const int64_t M = (int64_t)c->mw * c->mh;
    c->nint = (int32_t)((M + c->R - 1) / c->R);
    c->T = c->N * c->nint;
    c->stride_words = jpeg_stride_words(c->W, c->H, c->R);
    const int64_t ntile = (c->T + kJpegScanTile - 1) / kJpegScanTile;
    int64_t o = 0;
    c->stage = (uint32_t *)(base + o); o += jpeg_align(c->T * c->stride_words * 4);
    c->ilen = (uint32_t *)(base + o);  o += jpeg_align(c->T * 4);
    c->isize = (int64_t *)(base + o);  o += jpeg_align(c->T * 8);
    c->ioff = (int64_t *)(base + o);   o += jpeg_align(c->T * 8);
    c->tile_sum = (int64_t *)(base + o); o += jpeg_align(ntile * 8);
    c->tile_off = (int64_t *)(base + o); o += jpeg_align(ntile * 8);
    return o;
}

}  // namespace stac
