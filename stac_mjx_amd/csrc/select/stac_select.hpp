// Choosing calibration frames by pose diversity (stac_select.hip).  DESIGN.md "Choosing calibration frames".
//
// The offsets can only be identified from frames in which the joints move.  A frame's DESCRIPTOR is what does not change when the
// animal walks or turns: the P = K (K - 1) / 2 distances between its keypoints, d_p(t) of stac_pairwise.hpp (pairwise_dist; pairs
// (a, b), a < b, in lexicographic order).  The frames are chosen greedily, each the farthest from everything chosen so far:
//   candidate   frame t iff all 3 K coordinates are finite and cand[t] != 0 (cand == NULL: all ones)
//   s_0         the lowest-index candidate; radius2[0] = +inf
//   pick i >= 1 for every candidate t: acc = +0; for p = 0 .. P - 1 in order: e = d_p(t) - d_p(s_{i-1}); acc = acc + e * e;
//               dmin[t] = min(dmin[t], acc) (dmin starts at +inf; select_min);
//               s_i = the candidate with the largest dmin, ties to the lowest index; radius2[i] = that dmin
//   stop        before a pick whose dmin is 0 (every candidate equals an earlier pick), and when there is no candidate
//   outputs     sel[n_select] int64 in selection order, radius2[n_select] float32, n_selected; behind n_selected: -1 and NaN
// Everything is float32 with one rounding per operation (-ffp-contract=off).  dmin >= 0, so its bit pattern orders like its
// value: the maximum with its tie rule is the maximum of the 64-bit KEY bits(dmin) << 32 | (0xFFFFFFFF - t), which limits a
// series to 2^32 - 1 frames; key 0 is nobody's (the low word of a frame's key is >= 1).  Coordinates so large that a distance
// overflows float32 are outside the rule (acc is then NaN and select_min keeps dmin).
//
// What the kernels and the CPU build of tests/select_cases.py share is below; select_reference is the rule on the host.
#pragma once

#include <stdint.h>

#include "../stac_pairwise.hpp"

namespace stac {

constexpr int kSelectMaxKp = kPairwiseMaxKp;          // 2 <= K <= 64: at most 2016 distances per frame
constexpr int kSelectThreads = 256;                   // threads of a workgroup of the update pass and of the pick
constexpr int kSelectMaxBlocks = kPairwiseMaxBlocks;  // workgroups of the update pass at most: the grid strides beyond that
constexpr int kSelectTileFrames = 64;                 // frames of a tile of describe: one wavefront lane per frame
constexpr int kSelectMaxTiles = kPairwiseMaxWaves;    // workgroups of ONE wavefront of describe at most
constexpr int64_t kSelectMaxFrames = 0xFFFFFFFFll;    // 2^32 - 1: the index in the key
constexpr uint32_t kSelectInfBits = 0x7F800000u;
constexpr uint32_t kSelectNanBits = 0x7FC00000u;

STAC_PAIRWISE_HD bool select_candidate(const float *row, int32_t K, uint8_t cand) {
    bool ok = cand != 0;
    for (int32_t j = 0; j < 3 * K; ++j) ok = ok && prep_finite(row[j]);
    return ok;
}

// acc = acc + e * e, e = d - ds: one subtraction, one multiplication, one addition
STAC_PAIRWISE_HD float select_term(float acc, float d, float ds) {
    const float e = d - ds;
    const float ee = e * e;
    return acc + ee;
}

STAC_PAIRWISE_HD float select_min(float dmin, float acc) { return acc < dmin ? acc : dmin; }

STAC_PAIRWISE_HD uint64_t select_key(float dmin, int64_t t) { return (uint64_t)report_bits(dmin) << 32 | (uint64_t)(0xFFFFFFFFu - (uint32_t)t); }
STAC_PAIRWISE_HD int64_t select_key_frame(uint64_t key) { return (int64_t)(0xFFFFFFFFu - (uint32_t)key); }
STAC_PAIRWISE_HD uint32_t select_key_bits(uint64_t key) { return (uint32_t)(key >> 32); }
// Whether pick i ends the selection given the largest key: nobody's key, or (from the second pick on) a dmin of 0
STAC_PAIRWISE_HD bool select_stops(uint64_t key, int64_t i) { return key == 0 || (i >= 1 && select_key_bits(key) == 0); }

// Workspace of stac_select_diverse (byte offsets, all multiples of 8): dist float [P][stride] (d_p(t), one row per pair), dmin
// float [stride], flag uint8 [stride] (1: a candidate), part uint64 [kSelectMaxBlocks] (the largest key of every workgroup of the
// update pass), vec float [P] (the distances of the last pick), state int32 [2] ({done, unused}).  bytes < 0: bad arguments.
struct SelectLayout {
    int64_t pairs, stride, blocks, dist, dmin, flag, part, vec, state, bytes;
};

STAC_PAIRWISE_HD SelectLayout select_layout(int64_t T, int64_t K) {
    SelectLayout L = {0, 0, 0, 0, 0, 0, 0, 0, 0, -1};
    if (T < 1 || T > kSelectMaxFrames || K < 2 || K > kSelectMaxKp) return L;
    L.pairs = pairwise_pairs(K);
    L.stride = ((T - 1) / kSelectTileFrames + 1) * kSelectTileFrames;
    L.blocks = (T - 1) / kSelectThreads + 1;
    if (L.blocks > kSelectMaxBlocks) L.blocks = kSelectMaxBlocks;
    L.dist = 0;
    L.dmin = L.dist + 4 * L.pairs * L.stride;
    L.flag = L.dmin + 4 * L.stride;
    L.part = L.flag + L.stride;
    L.vec = L.part + 8 * kSelectMaxBlocks;
    L.state = L.vec + 8 * ((L.pairs + 1) / 2);
    L.bytes = L.state + 8;
    return L;
}

// The rule on the host.  vec [P], dmin [T] and flag [T] are the caller's scratch (no allocation here).  -> n_selected
inline int64_t select_reference(const float *kp, int64_t T, int32_t K, const uint8_t *cand, int64_t n_select, int64_t *sel, float *radius2,
                                float *vec, float *dmin, uint8_t *flag) {
    const int64_t K3 = 3 * (int64_t)K;
    for (int64_t t = 0; t < T; ++t) {
        flag[t] = select_candidate(kp + t * K3, K, cand ? cand[t] : 1) ? 1 : 0;
        dmin[t] = report_float(kSelectInfBits);
    }
    int64_t n = 0;
    for (int64_t i = 0; i < n_select; ++i) {
        uint64_t best = 0;
        for (int64_t t = 0; t < T; ++t) {
            if (!flag[t]) continue;
            if (i >= 1) {
                const float *r = kp + t * K3;
                float acc = 0.0f;
                int64_t p = 0;
                for (int32_t a = 0; a < K; ++a)
                    for (int32_t b = a + 1; b < K; ++b, ++p)
                        acc = select_term(acc, pairwise_dist(r[3 * a], r[3 * a + 1], r[3 * a + 2], r[3 * b], r[3 * b + 1], r[3 * b + 2]), vec[p]);
                dmin[t] = select_min(dmin[t], acc);
            }
            const uint64_t key = select_key(dmin[t], t);
            if (key > best) best = key;
        }
        if (select_stops(best, i)) break;
        const int64_t s = select_key_frame(best);
        sel[i] = s;
        radius2[i] = report_float(select_key_bits(best));
        n = i + 1;
        const float *r = kp + s * K3;
        int64_t p = 0;
        for (int32_t a = 0; a < K; ++a)
            for (int32_t b = a + 1; b < K; ++b, ++p) vec[p] = pairwise_dist(r[3 * a], r[3 * a + 1], r[3 * a + 2], r[3 * b], r[3 * b + 1], r[3 * b + 2]);
    }
    for (int64_t i = n; i < n_select; ++i) {
        sel[i] = -1;
        radius2[i] = report_float(kSelectNanBits);
    }
    return n;
}

}  // namespace stac
