// Ground clearance of fitted poses (stac_ground.hip).  DESIGN.md "Ground clearance".
//
// xpos [N][nbody][3] and xquat [N][nbody][4] (w, x, y, z) are the body frames of N fitted poses.  A GEOM TABLE of G rows says what
// hangs on the bodies: per geom g the six integers
//   type (kGroundSphere 2, kGroundCapsule 3, kGroundEllipsoid 4, kGroundCylinder 5, kGroundBox 6, kGroundMesh 7: mjtGeom),
//   body (1 .. nbody - 1), include (0 / 1), slot (-1, or 0 .. S - 1), vert_first, vert_count (a mesh's range into verts [V][3], its
//   vertices in the geom frame)
// and the fifteen floats size[3], pos[3], R[3][3] (the geom's frame in its body's: R is the rotation matrix of geom_quat, computed in
// float64 and rounded once).  Only the world z of things is needed.  Per frame t and geom g, with (w, x, y, z) = xquat[t][body]:
//   bz0 = 2 (x z - w y), bz1 = 2 (y z + w x), bz2 = 1 - 2 (x x + y y)          the z row of the body's rotation
//   cz  = xpos[t][body][2] + ((bz0 pos0 + bz1 pos1) + bz2 pos2)                the geom's centre
//   r_j = (bz0 R[0][j] + bz1 R[1][j]) + bz2 R[2][j]                            world z in the geom's axes
//   sphere h = s0; capsule h = s0 + |r2| s1; ellipsoid h = sqrt(((r0 s0)^2 + (r1 s1)^2) + (r2 s2)^2);
//   cylinder h = |r2| s1 + s0 sqrt(r0^2 + r1^2); box h = (|r0| s0 + |r1| s1) + |r2| s2;       z_g = cz - h
//   mesh z_g = cz + min_v ((r0 v0 + r1 v1) + r2 v2)
// Everything is float32 with one rounding per operation (-ffp-contract=off) and a correctly rounded square root.
// A MINIMUM here is the minimum of the finite values in the order of ground_key: the order of the floats, with -0 below +0, so that
// it has no order of evaluation and its bits do not depend on how it is reduced.
//   low_z [N], low_geom [N]      the smallest z_g over the geoms with include = 1 and the smallest g that attains it (the same bits);
//                                +inf and -1 without such a geom
//   track_z [N][S]               the smallest z_g over the geoms of each slot, included or not; +inf for a slot without geoms
//   geom_min [G]                 the smallest z_g of the geom over the frames; +inf without a finite one
//   geom_below [G] (int64)       the number of frames with z_g < z_ref
// A z_g that is not finite (NaN, +-inf) makes low_z of its frame the quiet NaN 0x7FC00000 and low_geom -1 if the geom is included,
// makes its slot's track_z of the frame that NaN if it has a slot, and is skipped in geom_min and geom_below.  Nothing else of the
// frame is touched.
//
// What the kernel and the CPU build of tests/ground_cases.py share is below; ground_reference is the rule on the host, serial.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define STAC_GROUND_HD __host__ __device__ inline
#else
#define STAC_GROUND_HD inline
#endif

namespace stac {

enum GroundType : int32_t { kGroundSphere = 2, kGroundCapsule = 3, kGroundEllipsoid = 4, kGroundCylinder = 5, kGroundBox = 6, kGroundMesh = 7 };
enum GroundMeta : int32_t { kGroundType = 0, kGroundBody = 1, kGroundInclude = 2, kGroundSlot = 3, kGroundVertFirst = 4, kGroundVertCount = 5 };

constexpr int32_t kGroundMetaWords = 6;    // integers of a table row
constexpr int32_t kGroundDataWords = 15;   // floats of a table row: size[3], pos[3], R[3][3]
constexpr int32_t kGroundMaxSlots = 32;    // track slots at most (a lane keeps their not-finite flags in one word)
constexpr int32_t kGroundTile = 64;        // frames of a tile: one per lane of the workgroup's one wavefront
constexpr int32_t kGroundBodyChunk = 48;   // bodies of a tile that are staged in LDS at a time: 4 words per (body, frame)
constexpr int32_t kGroundTilePitch = 65;   // words between two staged rows: 64 frames and one of padding (conflict-free both ways)
// The LDS of a workgroup is kGroundBodyChunk * 4 * kGroundTilePitch words of staged bodies (49 920 B: three workgroups share the
// 160 KiB of a CU), 64 words per slot and 2 words per geom (its running minimum and count).  The capacities follow from it:
constexpr int32_t kGroundMaxGeoms = 4096;  // geoms of a table at most: 32 KiB of running minima and counts
constexpr int32_t kGroundMaxBodies = 4096; // bodies at most: they pass through the staging rows 48 at a time, so LDS does not bound them;
                                           // this bounds the 32-bit word offsets within a tile (64 * 4096 * 4 < 2^31)
constexpr int32_t kGroundMaxVerts = 1 << 20;  // mesh vertices of a table at most: they stay in global memory (3 * V words < 2^31)
constexpr int64_t kGroundMaxFrames = 1ll << 40;

STAC_GROUND_HD uint32_t ground_bits(float x) {
    union { uint32_t u; float f; } v;
    v.f = x;
    return v.u;
}
STAC_GROUND_HD float ground_float(uint32_t u) {
    union { uint32_t u; float f; } v;
    v.u = u;
    return v.f;
}
STAC_GROUND_HD float ground_quiet_nan() { return ground_float(0x7FC00000u); }
STAC_GROUND_HD float ground_inf() { return ground_float(0x7F800000u); }
STAC_GROUND_HD float ground_abs(float x) { return ground_float(ground_bits(x) & 0x7FFFFFFFu); }  // clears the sign bit: no arithmetic
// Finite: neither an infinity nor a NaN, told from the exponent bits (no compiler may fold it away under any flag)
STAC_GROUND_HD bool ground_finite(float x) { return (ground_bits(x) & 0x7F800000u) != 0x7F800000u; }
// The order of the floats as the order of unsigned integers: -inf < ... < -0 < +0 < ... < +inf
STAC_GROUND_HD uint32_t ground_key(float x) {
    const uint32_t b = ground_bits(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
STAC_GROUND_HD float ground_unkey(uint32_t k) { return ground_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
constexpr uint32_t kGroundKeyInf = 0xFF800000u;  // ground_key(+inf): above the key of every finite value

// The z row of the rotation of the unit quaternion (w, x, y, z)
STAC_GROUND_HD void ground_body_row(float w, float x, float y, float z, float *bz) {
    bz[0] = 2.0f * (x * z - w * y);
    bz[1] = 2.0f * (y * z + w * x);
    bz[2] = 1.0f - 2.0f * (x * x + y * y);
}

// z_g of one geom in one frame: pz = xpos[t][body][2], bz the body's row, data the geom's fifteen floats, verts the table's vertices
STAC_GROUND_HD float ground_geom_z(float pz, const float *bz, int32_t type, const float *data, const float *verts, int32_t vert_first,
                                   int32_t vert_count) {
    const float *s = data, *p = data + 3, *R = data + 6;
    const float cz = pz + ((bz[0] * p[0] + bz[1] * p[1]) + bz[2] * p[2]);
    const float r0 = (bz[0] * R[0] + bz[1] * R[3]) + bz[2] * R[6];
    const float r1 = (bz[0] * R[1] + bz[1] * R[4]) + bz[2] * R[7];
    const float r2 = (bz[0] * R[2] + bz[1] * R[5]) + bz[2] * R[8];
    float h;
    switch (type) {
        case kGroundSphere: h = s[0]; break;
        case kGroundCapsule: h = s[0] + ground_abs(r2) * s[1]; break;
        case kGroundEllipsoid: {
            const float a = r0 * s[0], b = r1 * s[1], c = r2 * s[2];
            h = sqrtf((a * a + b * b) + c * c);
            break;
        }
        case kGroundCylinder: h = ground_abs(r2) * s[1] + s[0] * sqrtf(r0 * r0 + r1 * r1); break;
        case kGroundBox: h = (ground_abs(r0) * s[0] + ground_abs(r1) * s[1]) + ground_abs(r2) * s[2]; break;
        default: {  // kGroundMesh: the lowest vertex; one that is not finite makes the geom's z_g the quiet NaN
            uint32_t best = 0xFFFFFFFFu;
            bool bad = false;
            const float *v = verts + 3 * (int64_t)vert_first;
            for (int32_t i = 0; i < vert_count; ++i, v += 3) {
                const float d = (r0 * v[0] + r1 * v[1]) + r2 * v[2];
                bad |= !ground_finite(d);
                const uint32_t k = ground_key(d);
                best = k < best ? k : best;
            }
            return bad ? ground_quiet_nan() : cz + ground_unkey(best);
        }
    }
    return cz - h;
}

// A table row: 0, or the number of the first rule it breaks (the entry point turns it into a text)
//   1 an unknown type   2 a body outside 1 .. nbody - 1   3 include not 0 or 1   4 a slot outside -1 .. S - 1
//   5 a mesh whose range is empty or outside verts
inline int ground_check_geom(const int32_t *m, int32_t nbody, int32_t n_slots, int32_t n_verts) {
    if (m[kGroundType] < kGroundSphere || m[kGroundType] > kGroundMesh) return 1;
    if (m[kGroundBody] < 1 || m[kGroundBody] >= nbody) return 2;
    if (m[kGroundInclude] != 0 && m[kGroundInclude] != 1) return 3;
    if (m[kGroundSlot] < -1 || m[kGroundSlot] >= n_slots) return 4;
    if (m[kGroundType] == kGroundMesh &&
        (m[kGroundVertCount] < 1 || m[kGroundVertFirst] < 0 || (int64_t)m[kGroundVertFirst] + m[kGroundVertCount] > n_verts))
        return 5;
    return 0;
}

// Frames of a workgroup: whole tiles, as few as give at most kGroundMaxGroups workgroups (the outputs do not depend on it).  A
// chip holds 768 of these workgroups at a time (three per CU by their LDS), so a few thousand leave a short last round, while each
// still folds several tiles into its per-geom words before it touches the atomics.
constexpr int64_t kGroundMaxGroups = 4096;
inline int64_t ground_tiles_per_group(int64_t n_frames) {
    const int64_t tiles = (n_frames + kGroundTile - 1) / kGroundTile;
    return tiles <= kGroundMaxGroups ? 1 : (tiles + kGroundMaxGroups - 1) / kGroundMaxGroups;
}

// The rule on the host, one serial pass over a checked table.  Every output is written.
inline void ground_reference(const float *xpos, const float *xquat, int64_t N, int32_t nbody, const int32_t *meta, const float *data, int32_t G,
                             const float *verts, int32_t S, float z_ref, float *low_z, int32_t *low_geom, float *track_z, float *geom_min,
                             int64_t *geom_below) {
    for (int32_t g = 0; g < G; ++g) geom_min[g] = ground_inf(), geom_below[g] = 0;
    for (int64_t t = 0; t < N; ++t) {
        uint32_t low = kGroundKeyInf, track[kGroundMaxSlots], tbad = 0;
        int32_t low_g = -1;
        bool bad = false;
        for (int32_t s = 0; s < S; ++s) track[s] = kGroundKeyInf;
        for (int32_t g = 0; g < G; ++g) {
            const int32_t *m = meta + (int64_t)g * kGroundMetaWords;
            const float *q = xquat + (t * nbody + m[kGroundBody]) * 4;
            float bz[3];
            ground_body_row(q[0], q[1], q[2], q[3], bz);
            const float z = ground_geom_z(xpos[(t * nbody + m[kGroundBody]) * 3 + 2], bz, m[kGroundType], data + (int64_t)g * kGroundDataWords,
                                          verts, m[kGroundVertFirst], m[kGroundVertCount]);
            const bool fin = ground_finite(z);
            const uint32_t k = ground_key(z);
            if (m[kGroundInclude]) {
                bad |= !fin;
                if (fin && k < low) low = k, low_g = g;
            }
            if (m[kGroundSlot] >= 0) {
                if (!fin) tbad |= 1u << m[kGroundSlot];
                else if (k < track[m[kGroundSlot]]) track[m[kGroundSlot]] = k;
            }
            if (fin) {
                if (k < ground_key(geom_min[g])) geom_min[g] = z;
                geom_below[g] += z < z_ref;
            }
        }
        low_z[t] = bad ? ground_quiet_nan() : ground_unkey(low);
        low_geom[t] = bad ? -1 : low_g;
        for (int32_t s = 0; s < S; ++s) track_z[t * S + s] = ((tbad >> s) & 1u) ? ground_quiet_nan() : ground_unkey(track[s]);
    }
}

}  // namespace stac
