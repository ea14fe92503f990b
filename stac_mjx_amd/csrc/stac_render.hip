// Ray caster of primitive- and mesh-geom scenes: the hot path of Renderer / Stac.render (DESIGN.md "Rendering").
//
// One workgroup = one 16 x 16 tile of one frame (grid z strides over the frames).  Per frame the workgroup
//   1. builds the frame's primitive records in LDS (the primitive pass: world pose and bounding sphere of every
//      static primitive from xpos / xquat, the keypoint and marker spheres and the error segments);
//   2. culls them against the tile's frustum into a compact list (wave ballot + prefix count);
//   3. casts one ray per pixel centre against the list, keeps the nearest opaque hit and the kRenderLayers nearest
//      transparent hits in registers, shades and composites them, and writes rgb / seg / depth.
// A mesh instance is one more primitive: its record holds the pose of the geom frame and the bounding sphere of the mesh's
// root box; its triangles and their hierarchy stay in global memory (hit_mesh).  The kernel is built twice: render_kernel<false>
// is the kernel of mesh-free scenes, render_kernel<true> adds the mesh records, the culled list of mesh instances and the
// loop over it, after the loop over the quadrics and boxes so that the lanes of a wavefront walk the same tree together.
// The arithmetic is written operation by operation (no FMA: -ffp-contract=off) so that tests/tools/render_ref.c,
// the one CPU restatement of both kernels, built with float, reproduces every output bit for bit.
#include <hip/hip_runtime.h>

#include <math.h>

#include "stac_host.hpp"
#include "stac_render.hpp"

namespace stac {
namespace {

enum { T_NONE = -1, T_PLANE = 0, T_SPHERE = 2, T_CAPSULE = 3, T_ELLIPSOID = 4, T_CYLINDER = 5, T_BOX = 6, T_MESH = 7 };

constexpr float kMeshPad = 1.0f / 65536.0f;  // hit_mesh: box padding per unit of coordinate magnitude (float32 eps = 2^-24)

__device__ inline float dot3(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// w,x,y,z -> row-major rotation matrix (columns = the rotated frame's axes)
__device__ inline void quat_mat(const float *q, float *R) {
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    const float ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    const float wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
    R[0] = ww + xx - yy - zz; R[1] = 2.0f * (xy - wz);     R[2] = 2.0f * (xz + wy);
    R[3] = 2.0f * (xy + wz);  R[4] = ww - xx + yy - zz;    R[5] = 2.0f * (yz - wx);
    R[6] = 2.0f * (xz - wy);  R[7] = 2.0f * (yz + wx);     R[8] = ww - xx - yy + zz;
}

// R^T v (world -> local)
__device__ inline void mat_tvec(const float *R, const float *v, float *out) {
#pragma unroll
    for (int j = 0; j < 3; ++j) out[j] = R[j] * v[0] + R[3 + j] * v[1] + R[6 + j] * v[2];
}

// R v (local -> world)
__device__ inline void mat_vec(const float *R, const float *v, float *out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2];
}

__device__ inline bool finite3(const float *p) { return p[0] == p[0] && p[1] == p[1] && p[2] == p[2]; }

// Record layout (kRenderRecWords floats): c[0:3] world centre, R[3:12] world rotation (row-major), size[12:15],
// bounding radius [15], type [16], flags [17] (as floats: small integers are exact).  A mesh: c = world centre of the mesh's
// root box (what the cull needs), [12:15] = world position of the geom frame's origin, [18] = mesh index, [19] = sum over the
// axes of the root box's largest |coordinate| (the scale of hit_mesh's padding).
template <bool MESH>
__device__ void build_prim(const RenderScene &S, const RenderCall &C, int f, int i, float *r) {
    int type = T_NONE, flags = 0;
    float c[3] = {0.0f, 0.0f, 0.0f};
    float R[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    float sz[3] = {0.0f, 0.0f, 0.0f};
    [[maybe_unused]] float mesh_brad = 0.0f, mesh_idx = 0.0f, mesh_mag = 0.0f;
    const int P = S.P, K = S.K;
    if (i < P) {
        type = S.prim_type[i];
        flags = S.prim_flags[i];
        const int b = S.prim_body[i];
        const float *xp = C.xpos + ((size_t)f * S.nbody + b) * 3;
        float Rb[9], Rl[9];
        quat_mat(C.xquat + ((size_t)f * S.nbody + b) * 4, Rb);
        quat_mat(S.prim_quat + 4 * i, Rl);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int q = 0; q < 3; ++q) R[3 * a + q] = Rb[3 * a] * Rl[q] + Rb[3 * a + 1] * Rl[3 + q] + Rb[3 * a + 2] * Rl[6 + q];
        float lp[3];
        mat_vec(Rb, S.prim_pos + 3 * i, lp);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c[a] = xp[a] + lp[a];
            sz[a] = S.prim_size[3 * i + a];
        }
        if constexpr (MESH) {
            if (type == T_MESH) {
                const int mi = S.prim_mesh[i];
                const float *nd = S.mesh_nodes + (size_t)S.mesh_node_off[mi] * kRenderNodeWords;
                float bc[3], he[3], wc[3];
                float mag = 0.0f;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    bc[a] = (nd[a] + nd[3 + a]) * 0.5f;
                    he[a] = (nd[3 + a] - nd[a]) * 0.5f;
                    mag = mag + fmaxf(fabsf(nd[a]), fabsf(nd[3 + a]));
                }
                mat_vec(R, bc, wc);
#pragma unroll
                for (int a = 0; a < 3; ++a) { sz[a] = c[a]; c[a] = c[a] + wc[a]; }
                mesh_brad = sqrtf(dot3(he, he));
                mesh_idx = (float)mi;
                mesh_mag = mag;
            }
        }
    } else if (i < P + K) {
        const int k = i - P;
        if (C.kp) {
            const float *p = C.kp + ((size_t)f * K + k) * 3;
            if (finite3(p)) {
                type = T_SPHERE;
                c[0] = p[0]; c[1] = p[1]; c[2] = p[2];
                sz[0] = S.marker_r;
            }
        }
    } else if (i < P + 2 * K) {
        const int k = i - P - K;
        if (C.markers) {
            const float *p = C.markers + ((size_t)f * K + k) * 3;
            if (finite3(p)) {
                type = T_SPHERE;
                c[0] = p[0]; c[1] = p[1]; c[2] = p[2];
                sz[0] = S.marker_r;
            }
        }
    } else {
        const int k = i - P - 2 * K;
        if (C.show_error && C.kp && C.markers) {
            const float *a = C.kp + ((size_t)f * K + k) * 3;
            const float *m = C.markers + ((size_t)f * K + k) * 3;
            if (finite3(a) && finite3(m)) {
                float d[3] = {m[0] - a[0], m[1] - a[1], m[2] - a[2]};
                const float len = sqrtf(dot3(d, d));
                float w[3] = {0.0f, 0.0f, 1.0f};
                if (len > 0.0f) { w[0] = d[0] / len; w[1] = d[1] / len; w[2] = d[2] / len; }
                type = T_CAPSULE;
#pragma unroll
                for (int q = 0; q < 3; ++q) c[q] = a[q] + d[q] * 0.5f;
                R[2] = w[0]; R[5] = w[1]; R[8] = w[2];  // a capsule uses only its axis (column 2)
                sz[0] = S.seg_r;
                sz[1] = 0.5f * len;
            }
        }
    }
    float brad = 0.0f;
    if (type == T_SPHERE) brad = sz[0];
    else if (type == T_ELLIPSOID) brad = fmaxf(sz[0], fmaxf(sz[1], sz[2]));
    else if (type == T_CAPSULE) brad = sz[1] + sz[0];
    else if (type == T_CYLINDER || type == T_PLANE) brad = sqrtf(sz[0] * sz[0] + sz[1] * sz[1]);
    else if (type == T_BOX) brad = sqrtf(dot3(sz, sz));
    if constexpr (MESH) {
        if (type == T_MESH) brad = mesh_brad;
        r[18] = mesh_idx;
        r[19] = mesh_mag;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) { r[q] = c[q]; r[12 + q] = sz[q]; }
#pragma unroll
    for (int q = 0; q < 9; ++q) r[3 + q] = R[q];
    r[15] = brad;
    r[16] = (float)type;
    r[17] = (float)flags;
}

// Closest-approach sphere test: ray o + t d against |x - ctr| = rad.  Returns the entry t > 0 or -1.
__device__ inline float hit_sphere(const float *ctr, float rad, const float *o, const float *d, float dd) {
    const float oc[3] = {o[0] - ctr[0], o[1] - ctr[1], o[2] - ctr[2]};
    const float tca = -dot3(oc, d) / dd;
    const float p[3] = {oc[0] + d[0] * tca, oc[1] + d[1] * tca, oc[2] + d[2] * tca};
    const float h2 = rad * rad - dot3(p, p);
    if (!(h2 >= 0.0f)) return -1.0f;
    const float t = tca - sqrtf(h2 / dd);
    return t > 0.0f ? t : -1.0f;
}

// Entry t > 0 of the ray against record r (or -1), and the face that was hit (box axis; cylinder / capsule: 0 side,
// 1 top, 2 bottom).  o / d are the world ray, dd = |d|^2.
__device__ float intersect(const float *r, const float *o, const float *d, float dd, int *face) {
    const int type = (int)r[16];
    const float *c = r, *R = r + 3, *sz = r + 12;
    *face = 0;
    if (type == T_SPHERE) return hit_sphere(c, sz[0], o, d, dd);
    const float oc[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
    if (type == T_CAPSULE) {
        const float w[3] = {R[2], R[5], R[8]};
        const float hl = sz[1], rad = sz[0];
        const float oz = dot3(oc, w), dz = dot3(d, w);
        // an origin inside the capsule does not see it: nearer to the axis point at oz clamped to the segment than rad
        const float ozc = fminf(fmaxf(oz, -hl), hl);
        const float oq[3] = {oc[0] - w[0] * ozc, oc[1] - w[1] * ozc, oc[2] - w[2] * ozc};
        const float in2 = rad * rad - dot3(oq, oq);
        if (in2 > 0.0f) return -1.0f;
        const float op[3] = {oc[0] - w[0] * oz, oc[1] - w[1] * oz, oc[2] - w[2] * oz};
        const float dp[3] = {d[0] - w[0] * dz, d[1] - w[1] * dz, d[2] - w[2] * dz};
        const float a = dot3(dp, dp);
        float best = INFINITY;
        if (a > 0.0f) {
            const float tca = -dot3(op, dp) / a;
            const float p[3] = {op[0] + dp[0] * tca, op[1] + dp[1] * tca, op[2] + dp[2] * tca};
            const float h2 = rad * rad - dot3(p, p);
            if (h2 >= 0.0f) {
                const float t = tca - sqrtf(h2 / a);
                const float z = oz + dz * t;
                if (t > 0.0f && fabsf(z) <= hl) best = t;
            }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const float e = s == 0 ? hl : -hl;
            const float ctr[3] = {c[0] + w[0] * e, c[1] + w[1] * e, c[2] + w[2] * e};
            const float t = hit_sphere(ctr, rad, o, d, dd);
            if (t > 0.0f && t < best) { best = t; *face = 1 + s; }
        }
        return best < INFINITY ? best : -1.0f;
    }
    float ol[3], dl[3];
    mat_tvec(R, oc, ol);
    mat_tvec(R, d, dl);
    if (type == T_ELLIPSOID) {
        const float os[3] = {ol[0] / sz[0], ol[1] / sz[1], ol[2] / sz[2]};
        const float ds[3] = {dl[0] / sz[0], dl[1] / sz[1], dl[2] / sz[2]};
        const float a = dot3(ds, ds);
        const float tca = -dot3(os, ds) / a;
        const float p[3] = {os[0] + ds[0] * tca, os[1] + ds[1] * tca, os[2] + ds[2] * tca};
        const float h2 = 1.0f - dot3(p, p);
        if (!(h2 >= 0.0f)) return -1.0f;
        const float t = tca - sqrtf(h2 / a);
        return t > 0.0f ? t : -1.0f;
    }
    if (type == T_PLANE) {
        if (!(ol[2] > 0.0f && dl[2] < 0.0f)) return -1.0f;
        const float t = -ol[2] / dl[2];
        const float x = ol[0] + dl[0] * t, y = ol[1] + dl[1] * t;
        return (t > 0.0f && fabsf(x) <= sz[0] && fabsf(y) <= sz[1]) ? t : -1.0f;
    }
    if (type == T_BOX) {
        float tn = -INFINITY, tf = INFINITY;
        int ax = -1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (dl[k] == 0.0f) {
                if (fabsf(ol[k]) > sz[k]) return -1.0f;
            } else {
                const float t1 = (-sz[k] - ol[k]) / dl[k], t2 = (sz[k] - ol[k]) / dl[k];
                const float lo = t1 < t2 ? t1 : t2, hi = t1 < t2 ? t2 : t1;
                if (lo > tn) { tn = lo; ax = k; }
                if (hi < tf) tf = hi;
            }
        }
        *face = ax;
        return (ax >= 0 && tn <= tf && tn > 0.0f) ? tn : -1.0f;
    }
    if (type == T_CYLINDER) {
        const float rad = sz[0], hl = sz[1];
        float best = INFINITY;
        const float a = dl[0] * dl[0] + dl[1] * dl[1];
        if (a > 0.0f) {
            const float tca = -(ol[0] * dl[0] + ol[1] * dl[1]) / a;
            const float px = ol[0] + dl[0] * tca, py = ol[1] + dl[1] * tca;
            const float h2 = rad * rad - (px * px + py * py);
            if (h2 >= 0.0f) {
                const float t = tca - sqrtf(h2 / a);
                const float z = ol[2] + dl[2] * t;
                if (t > 0.0f && fabsf(z) <= hl) best = t;
            }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const float e = s == 0 ? hl : -hl;
            const bool facing = s == 0 ? (ol[2] > hl && dl[2] < 0.0f) : (ol[2] < -hl && dl[2] > 0.0f);
            if (facing) {
                const float t = (e - ol[2]) / dl[2];
                const float x = ol[0] + dl[0] * t, y = ol[1] + dl[1] * t;
                if (t > 0.0f && x * x + y * y <= rad * rad && t < best) { best = t; *face = 1 + s; }
            }
        }
        return best < INFINITY ? best : -1.0f;
    }
    return -1.0f;
}

// Nearest hit of the ray against the mesh instance of record r: t > 0 of the triangle with the smallest t, ties to the lower
// triangle index (*tri), or -1.  The ray goes to the geom frame; the nodes are walked in their depth-first order by skip
// links (no stack): a node whose padded box the ray misses, or enters beyond the best hit so far, hands over to its skip link.
// The padding (kMeshPad per unit of coordinate magnitude, far above the rounding of the slab test and of the triangle test)
// makes sure that no box is rejected whose triangle the ray hits, so the result is that of testing every triangle.
// Two-sided Moeller-Trumbore test on the face normal N = e1 x e2; N = 0 (a zero-area triangle) gives det = 0: never hit.
__device__ float hit_mesh(const RenderScene &S, const float *r, const float *o, const float *d, int *tri) {
    const float *R = r + 3, *org = r + 12;
    const int mi = (int)r[18];
    const float oc[3] = {o[0] - org[0], o[1] - org[1], o[2] - org[2]};
    float ol[3], dl[3];
    mat_tvec(R, oc, ol);
    mat_tvec(R, d, dl);
    const float pad = (fabsf(ol[0]) + fabsf(ol[1]) + fabsf(ol[2]) + r[19]) * kMeshPad;
    const float idl[3] = {1.0f / dl[0], 1.0f / dl[1], 1.0f / dl[2]};
    const int n0 = S.mesh_node_off[mi];
    const int nn = S.mesh_node_off[mi + 1] - n0;
    const float4 *nodes = reinterpret_cast<const float4 *>(S.mesh_nodes + (size_t)n0 * kRenderNodeWords);
    const float *tris = S.mesh_tris + (size_t)S.mesh_tri_off[mi] * 9;
    float best = INFINITY;
    int btri = -1;
    int n = 0;
    while (n < nn) {
        const float4 a = nodes[2 * n], b = nodes[2 * n + 1];
        const float lo[3] = {a.x, a.y, a.z}, hi[3] = {a.w, b.x, b.y};
        const int w6 = __float_as_int(b.z), w7 = __float_as_int(b.w);  // leaf: first, count; inner node: skip, 0
        float tn = -INFINITY, tf = INFINITY;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float t1 = ((lo[k] - pad) - ol[k]) * idl[k], t2 = ((hi[k] + pad) - ol[k]) * idl[k];
            const float lo_t = t1 < t2 ? t1 : t2, hi_t = t1 < t2 ? t2 : t1;
            if (lo_t > tn) tn = lo_t;
            if (hi_t < tf) tf = hi_t;
        }
        if (!(tn <= tf && tf > 0.0f && tn <= best)) {
            n = w7 > 0 ? n + 1 : w6;
            continue;
        }
        for (int k = 0; k < w7; ++k) {
            const int ti = w6 + k;
            const float *v = tris + (size_t)ti * 9;
            const float e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]};
            const float e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
            const float N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            const float det = -dot3(dl, N);
            if (det == 0.0f) continue;
            const float inv = 1.0f / det;
            const float ao[3] = {ol[0] - v[0], ol[1] - v[1], ol[2] - v[2]};
            const float dao[3] = {ao[1] * dl[2] - ao[2] * dl[1], ao[2] * dl[0] - ao[0] * dl[2], ao[0] * dl[1] - ao[1] * dl[0]};
            const float bu = dot3(e2, dao) * inv;
            const float bv = -dot3(e1, dao) * inv;
            const float t = dot3(ao, N) * inv;
            if (bu >= 0.0f && bv >= 0.0f && bu + bv <= 1.0f && t > 0.0f && (t < best || (t == best && ti < btri))) {
                best = t;
                btri = ti;
            }
        }
        n = n + 1;
    }
    *tri = btri;
    return btri >= 0 ? best : -1.0f;
}

// Unit world normal of record r at the hit (t, face) of the ray o + t d (a mesh: of its triangle tri, towards the ray's origin).
template <bool MESH>
__device__ void normal_at(const RenderScene &S, const float *r, const float *o, const float *d, float t, int face, int tri, float *n) {
    const int type = (int)r[16];
    const float *c = r, *R = r + 3, *sz = r + 12;
    const float q[3] = {o[0] + d[0] * t - c[0], o[1] + d[1] * t - c[1], o[2] + d[2] * t - c[2]};
    float v[3];
    if (type == T_SPHERE) {
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
    } else if (type == T_CAPSULE) {
        const float w[3] = {R[2], R[5], R[8]};
        const float z = face == 0 ? dot3(q, w) : (face == 1 ? sz[1] : -sz[1]);
        v[0] = q[0] - w[0] * z; v[1] = q[1] - w[1] * z; v[2] = q[2] - w[2] * z;
    } else if (type == T_PLANE) {
        v[0] = R[2]; v[1] = R[5]; v[2] = R[8];
    } else if (MESH && type == T_MESH) {
        if constexpr (MESH) {
            const float *p = S.mesh_tris + ((size_t)S.mesh_tri_off[(int)r[18]] + (size_t)tri) * 9;
            const float e1[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]};
            const float e2[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
            float N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            float dl[3];
            mat_tvec(R, d, dl);
            if (dot3(dl, N) > 0.0f) { N[0] = -N[0]; N[1] = -N[1]; N[2] = -N[2]; }
            mat_vec(R, N, v);
        }
    } else {
        float ql[3], nl[3];
        mat_tvec(R, q, ql);
        if (type == T_ELLIPSOID) {
            nl[0] = ql[0] / (sz[0] * sz[0]); nl[1] = ql[1] / (sz[1] * sz[1]); nl[2] = ql[2] / (sz[2] * sz[2]);
        } else if (type == T_BOX) {
            float dl[3];
            mat_tvec(R, d, dl);
            nl[0] = 0.0f; nl[1] = 0.0f; nl[2] = 0.0f;
            const float sgn = (face == 0 ? dl[0] : (face == 1 ? dl[1] : dl[2])) < 0.0f ? 1.0f : -1.0f;
            if (face == 0) nl[0] = sgn; else if (face == 1) nl[1] = sgn; else nl[2] = sgn;
        } else {  // cylinder
            nl[0] = face == 0 ? ql[0] : 0.0f;
            nl[1] = face == 0 ? ql[1] : 0.0f;
            nl[2] = face == 0 ? 0.0f : (face == 1 ? 1.0f : -1.0f);
        }
        mat_vec(R, nl, v);
    }
    const float len = sqrtf(dot3(v, v));
    n[0] = v[0] / len; n[1] = v[1] / len; n[2] = v[2] / len;
}

// Shaded colour of primitive `id` (record r) at the hit (t, face).  zc = the camera's z axis (towards the viewer).
template <bool MESH>
__device__ void shade(const RenderScene &S, const float *r, int id, const float *o, const float *d, float t, int face, int tri,
                      const float *zc, float *col) {
    float n[3];
    normal_at<MESH>(S, r, o, d, t, face, tri, n);
    const int P = S.P, K = S.K;
    float rgb[3];
    if (id < P) {
        const float *c1 = S.prim_rgba + 4 * id;
        rgb[0] = c1[0]; rgb[1] = c1[1]; rgb[2] = c1[2];
        const int flags = (int)r[17];
        if (flags & STAC_RENDER_CHECKER) {
            const float *c = r, *R = r + 3, *sz = r + 12;
            const float q[3] = {o[0] + d[0] * t - c[0], o[1] + d[1] * t - c[1], o[2] + d[2] * t - c[2]};
            float ql[3];
            mat_tvec(R, q, ql);
            const float *rep = S.prim_tex + 2 * id;
            const bool uni = (flags & STAC_RENDER_TEXUNIFORM) != 0;
            const float u = ql[0] * rep[0] / (uni ? 1.0f : 2.0f * sz[0]);
            const float v = ql[1] * rep[1] / (uni ? 1.0f : 2.0f * sz[1]);
            const int cell = (int)floorf(2.0f * u) + (int)floorf(2.0f * v);
            if (cell & 1) {
                const float *c2 = S.prim_rgb2 + 3 * id;
                rgb[0] = c2[0]; rgb[1] = c2[1]; rgb[2] = c2[2];
            }
        }
    } else if (id < P + K) {
        const float *c1 = S.kp_rgba + 4 * (id - P);
        rgb[0] = c1[0]; rgb[1] = c1[1]; rgb[2] = c1[2];
    } else if (id < P + 2 * K) {
        rgb[0] = S.marker_rgba[0]; rgb[1] = S.marker_rgba[1]; rgb[2] = S.marker_rgba[2];
    } else {
        rgb[0] = S.seg_rgba[0]; rgb[1] = S.seg_rgba[1]; rgb[2] = S.seg_rgba[2];
    }
    const float ch = fmaxf(dot3(n, zc), 0.0f);
    float L[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) L[q] = S.head_amb[q] + S.head_diff[q] * ch;
    for (int l = 0; l < S.nlight; ++l) {
        const float cl = fmaxf(-dot3(n, S.light_dir + 3 * l), 0.0f);
#pragma unroll
        for (int q = 0; q < 3; ++q) L[q] = L[q] + S.light_diff[3 * l + q] * cl;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) col[q] = rgb[q] * fminf(L[q], 1.0f);
}

// u (x) and v (y) of the ray through the centre of pixel column x / row y (row 0 at the top).
__device__ inline float pix_u(int x, int W, float tu) { return (((float)x + 0.5f) * 2.0f / (float)W - 1.0f) * tu; }
__device__ inline float pix_v(int y, int H, float tv) { return (1.0f - ((float)y + 0.5f) * 2.0f / (float)H) * tv; }

// true when the bounding sphere of record r lies entirely outside the frustum of the tile (half-spaces through the camera
// centre with normals in camera coordinates) or behind the camera.  The margin keeps the test conservative against the
// float rounding of the ray directions and of this test itself.
__device__ inline bool culled(const float *r, const float *cam, float uL, float uR, float vT, float vB) {
    if ((int)r[16] == T_NONE) return true;
    const float w[3] = {r[0] - cam[0], r[1] - cam[1], r[2] - cam[2]};
    float q[3];
    mat_tvec(cam + 3, w, q);
    const float m = r[15] * 1.001f + 1e-4f * sqrtf(dot3(q, q)) + 1e-6f;
    if (q[2] > m) return true;
    if ((q[0] + uL * q[2]) < -m * sqrtf(1.0f + uL * uL)) return true;
    if ((-q[0] - uR * q[2]) < -m * sqrtf(1.0f + uR * uR)) return true;
    if ((-q[1] - vT * q[2]) < -m * sqrtf(1.0f + vT * vT)) return true;
    if ((q[1] + vB * q[2]) < -m * sqrtf(1.0f + vB * vB)) return true;
    return false;
}

__device__ inline uint8_t quant(float c) {
    const float x = c < 0.0f ? 0.0f : (c > 1.0f ? 1.0f : c);
    return (uint8_t)(int)floorf(x * 255.0f + 0.5f);
}

// One hit of the pixel's ray: a transparent one goes into the sorted layers, an opaque one competes for the nearest.
// key = bits(t) << 32 | id << 22 | tri << 2 | face (t > 0, so the bits of t order like t; id < 2^10, tri < 2^20, 0 for a
// primitive that is no mesh): the layers are ordered by (t, id); ~0 = empty.
__device__ __forceinline__ void take_hit(const float *r, int id, float t, int face, int tri, unsigned long long (&L)[kRenderLayers],
                                         float &to, int &io, int &fo, int &tro) {
    if (((int)r[17]) & STAC_RENDER_TRANSPARENT) {
        unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | ((unsigned)id << (kRenderTriBits + 2)) |
                                 ((unsigned)tri << 2) | (unsigned)face;
#pragma unroll
        for (int k = 0; k < kRenderLayers; ++k) {  // insertion into the sorted list; the largest key drops out
            const unsigned long long cur = L[k];
            L[k] = key < cur ? key : cur;
            key = key < cur ? cur : key;
        }
    } else if (t < to || (t == to && id < io)) {
        to = t; io = id; fo = face; tro = tri;
    }
}

template <bool MESH>
__global__ __launch_bounds__(kRenderTile *kRenderTile) void render_kernel(const RenderScene *__restrict__ Sp, RenderCall C) {
    const RenderScene &S = *Sp;
    __shared__ float rec[kRenderMaxPrims * kRenderRecWords];
    __shared__ int list[kRenderMaxPrims];
    __shared__ int wcount[kRenderTile * kRenderTile / 64];
    __shared__ int mlist[MESH ? kRenderMaxPrims : 1];  // the tile's mesh instances
    __shared__ int wmcount[kRenderTile * kRenderTile / 64];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int Ptot = S.P + 3 * S.K;
    const int x0 = blockIdx.x * kRenderTile, y0 = blockIdx.y * kRenderTile;
    const int x = x0 + (tid % kRenderTile), y = y0 + (tid / kRenderTile);
    const bool inside = x < C.W && y < C.H;
    const float tv = C.tanh, tu = C.tanh * ((float)C.W / (float)C.H);
    const float uL = pix_u(x0, C.W, tu), uR = pix_u(min(x0 + kRenderTile, C.W) - 1, C.W, tu);
    const float vT = pix_v(y0, C.H, tv), vB = pix_v(min(y0 + kRenderTile, C.H) - 1, C.H, tv);
    for (int f = blockIdx.z; f < C.N; f += gridDim.z) {
        __syncthreads();  // the previous frame's readers are done with rec / list
        for (int i = tid; i < Ptot; i += kRenderTile * kRenderTile) build_prim<MESH>(S, C, f, i, rec + i * kRenderRecWords);
        __syncthreads();
        const float *cam = C.cam + (size_t)f * 12;
        int count = 0;
        [[maybe_unused]] int mcount = 0;
        for (int base = 0; base < Ptot; base += kRenderTile * kRenderTile) {
            const int i = base + tid;
            bool vis = i < Ptot && !culled(rec + i * kRenderRecWords, cam, uL, uR, vT, vB);
            bool mvis = false;
            if constexpr (MESH) {
                mvis = vis && (int)rec[i * kRenderRecWords + 16] == T_MESH;
                vis = vis && !mvis;
                const unsigned long long mm = __ballot(mvis);
                if (lane == 0) wmcount[wave] = __popcll(mm);
                __syncthreads();
                int moff = mcount, mtotal = 0;
#pragma unroll
                for (int w = 0; w < kRenderTile * kRenderTile / 64; ++w) {
                    if (w < wave) moff += wmcount[w];
                    mtotal += wmcount[w];
                }
                if (mvis) mlist[moff + __popcll(mm & ((1ull << lane) - 1ull))] = i;
                mcount += mtotal;
            }
            const unsigned long long mask = __ballot(vis);
            const int pre = __popcll(mask & ((1ull << lane) - 1ull));
            if (lane == 0) wcount[wave] = __popcll(mask);
            __syncthreads();
            int off = count, total = 0;
#pragma unroll
            for (int w = 0; w < kRenderTile * kRenderTile / 64; ++w) {
                if (w < wave) off += wcount[w];
                total += wcount[w];
            }
            if (vis) list[off + pre] = i;
            count += total;
            __syncthreads();
        }
        if (!inside) continue;
        const float o[3] = {cam[0], cam[1], cam[2]};
        const float *Rc = cam + 3;
        const float u = pix_u(x, C.W, tu), v = pix_v(y, C.H, tv);
        float d[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) d[q] = Rc[3 * q] * u + Rc[3 * q + 1] * v - Rc[3 * q + 2];
        {
            const float len = sqrtf(dot3(d, d));
            d[0] = d[0] / len; d[1] = d[1] / len; d[2] = d[2] / len;
        }
        const float dd = dot3(d, d);
        float to = INFINITY;
        int io = -1, fo = 0, tro = 0;
        // the kRenderLayers nearest transparent hits, sorted by (t, id): see take_hit.  One 64-bit key per slot keeps t, id,
        // triangle and face together through the network.
        unsigned long long L[kRenderLayers];
#pragma unroll
        for (int k = 0; k < kRenderLayers; ++k) L[k] = ~0ull;
        for (int j = 0; j < count; ++j) {
            const int id = list[j];
            const float *r = rec + id * kRenderRecWords;
            int face;
            const float t = intersect(r, o, d, dd, &face);
            if (!(t > 0.0f)) continue;
            take_hit(r, id, t, face, 0, L, to, io, fo, tro);
        }
        if constexpr (MESH) {
            for (int j = 0; j < mcount; ++j) {
                const int id = mlist[j];
                const float *r = rec + id * kRenderRecWords;
                int tri;
                const float t = hit_mesh(S, r, o, d, &tri);
                if (!(t > 0.0f)) continue;
                take_hit(r, id, t, 0, tri, L, to, io, fo, tro);
            }
        }
        const float zc[3] = {Rc[2], Rc[5], Rc[8]};
        float col[3] = {S.bg[0], S.bg[1], S.bg[2]};
        if (io >= 0) shade<MESH>(S, rec + io * kRenderRecWords, io, o, d, to, fo, tro, zc, col);
        const float a = S.alpha, na = 1.0f - S.alpha;
#pragma unroll
        for (int k = kRenderLayers - 1; k >= 0; --k) {  // back to front
            const float tk = __uint_as_float((unsigned)(L[k] >> 32));
            const int ik = (int)((L[k] >> (kRenderTriBits + 2)) & 0x3ffu), fk = (int)(L[k] & 3u);
            const int trk = (int)((L[k] >> 2) & ((1u << kRenderTriBits) - 1u));
            if (L[k] != ~0ull && tk < to) {
                float s[3];
                shade<MESH>(S, rec + ik * kRenderRecWords, ik, o, d, tk, fk, trk, zc, s);
#pragma unroll
                for (int q = 0; q < 3; ++q) col[q] = col[q] * na + s[q] * a;
            }
        }
        const size_t px = ((size_t)f * C.H + y) * C.W + x;
        if (C.rgb) {
            C.rgb[3 * px] = quant(col[0]);
            C.rgb[3 * px + 1] = quant(col[1]);
            C.rgb[3 * px + 2] = quant(col[2]);
        }
        if (C.seg) C.seg[px] = io;
        if (C.depth) C.depth[px] = to;
    }
}

}  // namespace

static hipError_t launch_render(const RenderScene *S, const RenderCall &C, bool meshes, hipStream_t s) {
    if (C.N <= 0) return hipSuccess;
    const dim3 grid((C.W + kRenderTile - 1) / kRenderTile, (C.H + kRenderTile - 1) / kRenderTile, C.N < 65535 ? C.N : 65535);
    if (meshes) hipLaunchKernelGGL(render_kernel<true>, grid, dim3(kRenderTile * kRenderTile), 0, s, S, C);
    else hipLaunchKernelGGL(render_kernel<false>, grid, dim3(kRenderTile * kRenderTile), 0, s, S, C);
    return hipGetLastError();
}

}  // namespace stac

// ---- C ABI entry points (include/stac_hip.h): the scene object and stac_render -----------------------------------------------------
struct stac_render_scene {
    int device = 0;
    RenderScene S{};               // what d_scene holds (device pointers into d_int / d_float)
    RenderScene *d_scene = nullptr;
    int32_t *d_int = nullptr;
    float *d_float = nullptr;
    float *d_nodes = nullptr;      // meshes: kRenderNodeWords words per node (see stac_render.hpp)
    float *d_tris = nullptr;       // [NT,3,3]
    bool has_mesh = false;         // a type-7 primitive: render with the mesh kernel
};

// Checks stac_render_meshes against the tables (see include/stac_hip.h).  Returns STAC_OK, or the code of the fail() it made.
static int check_render_meshes(const stac_render_tables *t, const stac_render_meshes *ms, bool *has_mesh) {
    const std::string who = "stac_render_scene_create_with_meshes: ";
    *has_mesh = false;
    if (ms->nmesh < 0 || (ms->nmesh && (!ms->node_offset || !ms->tri_offset || !ms->node_box || !ms->node_link || !ms->tri_vertex)))
        return fail(STAC_ERR_INVALID, who + "bad argument");
    if (ms->nmesh && (ms->node_offset[0] != 0 || ms->tri_offset[0] != 0))
        return fail(STAC_ERR_INVALID, who + "node_offset[0] and tri_offset[0] must be 0");
    for (int k = 0; k < ms->nmesh; ++k) {
        const long nn = (long)ms->node_offset[k + 1] - ms->node_offset[k], nt = (long)ms->tri_offset[k + 1] - ms->tri_offset[k];
        if (nn < 1 || nt < 0) return fail(STAC_ERR_INVALID, who + "mesh " + std::to_string(k) + " has no node, or offsets that decrease");
        if (nt > STAC_RENDER_MAX_MESH_TRIS)
            return fail(STAC_ERR_CAPACITY, who + "mesh " + std::to_string(k) + " has " + std::to_string(nt) +
                                               " triangles, more than STAC_RENDER_MAX_MESH_TRIS = " + std::to_string(STAC_RENDER_MAX_MESH_TRIS));
        const int32_t *link = ms->node_link + 3 * (size_t)ms->node_offset[k];
        for (long n = 0; n < nn; ++n) {
            const long skip = link[3 * n], first = link[3 * n + 1], count = link[3 * n + 2];
            if (skip <= n || skip > nn || (count > 0 && skip != n + 1))
                return fail(STAC_ERR_INVALID, who + "mesh " + std::to_string(k) + " node " + std::to_string(n) + ": skip link " +
                                                  std::to_string(skip) + " does not point forward inside the mesh's " + std::to_string(nn) +
                                                  " nodes (a leaf's is the next node)");
            if (count < 0 || (count > 0 && (first < 0 || first + count > nt)))
                return fail(STAC_ERR_INVALID, who + "mesh " + std::to_string(k) + " node " + std::to_string(n) + ": leaf range " +
                                                  std::to_string(first) + " + " + std::to_string(count) + " outside the mesh's " +
                                                  std::to_string(nt) + " triangles");
        }
    }
    for (int i = 0; i < t->nprim; ++i) {
        if (t->prim_type[i] != 7) continue;
        *has_mesh = true;
        if (!ms->prim_mesh || ms->prim_mesh[i] < 0 || ms->prim_mesh[i] >= ms->nmesh)
            return fail(STAC_ERR_INVALID, who + "primitive " + std::to_string(i) + " is a mesh (type 7) without a mesh, or with a mesh index out of range");
    }
    return STAC_OK;
}

extern "C" stac_render_scene *stac_render_scene_create(const stac_model *m, const stac_render_tables *t) {
    return stac_render_scene_create_with_meshes(m, t, nullptr);
}

extern "C" stac_render_scene *stac_render_scene_create_with_meshes(const stac_model *m, const stac_render_tables *t,
                                                                   const stac_render_meshes *ms) {
    if (!m || !t || t->nprim < 0 || t->nkp < 0 || t->nlight < 0 || (t->nprim && (!t->prim_type || !t->prim_body || !t->prim_flags
        || !t->prim_size || !t->prim_pos || !t->prim_quat || !t->prim_rgba || !t->prim_rgb2 || !t->prim_texrepeat))
        || (t->nkp && !t->kp_rgba) || (t->nlight && (!t->light_dir || !t->light_diffuse))) {
        fail(STAC_ERR_INVALID, "stac_render_scene_create: bad argument");
        return nullptr;
    }
    const long total = (long)t->nprim + 3L * t->nkp;
    if (total > STAC_RENDER_MAX_PRIMS) {
        fail(STAC_ERR_CAPACITY, "stac_render_scene_create: " + std::to_string(total) + " primitives (P + 3K) exceed STAC_RENDER_MAX_PRIMS = " +
                                    std::to_string(STAC_RENDER_MAX_PRIMS));
        return nullptr;
    }
    const int P = t->nprim, K = t->nkp, NL = t->nlight;
    for (int i = 0; i < P; ++i) {
        const int ty = t->prim_type[i];
        if (t->prim_body[i] < 0 || t->prim_body[i] >= m->h.nbody || !(ty == 0 || (ty >= 2 && ty <= 6) || (ty == 7 && ms))) {
            fail(STAC_ERR_INVALID, "stac_render_scene_create: primitive " + std::to_string(i) + " has a bad type or body");
            return nullptr;
        }
    }
    bool has_mesh = false;
    if (ms && check_render_meshes(t, ms, &has_mesh) != STAC_OK) return nullptr;
    // with meshes the int block grows by mesh[P] node_offset[M+1] tri_offset[M+1]; nodes and triangles get blocks of their own
    const int M = has_mesh ? ms->nmesh : 0;
    std::vector<float> hnodes;
    std::vector<int32_t> hnoff, htoff;
    if (has_mesh) {
        // developer switch: every mesh as one leaf over all its triangles, to show what the hierarchy saves
        const char *env = getenv("STAC_RENDER_MESH_SINGLE_LEAF");
        const bool single = env && env[0] && env[0] != '0';
        hnoff.push_back(0);
        for (int k = 0; k < M; ++k) {
            const size_t n0 = (size_t)ms->node_offset[k], nn = single ? 1 : (size_t)(ms->node_offset[k + 1] - ms->node_offset[k]);
            for (size_t n = 0; n < nn; ++n) {
                const float *b = ms->node_box + 6 * (n0 + n);
                const int32_t *l = ms->node_link + 3 * (n0 + n);
                const bool leaf = single || l[2] > 0;
                // device node: lo[3], hi[3], then (first, count) of a leaf or (skip, 0) of an inner node, as bit patterns
                const int32_t nt = ms->tri_offset[k + 1] - ms->tri_offset[k];
                const int32_t w6 = single ? (nt > 0 ? 0 : 1) : (leaf ? l[1] : l[0]);  // (an empty mesh: an inner node that ends the walk)
                const int32_t w7 = single ? nt : (leaf ? l[2] : 0);
                float f6, f7;
                memcpy(&f6, &w6, 4);
                memcpy(&f7, &w7, 4);
                hnodes.insert(hnodes.end(), b, b + 6);
                hnodes.push_back(f6);
                hnodes.push_back(f7);
            }
            hnoff.push_back((int32_t)(hnodes.size() / stac::kRenderNodeWords));
        }
        htoff.assign(ms->tri_offset, ms->tri_offset + M + 1);
    }
    // int block: type[P] body[P] flags[P]; float block: size[3P] pos[3P] quat[4P] rgba[4P] rgb2[3P] tex[2P] kp_rgba[4K]
    // light_dir[3NL] light_diff[3NL]
    std::vector<int32_t> hi;
    hi.insert(hi.end(), t->prim_type, t->prim_type + P);
    hi.insert(hi.end(), t->prim_body, t->prim_body + P);
    hi.insert(hi.end(), t->prim_flags, t->prim_flags + P);
    if (has_mesh) {
        for (int i = 0; i < P; ++i) hi.push_back(t->prim_type[i] == 7 ? ms->prim_mesh[i] : -1);
        hi.insert(hi.end(), hnoff.begin(), hnoff.end());
        hi.insert(hi.end(), htoff.begin(), htoff.end());
    }
    std::vector<float> hf;
    size_t off[8];
    auto put = [&](int k, const float *p, size_t n) { off[k] = hf.size(); if (n) hf.insert(hf.end(), p, p + n); };
    put(0, t->prim_size, 3 * (size_t)P); put(1, t->prim_pos, 3 * (size_t)P); put(2, t->prim_quat, 4 * (size_t)P);
    put(3, t->prim_rgba, 4 * (size_t)P); put(4, t->prim_rgb2, 3 * (size_t)P); put(5, t->prim_texrepeat, 2 * (size_t)P);
    put(6, t->kp_rgba, 4 * (size_t)K);
    const size_t off_ld = hf.size();
    if (NL) hf.insert(hf.end(), t->light_dir, t->light_dir + 3 * (size_t)NL);
    const size_t off_lc = hf.size();
    if (NL) hf.insert(hf.end(), t->light_diffuse, t->light_diffuse + 3 * (size_t)NL);
    DeviceGuard dg(m->device);
    auto *sc = new stac_render_scene;
    sc->device = m->device;
    auto bail = [&](hipError_t e) {
        fail(STAC_ERR_HIP, std::string("stac_render_scene_create: ") + hipGetErrorString(e));
        stac_render_scene_destroy(sc);  // (frees what has been allocated so far)
        return nullptr;
    };
    hipError_t e = upload(&sc->d_int, hi.data(), hi.size());
    if (e != hipSuccess) return bail(e);
    e = upload(&sc->d_float, hf.data(), hf.size());
    if (e != hipSuccess) return bail(e);
    RenderScene &S = sc->S;
    sc->has_mesh = has_mesh;
    if (has_mesh) {
        e = upload(&sc->d_nodes, hnodes.data(), hnodes.size());
        if (e != hipSuccess) return bail(e);
        const size_t nt = 9 * (size_t)ms->tri_offset[M];
        const float none[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        e = upload(&sc->d_tris, nt ? ms->tri_vertex : none, nt ? nt : 9);
        if (e != hipSuccess) return bail(e);
        S.nmesh = M;
        S.prim_mesh = sc->d_int + 3 * P; S.mesh_node_off = sc->d_int + 4 * P; S.mesh_tri_off = sc->d_int + 4 * P + M + 1;
        S.mesh_nodes = sc->d_nodes; S.mesh_tris = sc->d_tris;
    }
    S.P = P; S.K = K; S.nbody = m->h.nbody; S.nlight = NL;
    S.prim_type = sc->d_int; S.prim_body = sc->d_int + P; S.prim_flags = sc->d_int + 2 * P;
    S.prim_size = sc->d_float + off[0]; S.prim_pos = sc->d_float + off[1]; S.prim_quat = sc->d_float + off[2];
    S.prim_rgba = sc->d_float + off[3]; S.prim_rgb2 = sc->d_float + off[4]; S.prim_tex = sc->d_float + off[5];
    S.kp_rgba = sc->d_float + off[6]; S.light_dir = sc->d_float + off_ld; S.light_diff = sc->d_float + off_lc;
    for (int q = 0; q < 4; ++q) { S.marker_rgba[q] = t->marker_rgba[q]; S.seg_rgba[q] = t->segment_rgba[q]; }
    S.marker_r = t->marker_radius; S.seg_r = t->segment_radius;
    for (int q = 0; q < 3; ++q) { S.head_amb[q] = t->head_ambient[q]; S.head_diff[q] = t->head_diffuse[q]; S.bg[q] = t->background[q]; }
    S.alpha = t->alpha;
    e = upload(&sc->d_scene, &sc->S, 1);
    if (e != hipSuccess) return bail(e);
    clear_error();
    return sc;
}

extern "C" void stac_render_scene_destroy(stac_render_scene *sc) {
    if (!sc) return;
    DeviceGuard dg(sc->device);
    (void)hipFree(sc->d_int);
    (void)hipFree(sc->d_float);
    (void)hipFree(sc->d_scene);
    if (sc->d_nodes) (void)hipFree(sc->d_nodes);
    if (sc->d_tris) (void)hipFree(sc->d_tris);
    delete sc;
}

extern "C" int32_t stac_render(const stac_render_scene *sc, int32_t N, const float *xpos, const float *xquat, const float *kp,
                               const float *markers, int32_t show_error, const float *cam, float tan_half_fovy, int32_t width,
                               int32_t height, uint8_t *rgb_out, int32_t *seg_out, float *depth_out, void *stream) {
    if (!sc || N < 0 || width < 1 || height < 1 || width > 32768 || height > 32768 || !(tan_half_fovy > 0.0f) ||
        !(tan_half_fovy < INFINITY) || (N > 0 && (!xpos || !xquat || !cam)))
        return fail(STAC_ERR_INVALID, "stac_render: bad argument");
    DeviceGuard dg(sc->device);
    RenderCall C{};
    C.N = N; C.W = width; C.H = height; C.show_error = show_error ? 1 : 0;
    C.xpos = xpos; C.xquat = xquat; C.kp = kp; C.markers = markers; C.cam = cam; C.tanh = tan_half_fovy;
    C.rgb = rgb_out; C.seg = seg_out; C.depth = depth_out;
    return launch_result("stac_render", launch_render(sc->d_scene, C, sc->has_mesh, (hipStream_t)stream));
}
