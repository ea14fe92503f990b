/*
 * render_ref.c -- CPU restatement of the frame rule of DESIGN.md "Rendering", mesh geoms included, and of the arithmetic of
 * stac_mjx_amd/csrc/stac_render.hip (TEST INFRASTRUCTURE ONLY): the one checker of the render kernel, render_kernel<false>
 * and render_kernel<true> alike.
 *
 * A mesh instance (type 7) is walked through the hierarchy arrays of stac_render_meshes exactly as the kernel walks them
 * (rr_render), or tested triangle by triangle with the hierarchy ignored (rr_render_brute).  A scene without meshes has
 * nmesh = 0 and null mesh pointers.
 *
 * Built twice by tests/tools/build_render_ref.py:
 *   -DRR_REAL=float : the kernel's operation order, operation by operation (no FMA, -ffp-contract=off): the
 *                     tolerance-0 checker of the GPU tests;
 *   -DRR_REAL=double: the same rule evaluated in double, the independent evaluation.  It also flags the pixels
 *                     whose outcome float32 rounding can flip (rr_render's `amb`, see compare_builds in tests/render_cases.py).
 * It does not cull: it only skips a primitive whose bounding sphere misses the ray by a generous margin, tested
 * in double.  Rows run in parallel with OpenMP.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#ifndef RR_REAL
#define RR_REAL float
#endif
typedef RR_REAL real;

#define IS_F32 (sizeof(real) == 4)
#define R_(x) ((real)(x))
#define SQRT(x) (IS_F32 ? (real)sqrtf((float)(x)) : (real)sqrt((double)(x)))
#define FLOOR(x) (IS_F32 ? (real)floorf((float)(x)) : (real)floor((double)(x)))
#define FABS(x) (IS_F32 ? (real)fabsf((float)(x)) : (real)fabs((double)(x)))
static real rmax(real a, real b) { return IS_F32 ? (real)fmaxf((float)a, (float)b) : (real)fmax((double)a, (double)b); }
static real rmin(real a, real b) { return IS_F32 ? (real)fminf((float)a, (float)b) : (real)fmin((double)a, (double)b); }

/* margin of a hit test against float32 rounding: 64 x 2^-24 */
#define AMB_TOL (64.0 / 16777216.0)

enum { T_NONE = -1, T_PLANE = 0, T_SPHERE = 2, T_CAPSULE = 3, T_ELLIPSOID = 4, T_CYLINDER = 5, T_BOX = 6, T_MESH = 7 };
#define MESH_PAD R_(1.0 / 65536.0)
enum { F_TRANSPARENT = 1, F_CHECKER = 2, F_TEXUNIFORM = 4 };
#define LAYERS 8
#define MAXP 512

typedef struct {
    int nprim, nbody, nkp, nlight;
    const int32_t *prim_type, *prim_body, *prim_flags;
    const float *prim_size, *prim_pos, *prim_quat, *prim_rgba, *prim_rgb2, *prim_tex;
    const float *kp_rgba, *light_dir, *light_diff;
    float marker_rgba[4], seg_rgba[4];
    float marker_r, seg_r;
    float head_amb[3], head_diff[3];
    float alpha;
    float bg[3];
    /* stac_render_meshes */
    int nmesh;
    const int32_t *node_offset, *tri_offset;
    const float *node_box;
    const int32_t *node_link;
    const float *tri_vertex;
    const int32_t *prim_mesh;
} rr_scene;

typedef struct {
    real c[3], R[9], sz[3], brad;
    int type, flags;
    int mesh;  /* a mesh: sz = world position of the geom frame's origin, c = world centre of the root box */
    real mag;
} rec_t;

static real dot3(const real *a, const real *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static real dot3f(const real *a, const float *b) { return a[0] * R_(b[0]) + a[1] * R_(b[1]) + a[2] * R_(b[2]); }

static void quat_mat(const float *qf, real *R) {
    const real w = R_(qf[0]), x = R_(qf[1]), y = R_(qf[2]), z = R_(qf[3]);
    const real ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    const real wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
    R[0] = ww + xx - yy - zz; R[1] = R_(2) * (xy - wz);   R[2] = R_(2) * (xz + wy);
    R[3] = R_(2) * (xy + wz); R[4] = ww - xx + yy - zz;   R[5] = R_(2) * (yz - wx);
    R[6] = R_(2) * (xz - wy); R[7] = R_(2) * (yz + wx);   R[8] = ww - xx - yy + zz;
}
static void mat_tvec(const real *R, const real *v, real *out) {
    for (int j = 0; j < 3; ++j) out[j] = R[j] * v[0] + R[3 + j] * v[1] + R[6 + j] * v[2];
}
static void mat_vec(const real *R, const real *v, real *out) {
    for (int i = 0; i < 3; ++i) out[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2];
}
static int finite3(const float *p) { return p[0] == p[0] && p[1] == p[1] && p[2] == p[2]; }

static void build_prim(const rr_scene *S, int f, int i, const float *xpos, const float *xquat, const float *kp,
                       const float *markers, int show_error, rec_t *r) {
    int type = T_NONE, flags = 0;
    real c[3] = {0, 0, 0}, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, sz[3] = {0, 0, 0}, brad = 0;
    r->mesh = -1; r->mag = 0;
    const int P = S->nprim, K = S->nkp;
    if (i < P) {
        type = S->prim_type[i];
        flags = S->prim_flags[i];
        const int b = S->prim_body[i];
        const float *xp = xpos + ((size_t)f * S->nbody + b) * 3;
        real Rb[9], Rl[9], lp[3], pp[3];
        quat_mat(xquat + ((size_t)f * S->nbody + b) * 4, Rb);
        quat_mat(S->prim_quat + 4 * i, Rl);
        for (int a = 0; a < 3; ++a)
            for (int q = 0; q < 3; ++q) R[3 * a + q] = Rb[3 * a] * Rl[q] + Rb[3 * a + 1] * Rl[3 + q] + Rb[3 * a + 2] * Rl[6 + q];
        for (int a = 0; a < 3; ++a) pp[a] = R_(S->prim_pos[3 * i + a]);
        mat_vec(Rb, pp, lp);
        for (int a = 0; a < 3; ++a) { c[a] = R_(xp[a]) + lp[a]; sz[a] = R_(S->prim_size[3 * i + a]); }
        if (type == T_MESH) {
            const int mi = S->prim_mesh[i];
            const float *nd = S->node_box + 6 * (size_t)S->node_offset[mi];
            real bc[3], he[3], wc[3], mag = 0;
            for (int a = 0; a < 3; ++a) {
                bc[a] = (R_(nd[a]) + R_(nd[3 + a])) * R_(0.5);
                he[a] = (R_(nd[3 + a]) - R_(nd[a])) * R_(0.5);
                mag = mag + rmax(FABS(R_(nd[a])), FABS(R_(nd[3 + a])));
            }
            mat_vec(R, bc, wc);
            for (int a = 0; a < 3; ++a) { sz[a] = c[a]; c[a] = c[a] + wc[a]; }
            brad = SQRT(dot3(he, he));
            r->mesh = mi;
            r->mag = mag;
        }
    } else if (i < P + K) {
        if (kp) {
            const float *p = kp + ((size_t)f * K + (i - P)) * 3;
            if (finite3(p)) { type = T_SPHERE; for (int q = 0; q < 3; ++q) c[q] = R_(p[q]); sz[0] = R_(S->marker_r); }
        }
    } else if (i < P + 2 * K) {
        if (markers) {
            const float *p = markers + ((size_t)f * K + (i - P - K)) * 3;
            if (finite3(p)) { type = T_SPHERE; for (int q = 0; q < 3; ++q) c[q] = R_(p[q]); sz[0] = R_(S->marker_r); }
        }
    } else {
        const int k = i - P - 2 * K;
        if (show_error && kp && markers) {
            const float *a = kp + ((size_t)f * K + k) * 3, *m = markers + ((size_t)f * K + k) * 3;
            if (finite3(a) && finite3(m)) {
                real d[3] = {R_(m[0]) - R_(a[0]), R_(m[1]) - R_(a[1]), R_(m[2]) - R_(a[2])};
                const real len = SQRT(dot3(d, d));
                real w[3] = {0, 0, 1};
                if (len > 0) { w[0] = d[0] / len; w[1] = d[1] / len; w[2] = d[2] / len; }
                type = T_CAPSULE;
                for (int q = 0; q < 3; ++q) c[q] = R_(a[q]) + d[q] * R_(0.5);
                R[2] = w[0]; R[5] = w[1]; R[8] = w[2];
                sz[0] = R_(S->seg_r);
                sz[1] = R_(0.5) * len;
            }
        }
    }
    if (type == T_SPHERE) brad = sz[0];
    else if (type == T_ELLIPSOID) brad = rmax(sz[0], rmax(sz[1], sz[2]));
    else if (type == T_CAPSULE) brad = sz[1] + sz[0];
    else if (type == T_CYLINDER || type == T_PLANE) brad = SQRT(sz[0] * sz[0] + sz[1] * sz[1]);
    else if (type == T_BOX) brad = SQRT(dot3(sz, sz));
    memcpy(r->c, c, sizeof c); memcpy(r->R, R, sizeof R); memcpy(r->sz, sz, sizeof sz);
    r->brad = brad; r->type = type; r->flags = flags;
}

/* amb: set when a decision below is within AMB_TOL of flipping (margin <= AMB_TOL x condition number) */
static void flag(int *amb, double margin, double scale) {
    if (fabs(margin) <= AMB_TOL * scale) *amb = 1;
}

static real hit_sphere(const real *ctr, real rad, const real *o, const real *d, real dd, int *amb) {
    const real oc[3] = {o[0] - ctr[0], o[1] - ctr[1], o[2] - ctr[2]};
    const real tca = -dot3(oc, d) / dd;
    const real p[3] = {oc[0] + d[0] * tca, oc[1] + d[1] * tca, oc[2] + d[2] * tca};
    const real h2 = rad * rad - dot3(p, p);
    /* quadric: margin |h2| / r^2, condition number |o - c| / r */
    flag(amb, (double)h2, sqrt((double)dot3(oc, oc)) * (double)rad);
    if (!(h2 >= 0)) return -1;
    const real t = tca - SQRT(h2 / dd);
    flag(amb, (double)t, sqrt((double)dot3(oc, oc)));
    return t > 0 ? t : -1;
}

static real intersect(const rec_t *r, const real *o, const real *d, real dd, int *face, int *amb) {
    const int type = r->type;
    const real *c = r->c, *R = r->R, *sz = r->sz;
    *face = 0;
    if (type == T_SPHERE) return hit_sphere(c, sz[0], o, d, dd, amb);
    const real oc[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
    const double ocn = sqrt((double)dot3(oc, oc));
    if (type == T_CAPSULE) {
        const real w[3] = {R[2], R[5], R[8]};
        const real hl = sz[1], rad = sz[0];
        const real oz = dot3(oc, w), dz = dot3(d, w);
        /* an origin inside the capsule does not see it: nearer to the axis point at oz clamped to the segment than rad */
        const real ozc = rmin(rmax(oz, -hl), hl);
        const real oq[3] = {oc[0] - w[0] * ozc, oc[1] - w[1] * ozc, oc[2] - w[2] * ozc};
        const real in2 = rad * rad - dot3(oq, oq);
        flag(amb, (double)in2, ocn * (double)rad);
        if (in2 > 0) return -1;
        const real op[3] = {oc[0] - w[0] * oz, oc[1] - w[1] * oz, oc[2] - w[2] * oz};
        const real dp[3] = {d[0] - w[0] * dz, d[1] - w[1] * dz, d[2] - w[2] * dz};
        const real a = dot3(dp, dp);
        real best = (real)INFINITY;
        if (a > 0) {
            const real tca = -dot3(op, dp) / a;
            const real p[3] = {op[0] + dp[0] * tca, op[1] + dp[1] * tca, op[2] + dp[2] * tca};
            const real h2 = rad * rad - dot3(p, p);
            flag(amb, (double)h2, ocn * (double)rad);
            if (h2 >= 0) {
                const real t = tca - SQRT(h2 / a);
                const real z = oz + dz * t;
                flag(amb, (double)(FABS(z) - hl), ocn);
                if (t > 0 && FABS(z) <= hl) best = t;
            }
        }
        for (int s = 0; s < 2; ++s) {
            const real e = s == 0 ? hl : -hl;
            const real ctr[3] = {c[0] + w[0] * e, c[1] + w[1] * e, c[2] + w[2] * e};
            const real t = hit_sphere(ctr, rad, o, d, dd, amb);
            if (t > 0 && best < (real)INFINITY) flag(amb, (double)(t - best), ocn);
            if (t > 0 && t < best) { best = t; *face = 1 + s; }
        }
        return best < (real)INFINITY ? best : -1;
    }
    real ol[3], dl[3];
    mat_tvec(R, oc, ol);
    mat_tvec(R, d, dl);
    if (type == T_ELLIPSOID) {
        const real os[3] = {ol[0] / sz[0], ol[1] / sz[1], ol[2] / sz[2]};
        const real ds[3] = {dl[0] / sz[0], dl[1] / sz[1], dl[2] / sz[2]};
        const real a = dot3(ds, ds);
        const real tca = -dot3(os, ds) / a;
        const real p[3] = {os[0] + ds[0] * tca, os[1] + ds[1] * tca, os[2] + ds[2] * tca};
        const real h2 = 1 - dot3(p, p);
        flag(amb, (double)h2, sqrt((double)dot3(os, os)));  /* unit sphere: margin |h2|, condition |o - c| in radii */
        if (!(h2 >= 0)) return -1;
        const real t = tca - SQRT(h2 / a);
        flag(amb, (double)t, ocn);
        return t > 0 ? t : -1;
    }
    if (type == T_PLANE) {
        if (!(ol[2] > 0 && dl[2] < 0)) return -1;
        const real t = -ol[2] / dl[2];
        const real x = ol[0] + dl[0] * t, y = ol[1] + dl[1] * t;
        flag(amb, (double)(FABS(x) - sz[0]), ocn + fabs((double)t));
        flag(amb, (double)(FABS(y) - sz[1]), ocn + fabs((double)t));
        return (t > 0 && FABS(x) <= sz[0] && FABS(y) <= sz[1]) ? t : -1;
    }
    if (type == T_BOX) {
        real tn = -(real)INFINITY, tf = (real)INFINITY, tn2 = -(real)INFINITY;
        int ax = -1;
        for (int k = 0; k < 3; ++k) {
            if (dl[k] == 0) {
                if (FABS(ol[k]) > sz[k]) return -1;
            } else {
                const real t1 = (-sz[k] - ol[k]) / dl[k], t2 = (sz[k] - ol[k]) / dl[k];
                const real lo = t1 < t2 ? t1 : t2, hi = t1 < t2 ? t2 : t1;
                if (lo > tn) { tn2 = tn; tn = lo; ax = k; } else if (lo > tn2) tn2 = lo;
                if (hi < tf) tf = hi;
            }
        }
        *face = ax;
        if (ax >= 0) {
            flag(amb, (double)(tf - tn), ocn);             /* slab overlap */
            if (tn <= tf && tn > 0 && tn2 > -(real)INFINITY) flag(amb, (double)(tn - tn2), ocn);  /* which face */
            flag(amb, (double)tn, ocn);
        }
        return (ax >= 0 && tn <= tf && tn > 0) ? tn : -1;
    }
    if (type == T_CYLINDER) {
        const real rad = sz[0], hl = sz[1];
        real best = (real)INFINITY;
        const real a = dl[0] * dl[0] + dl[1] * dl[1];
        if (a > 0) {
            const real tca = -(ol[0] * dl[0] + ol[1] * dl[1]) / a;
            const real px = ol[0] + dl[0] * tca, py = ol[1] + dl[1] * tca;
            const real h2 = rad * rad - (px * px + py * py);
            flag(amb, (double)h2, ocn * (double)rad);
            if (h2 >= 0) {
                const real t = tca - SQRT(h2 / a);
                const real z = ol[2] + dl[2] * t;
                flag(amb, (double)(FABS(z) - hl), ocn);
                if (t > 0 && FABS(z) <= hl) best = t;
            }
        }
        for (int s = 0; s < 2; ++s) {
            const real e = s == 0 ? hl : -hl;
            const int facing = s == 0 ? (ol[2] > hl && dl[2] < 0) : (ol[2] < -hl && dl[2] > 0);
            if (facing) {
                const real t = (e - ol[2]) / dl[2];
                const real x = ol[0] + dl[0] * t, y = ol[1] + dl[1] * t;
                flag(amb, (double)(x * x + y * y - rad * rad), ocn * (double)rad);
                if (t > 0 && x * x + y * y <= rad * rad && t < best) { best = t; *face = 1 + s; }
            }
        }
        return best < (real)INFINITY ? best : -1;
    }
    return -1;
}

/* One triangle of the mesh against the geom-frame ray ol + t dl; updates (best, btri).  amb: the barycentric sign tests,
 * t > 0 and the tie with the best hit so far, each against 64 x 2^-24 times its condition number: the numerators are
 * formed from ao = ol - v0 (error about eps (|ol| + |v0|)) times an edge, divided by det. */
static void hit_tri(const float *v, int ti, const real *ol, const real *dl, real *best, int *btri, int *bill, int *amb) {
    int ill = 0;
    const real v0[3] = {R_(v[0]), R_(v[1]), R_(v[2])};
    const real e1[3] = {R_(v[3]) - v0[0], R_(v[4]) - v0[1], R_(v[5]) - v0[2]};
    const real e2[3] = {R_(v[6]) - v0[0], R_(v[7]) - v0[1], R_(v[8]) - v0[2]};
    const real N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const real det = -dot3(dl, N);
    if (det == 0) return;
    const real inv = R_(1) / det;
    const real ao[3] = {ol[0] - v0[0], ol[1] - v0[1], ol[2] - v0[2]};
    const real dao[3] = {ao[1] * dl[2] - ao[2] * dl[1], ao[2] * dl[0] - ao[0] * dl[2], ao[0] * dl[1] - ao[1] * dl[0]};
    const real bu = dot3(e2, dao) * inv;
    const real bv = -dot3(e1, dao) * inv;
    const real t = dot3(ao, N) * inv;
    {
        const double A = sqrt((double)dot3(ol, ol)) + sqrt((double)dot3(v0, v0)) + sqrt((double)dot3(ao, ao));
        const double l1 = sqrt((double)dot3(e1, e1)), l2 = sqrt((double)dot3(e2, e2)), ln = sqrt((double)dot3(N, N));
        const double ad = fabs((double)det);
        const int near_in = (double)bu >= -0.5 && (double)bv >= -0.5 && (double)(bu + bv) <= 1.5;  /* far misses cannot flip */
        if (near_in) {
            const int in_u = bu >= 0, in_v = bv >= 0, in_w = bu + bv <= 1;
            /* a sign test matters when the other two hold (or are themselves close: they get flagged on their own) */
            if (in_v && in_w) flag(amb, (double)bu, A * l2 / ad + fabs((double)bu));
            if (in_u && in_w) flag(amb, (double)bv, A * l1 / ad + fabs((double)bv));
            if (in_u && in_v) flag(amb, 1.0 - (double)(bu + bv), A * (l1 + l2) / ad + 1.0);
            if (in_u && in_v && in_w) {
                flag(amb, (double)t, A * ln / ad);
                if (*btri >= 0 && t > 0) flag(amb, (double)(t - *best), A * ln / ad + fabs((double)t));
                /* depth of a grazing hit.  t = (ao . N) / det cancels in both dot products when the ray runs nearly in
                 * the triangle's plane: ao carries an absolute error of about 4 eps A, the numerator 3 more roundings,
                 * det about 8 eps |N|, so the relative error of t is bounded by 8 eps (A / t + 1) |N| / |det|.  Where
                 * that bound exceeds the 1e-5 that compare_builds allows a depth, float32 cannot give the depth: the pixel
                 * is flagged if this hit becomes its depth (*bill, see render). */
                if (t > 0 && 8.0 / 16777216.0 * (A / (double)t + 1.0) * ln / ad > 1e-5) ill = 1;
            }
        }
    }
    if (bu >= 0 && bv >= 0 && bu + bv <= 1 && t > 0 && (t < *best || (t == *best && ti < *btri))) {
        *best = t;
        *btri = ti;
        *bill = ill;
    }
}

/* The kernel's hit_mesh; brute != 0 ignores the hierarchy and tests every triangle of the mesh in index order. */
static real hit_mesh(const rr_scene *S, const rec_t *r, const real *o, const real *d, int brute, int *tri, int *ill, int *amb) {
    const real *R = r->R, *org = r->sz;
    const int mi = r->mesh;
    const real oc[3] = {o[0] - org[0], o[1] - org[1], o[2] - org[2]};
    real ol[3], dl[3];
    mat_tvec(R, oc, ol);
    mat_tvec(R, d, dl);
    const real pad = (FABS(ol[0]) + FABS(ol[1]) + FABS(ol[2]) + r->mag) * MESH_PAD;
    const real idl[3] = {R_(1) / dl[0], R_(1) / dl[1], R_(1) / dl[2]};
    const int n0 = S->node_offset[mi], nn = S->node_offset[mi + 1] - n0;
    const float *box = S->node_box + 6 * (size_t)n0;
    const int32_t *link = S->node_link + 3 * (size_t)n0;
    const float *tris = S->tri_vertex + 9 * (size_t)S->tri_offset[mi];
    const int nt = S->tri_offset[mi + 1] - S->tri_offset[mi];
    real best = (real)INFINITY;
    int btri = -1;
    if (brute) {
        for (int ti = 0; ti < nt; ++ti) hit_tri(tris + 9 * (size_t)ti, ti, ol, dl, &best, &btri, ill, amb);
    } else {
        int n = 0;
        while (n < nn) {
            const float *b = box + 6 * (size_t)n;
            real tn = -(real)INFINITY, tf = (real)INFINITY;
            for (int k = 0; k < 3; ++k) {
                const real t1 = ((R_(b[k]) - pad) - ol[k]) * idl[k], t2 = ((R_(b[3 + k]) + pad) - ol[k]) * idl[k];
                const real lo_t = t1 < t2 ? t1 : t2, hi_t = t1 < t2 ? t2 : t1;
                if (lo_t > tn) tn = lo_t;
                if (hi_t < tf) tf = hi_t;
            }
            if (!(tn <= tf && tf > 0 && tn <= best)) { n = link[3 * n]; continue; }
            const int first = link[3 * n + 1], count = link[3 * n + 2];
            if (count == 0) { n = n + 1; continue; }
            for (int k = 0; k < count; ++k) hit_tri(tris + 9 * (size_t)(first + k), first + k, ol, dl, &best, &btri, ill, amb);
            n = link[3 * n];
        }
    }
    *tri = btri;
    return btri >= 0 ? best : -1;
}

static void normal_at(const rr_scene *S, const rec_t *r, const real *o, const real *d, real t, int face, int tri, real *n) {
    const int type = r->type;
    const real *c = r->c, *R = r->R, *sz = r->sz;
    const real q[3] = {o[0] + d[0] * t - c[0], o[1] + d[1] * t - c[1], o[2] + d[2] * t - c[2]};
    real v[3];
    if (type == T_SPHERE) {
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
    } else if (type == T_CAPSULE) {
        const real w[3] = {R[2], R[5], R[8]};
        const real z = face == 0 ? dot3(q, w) : (face == 1 ? sz[1] : -sz[1]);
        v[0] = q[0] - w[0] * z; v[1] = q[1] - w[1] * z; v[2] = q[2] - w[2] * z;
    } else if (type == T_PLANE) {
        v[0] = R[2]; v[1] = R[5]; v[2] = R[8];
    } else if (type == T_MESH) {
        const float *p = S->tri_vertex + 9 * ((size_t)S->tri_offset[r->mesh] + (size_t)tri);
        const real e1[3] = {R_(p[3]) - R_(p[0]), R_(p[4]) - R_(p[1]), R_(p[5]) - R_(p[2])};
        const real e2[3] = {R_(p[6]) - R_(p[0]), R_(p[7]) - R_(p[1]), R_(p[8]) - R_(p[2])};
        real N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        real dl[3];
        mat_tvec(R, d, dl);
        if (dot3(dl, N) > 0) { N[0] = -N[0]; N[1] = -N[1]; N[2] = -N[2]; }
        mat_vec(R, N, v);
    } else {
        real ql[3], nl[3];
        mat_tvec(R, q, ql);
        if (type == T_ELLIPSOID) {
            nl[0] = ql[0] / (sz[0] * sz[0]); nl[1] = ql[1] / (sz[1] * sz[1]); nl[2] = ql[2] / (sz[2] * sz[2]);
        } else if (type == T_BOX) {
            real dl[3];
            mat_tvec(R, d, dl);
            nl[0] = 0; nl[1] = 0; nl[2] = 0;
            const real sgn = (face == 0 ? dl[0] : (face == 1 ? dl[1] : dl[2])) < 0 ? R_(1) : R_(-1);
            if (face == 0) nl[0] = sgn; else if (face == 1) nl[1] = sgn; else nl[2] = sgn;
        } else {
            nl[0] = face == 0 ? ql[0] : 0;
            nl[1] = face == 0 ? ql[1] : 0;
            nl[2] = face == 0 ? 0 : (face == 1 ? R_(1) : R_(-1));
        }
        mat_vec(R, nl, v);
    }
    const real len = SQRT(dot3(v, v));
    n[0] = v[0] / len; n[1] = v[1] / len; n[2] = v[2] / len;
}

static void shade(const rr_scene *S, const rec_t *r, int id, const real *o, const real *d, real t, int face, int tri,
                  const real *zc, real *col, int *amb) {
    real n[3], rgb[3];
    normal_at(S, r, o, d, t, face, tri, n);
    const int P = S->nprim, K = S->nkp;
    if (id < P) {
        const float *c1 = S->prim_rgba + 4 * id;
        rgb[0] = R_(c1[0]); rgb[1] = R_(c1[1]); rgb[2] = R_(c1[2]);
        if (r->flags & F_CHECKER) {
            const real *c = r->c, *R = r->R, *sz = r->sz;
            const real q[3] = {o[0] + d[0] * t - c[0], o[1] + d[1] * t - c[1], o[2] + d[2] * t - c[2]};
            real ql[3];
            mat_tvec(R, q, ql);
            const float *rep = S->prim_tex + 2 * id;
            const int uni = (r->flags & F_TEXUNIFORM) != 0;
            const real su = uni ? R_(1) : R_(2) * sz[0], sv = uni ? R_(1) : R_(2) * sz[1];
            const real u = ql[0] * R_(rep[0]) / su;
            const real v = ql[1] * R_(rep[1]) / sv;
            /* checker edge: |2u - nearest integer| against the rounding of 2u (|o - c| scaled to texture units) */
            const double ocn = sqrt((double)dot3(q, q)) + sqrt((double)(dot3(o, o))) + sqrt((double)dot3(c, c));
            flag(amb, 2.0 * (double)u - floor(2.0 * (double)u + 0.5), fabs(2.0 * (double)u) + 2.0 * rep[0] * ocn / (double)su);
            flag(amb, 2.0 * (double)v - floor(2.0 * (double)v + 0.5), fabs(2.0 * (double)v) + 2.0 * rep[1] * ocn / (double)sv);
            const int cell = (int)FLOOR(R_(2) * u) + (int)FLOOR(R_(2) * v);
            if (cell & 1) {
                const float *c2 = S->prim_rgb2 + 3 * id;
                rgb[0] = R_(c2[0]); rgb[1] = R_(c2[1]); rgb[2] = R_(c2[2]);
            }
        }
    } else if (id < P + K) {
        const float *c1 = S->kp_rgba + 4 * (id - P);
        rgb[0] = R_(c1[0]); rgb[1] = R_(c1[1]); rgb[2] = R_(c1[2]);
    } else if (id < P + 2 * K) {
        for (int q = 0; q < 3; ++q) rgb[q] = R_(S->marker_rgba[q]);
    } else {
        for (int q = 0; q < 3; ++q) rgb[q] = R_(S->seg_rgba[q]);
    }
    const real ch = rmax(dot3(n, zc), 0);
    real L[3];
    for (int q = 0; q < 3; ++q) L[q] = R_(S->head_amb[q]) + R_(S->head_diff[q]) * ch;
    for (int l = 0; l < S->nlight; ++l) {
        const real cl = rmax(-dot3f(n, S->light_dir + 3 * l), 0);
        for (int q = 0; q < 3; ++q) L[q] = L[q] + R_(S->light_diff[3 * l + q]) * cl;
    }
    for (int q = 0; q < 3; ++q) col[q] = rgb[q] * rmin(L[q], 1);
}

static uint8_t quant(real c) {
    const real x = c < 0 ? R_(0) : (c > 1 ? R_(1) : c);
    return (uint8_t)(int)FLOOR(x * R_(255) + R_(0.5));
}

typedef struct { real t; int id, face, tri; } hit_t;

static int hit_less(const hit_t *a, const hit_t *b) { return a->t < b->t || (a->t == b->t && a->id < b->id); }

/* Renders N frames; rgb [N,H,W,3], seg [N,H,W], depth [N,H,W], amb [N,H,W] (each may be NULL).  Returns 0. */
static int render(const rr_scene *S, int N, const float *xpos, const float *xquat, const float *kp, const float *markers,
                  int show_error, const float *cam, float tanhf_, int W, int H, uint8_t *rgb, int32_t *seg, float *depth,
                  uint8_t *ambout, int brute) {
    const int Ptot = S->nprim + 3 * S->nkp;
    if (Ptot > MAXP) return -3;
    rec_t *recs = (rec_t *)malloc(sizeof(rec_t) * (Ptot > 0 ? Ptot : 1));
    for (int f = 0; f < N; ++f) {
        for (int i = 0; i < Ptot; ++i) build_prim(S, f, i, xpos, xquat, kp, markers, show_error, &recs[i]);
        const float *cm = cam + (size_t)f * 12;
        const real tv = R_(tanhf_), tu = R_(tanhf_) * ((real)W / (real)H);
#pragma omp parallel for schedule(dynamic, 4)
        for (int y = 0; y < H; ++y) {
            hit_t tr[MAXP];
            for (int x = 0; x < W; ++x) {
                int amb = 0;
                const real o[3] = {R_(cm[0]), R_(cm[1]), R_(cm[2])};
                real Rc[9];
                for (int q = 0; q < 9; ++q) Rc[q] = R_(cm[3 + q]);
                const real u = (((real)x + R_(0.5)) * R_(2) / (real)W - R_(1)) * tu;
                const real v = (R_(1) - ((real)y + R_(0.5)) * R_(2) / (real)H) * tv;
                real d[3];
                for (int q = 0; q < 3; ++q) d[q] = Rc[3 * q] * u + Rc[3 * q + 1] * v - Rc[3 * q + 2];
                {
                    const real len = SQRT(dot3(d, d));
                    d[0] = d[0] / len; d[1] = d[1] / len; d[2] = d[2] / len;
                }
                const real dd = dot3(d, d);
                real to = (real)INFINITY, to2 = (real)INFINITY;
                int io = -1, fo = 0, tro = 0, nt = 0, to_ill = 0;
                for (int i = 0; i < Ptot; ++i) {
                    const rec_t *r = &recs[i];
                    if (r->type == T_NONE) continue;
                    /* skip only what misses by far: bounding sphere vs the ray, in double, margin 1 % + 1e-6 */
                    double w[3], dn[3], wd = 0, ww = 0;
                    for (int q = 0; q < 3; ++q) { w[q] = (double)r->c[q] - (double)o[q]; dn[q] = (double)d[q]; }
                    for (int q = 0; q < 3; ++q) { wd += w[q] * dn[q]; ww += w[q] * w[q]; }
                    const double br = (double)r->brad * 1.01 + 1e-6 + 1e-6 * sqrt(ww);
                    if (wd < -br) continue;
                    if (ww - wd * wd > br * br) continue;
                    int face, tri = 0, ill = 0;
                    const real t = r->type == T_MESH ? (face = 0, hit_mesh(S, r, o, d, brute, &tri, &ill, &amb))
                                                     : intersect(r, o, d, dd, &face, &amb);
                    if (!(t > 0)) continue;
                    if (r->flags & F_TRANSPARENT) {
                        tr[nt].t = t; tr[nt].id = i; tr[nt].face = face; tr[nt].tri = tri; ++nt;
                    } else if (t < to || (t == to && i < io)) {
                        to2 = to;
                        to = t; io = i; fo = face; tro = tri; to_ill = ill;
                    } else if (t < to2) {
                        to2 = t;
                    }
                }
                if (io >= 0 && to_ill) amb = 1;  /* the depth is a grazing mesh hit's: see hit_tri */
                /* depth ties between the two nearest opaque hits: relative gap */
                if (io >= 0 && to2 < (real)INFINITY) flag(&amb, (double)(to2 - to), (double)to);
                /* the LAYERS nearest transparent hits by (t, id) */
                for (int a = 1; a < nt; ++a) {
                    hit_t h = tr[a];
                    int b = a - 1;
                    while (b >= 0 && hit_less(&h, &tr[b])) { tr[b + 1] = tr[b]; --b; }
                    tr[b + 1] = h;
                }
                for (int a = 0; a < nt && a <= LAYERS; ++a) {
                    if (a > 0) flag(&amb, (double)(tr[a].t - tr[a - 1].t), (double)tr[a].t);
                    if (io >= 0) flag(&amb, (double)(tr[a].t - to), (double)to);
                }
                const real zc[3] = {Rc[2], Rc[5], Rc[8]};
                real col[3] = {R_(S->bg[0]), R_(S->bg[1]), R_(S->bg[2])};
                if (io >= 0) shade(S, &recs[io], io, o, d, to, fo, tro, zc, col, &amb);
                const real a = R_(S->alpha), na = R_(1) - R_(S->alpha);
                for (int k = (nt < LAYERS ? nt : LAYERS) - 1; k >= 0; --k) {
                    if (tr[k].t < to) {
                        real s[3];
                        shade(S, &recs[tr[k].id], tr[k].id, o, d, tr[k].t, tr[k].face, tr[k].tri, zc, s, &amb);
                        for (int q = 0; q < 3; ++q) col[q] = col[q] * na + s[q] * a;
                    }
                }
                const size_t px = ((size_t)f * H + y) * W + x;
                if (rgb) for (int q = 0; q < 3; ++q) rgb[3 * px + q] = quant(col[q]);
                if (seg) seg[px] = io;
                if (depth) depth[px] = (float)to;
                if (ambout) ambout[px] = (uint8_t)amb;
            }
        }
    }
    free(recs);
    return 0;
}

int rr_render(const rr_scene *S, int N, const float *xpos, const float *xquat, const float *kp, const float *markers,
              int show_error, const float *cam, float tanhf_, int W, int H, uint8_t *rgb, int32_t *seg, float *depth,
              uint8_t *ambout) {
    return render(S, N, xpos, xquat, kp, markers, show_error, cam, tanhf_, W, H, rgb, seg, depth, ambout, 0);
}

/* The same picture with the hierarchy ignored: every triangle of every mesh instance is tested. */
int rr_render_brute(const rr_scene *S, int N, const float *xpos, const float *xquat, const float *kp, const float *markers,
                    int show_error, const float *cam, float tanhf_, int W, int H, uint8_t *rgb, int32_t *seg, float *depth,
                    uint8_t *ambout) {
    return render(S, N, xpos, xquat, kp, markers, show_error, cam, tanhf_, W, H, rgb, seg, depth, ambout, 1);
}
