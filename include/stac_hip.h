/*
 * stac_hip.h -- C ABI of the MI355X-native STAC pose-fitting engine (libstac_hip.so).
 *
 * This is the drop-in boundary for the hot path of talmolab/stac-mjx: the solver seam
 * `StacCore.q_opt / StacCore.m_opt` (stac_mjx/stac_core.py:175-275) and, one level up, the three
 * phase drivers of stac_mjx/compute_stac.py that call it once per frame (:17-104, :107-167,
 * :170-278) and that `Stac.ik_only` vmaps over clips (stac_mjx/stac.py:405-440).
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in the signatures (`stream` is a hipStream_t passed
 *     as void*; NULL = the default stream).
 *   - every `float*` / `uint32_t*` data argument is a DEVICE pointer owned by the caller (e.g. a
 *     PyTorch-ROCm tensor) unless the comment says "host".  The library never frees caller memory.
 *   - all calls are asynchronous on `stream`.  Host-side waits, complete list: (1) a stac_q_solve / stac_q_phase
 *     call with a NEW set of masks (or stac_q_solve with new lb / ub) waits once for its own small table uploads
 *     on that stream (the host arrays are the caller's temporaries); (2) stac_fk / stac_q_phase called WITHOUT
 *     xpos / xquat outputs grow an internal scratch block to its high-water mark -- growing frees the old block,
 *     which waits for the device.  Launch control words are set by a kernel on the stream, every other buffer is
 *     allocated at stac_model_create.
 *   - a model belongs to the device that was current at stac_model_create; every entry point makes that device
 *     current for its duration and restores the caller's.
 *   - developer switches (STAC_HIP_* environment variables) are read once, at
 *     stac_model_create.
 *   - return value: 0 = OK, negative = error (see stac_last_error()); no exceptions cross the ABI.
 *   - layouts are C-contiguous float32; clip-major: kp[C][F][3K], qpos[C][F][nq].
 *   - re-entrant per model: one call at a time on a given stac_model, which owns scratch buffers for the launch in
 *     flight;
 *     no global state besides the thread-local error string.
 */
#ifndef STAC_HIP_H
#define STAC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STAC_HIP_ABI_VERSION 3

/* mjtJoint values (same as MuJoCo's, so tables from a MuJoCo compile can be passed as they are). */
enum { STAC_JNT_FREE = 0, STAC_JNT_BALL = 1, STAC_JNT_SLIDE = 2, STAC_JNT_HINGE = 3 };

enum {
    STAC_OK = 0,
    STAC_ERR_INVALID = -1,  /* bad argument */
    STAC_ERR_HIP = -2,      /* a HIP runtime call failed */
    STAC_ERR_CAPACITY = -3, /* model exceeds the compiled kernel limits */
    STAC_ERR_NO_DEVICE = -4 /* no usable GPU */
};

/* Flat kinematic model, HOST pointers, copied at stac_model_create.
 * Replaces what the reference gets from mjx.put_model(mj_model) (stac_mjx/utils.py:34-46) plus the
 * bounds of stac_mjx/stac.py:54-88.  Field meaning = MuJoCo's mjModel fields of the same name. */
typedef struct stac_model_tables {
    int32_t nbody, njnt, nq, nsite;  /* nsite = K fit sites (one per keypoint) */
    const int32_t *body_parentid;    /* [nbody]   */
    const float *body_pos;           /* [nbody,3] */
    const float *body_quat;          /* [nbody,4] w,x,y,z */
    const int32_t *body_jntadr;      /* [nbody]   (-1 if none) */
    const int32_t *body_jntnum;      /* [nbody]   */
    const int32_t *jnt_type;         /* [njnt]    */
    const int32_t *jnt_qposadr;      /* [njnt]    */
    const int32_t *jnt_bodyid;       /* [njnt]    */
    const float *jnt_pos;            /* [njnt,3]  */
    const float *jnt_axis;           /* [njnt,3]  unit */
    const float *qpos0;              /* [nq]      */
    const int32_t *site_bodyid;      /* [K]       */
    const float *site_pos;           /* [K,3]     initial marker offsets */
    const float *lb;                 /* [nq]  box bounds of the q_phase (stac.py:54-88) */
    const float *ub;                 /* [nq]  */
} stac_model_tables;

/* Solver hyper-parameters (host struct).  Replaces StacCore.__init__(tol, n_iter_q)
 * (stac_mjx/stac_core.py:182-191) and the jaxopt defaults it relies on. */
typedef struct stac_q_params {
    float tol;               /* FTOL: stop when ||clip(x - grad) - x||_2 <= tol */
    int32_t maxiter;         /* N_ITER_Q (>= 1) */
    int32_t maxls;           /* line-search halvings, jaxopt default 15 */
    int32_t lanes_per_chain; /* 0 = auto; else 8, 16, 32 or 64 lanes of a wavefront per chain (a width that is not built for
                                this model -- 4 always -- runs on the next wider one; results do not depend on it) */
    int32_t solver;          /* STAC_SOLVER_PG (the reference's algorithm, parity mode) or STAC_SOLVER_LM */
    float lm_lambda0;        /* LM only: initial damping (0 -> 1e-2); maxiter then counts accepted LM steps */
} stac_q_params;

/* STAC_SOLVER_LM is an optional fast solver, NOT the reference's algorithm: projected Levenberg-Marquardt on the
 * same objective, masks, bounds, stopping residual and sequencing (analytic site Jacobians, J^T J + damping,
 * Cholesky in LDS).  It fits the markers at least as well as the truncated projected gradient but does not
 * reproduce its iterates; it is available in stac_q_phase only. */
enum { STAC_SOLVER_PG = 0, STAC_SOLVER_LM = 1 };

typedef struct stac_model stac_model; /* opaque */

/* Thread-local description of the last error returned on this thread ("" if none). */
const char *stac_last_error(void);
/* Its status code (STAC_ERR_*; 0 if none): what a NULL from stac_model_create does not carry. */
int32_t stac_last_error_code(void);
int32_t stac_abi_version(void);
/* Number of visible GPUs (0 if none); does not initialise a device. */
int32_t stac_device_count(void);

/* Uploads the tables to the current device.  Returns NULL on failure (see stac_last_error). */
stac_model *stac_model_create(const stac_model_tables *host_tables);
void stac_model_destroy(stac_model *m);
/* info[8] (host) = {nbody, njnt, nq, K, n_active_bodies, n_active_joints, n_levels, max_lanes_hint} */
int32_t stac_model_info(const stac_model *m, int32_t *info);

/* utils.set_site_pos / get_site_pos (stac_mjx/utils.py:93-126): offsets[K,3] device pointer. */
int32_t stac_set_site_pos(stac_model *m, const float *offsets, void *stream);
int32_t stac_get_site_pos(const stac_model *m, float *offsets_out, void *stream);

/* utils.kinematics on N poses (stac_mjx/utils.py:49-60 -> mjx smooth.kinematics).
 * qpos[N,nq] is read; outputs may be NULL: qpos_norm_out[N,nq] (quaternions normalised, as MJX
 * writes back), xpos[N,nbody,3], xquat[N,nbody,4], site_xpos[N,K,3]. */
int32_t stac_fk(const stac_model *m, const float *qpos, int32_t N, float *qpos_norm_out, float *xpos,
                float *xquat, float *site_xpos, void *stream);

/* Batched StacCore.q_opt (stac_mjx/stac_core.py:193-235): N independent solves with the same masks.
 *   kp[N,3K], q0[N,nq]; qs_to_opt[nq] and kps_to_opt[3K] are HOST uint8 masks.
 *   lb[nq], ub[nq]: HOST float box of THIS call, as q_opt takes it per call (hyperparams_proj, stac_core.py:83);
 *   both NULL = the bounds given at stac_model_create.
 *   params_out[N,nq]  = res.params (not blended with q0 -- the caller applies make_qs)
 *   state_out[N,4]    = {error, stepsize, t, loss(params)}   (res.state)
 *   counters_out[N,4] = {iter_num, ls_evals, grad_evals, 1}  (may be NULL) */
int32_t stac_q_solve(const stac_model *m, const stac_q_params *p, const float *kp, const float *q0,
                     const uint8_t *qs_to_opt, const uint8_t *kps_to_opt, const float *lb, const float *ub,
                     int32_t N, float *params_out, float *state_out, uint32_t *counters_out, void *stream);

/* The q_phase of C clips of F frames each, one warm-started chain per clip: per clip
 * [root_optimization on frame 0 (compute_stac.py:17-104) if do_root_opt] then pose_optimization
 * (compute_stac.py:170-278: per frame one full-body solve + P part solves, each followed by
 * replace_qs).  This is what Stac.ik_only vmaps over clips (stac.py:405-440) and what
 * Stac.fit_offsets runs on its single chain (stac.py:298-311, C = 1, q_init = carried qpos).
 *   kp[C,F,3K]; q_init[C,nq] or NULL (-> qpos0, like mjx.make_data)
 *   part_masks: HOST uint8 [P,nq]; trunk_kps: HOST uint8 [K] (used only when do_root_opt)
 *   qpos_out[C,F,nq], err_out[C,F] (PG residual of the frame's LAST solve, compute_stac.py:252),
 *   counters_out[C,F,4] = {sum iter, sum ls_evals, sum grad_evals, n_solves} (may be NULL),
 *   q_carry_out[C,nq] final qpos of every chain (may be NULL),
 *   xpos_out[C,F,nbody,3], xquat_out[C,F,nbody,4], markers_out[C,F,K,3] (each may be NULL). */
int32_t stac_q_phase(const stac_model *m, const stac_q_params *p, const float *kp,
                     const float *q_init, const uint8_t *part_masks, const uint8_t *trunk_kps,
                     int32_t C, int32_t F, int32_t P, int32_t root_kp_idx, int32_t root_dims,
                     int32_t do_root_opt, float *qpos_out, float *err_out, uint32_t *counters_out,
                     float *q_carry_out, float *xpos_out, float *xquat_out, float *markers_out,
                     void *stream);

/* Cross-frame sums of the offset phase (_m_opt, stac_mjx/stac_core.py:148-160) over T frames:
 * partial[3K+2] = { s[K,3] = sum_t R^T (y - p),  z2 = sum |y - p|^2,  T }.
 * With several GPUs each rank calls this on its shard and the host all-reduces `partial`
 * (one RCCL all-reduce of 3K+2 floats) before stac_m_phase_finish.
 * workspace: device scratch of at least stac_m_phase_workspace_floats(m, T) floats. */
int64_t stac_m_phase_workspace_floats(const stac_model *m, int32_t T);
int32_t stac_m_phase_partial(const stac_model *m, const float *kp, const float *q, int32_t T,
                             float *workspace, float *partial, void *stream);
/* Closed form (stac_core.py:162-170): offsets_out[K,3], err_out[1].  All device pointers. */
int32_t stac_m_phase_finish(const stac_model *m, const float *partial, const float *initial_offsets,
                            const float *is_regularized, float reg_coef, float *offsets_out,
                            float *err_out, void *stream);

/* ---- Rendering (DESIGN.md "Rendering"): a ray caster over primitive and mesh geoms, keypoints and markers. --------
 * Static primitives (P: the visible model geoms, then the visible model sites) are posed by their body's xpos / xquat;
 * per frame there are also K keypoint spheres, K marker spheres and, with show_error, K keypoint-to-marker capsules.
 * Primitive ids: static 0..P-1, keypoint k -> P+k, marker k -> P+K+k, segment k -> P+2K+k.  P + 3K must not exceed
 * STAC_RENDER_MAX_PRIMS (STAC_ERR_CAPACITY otherwise). */
#define STAC_RENDER_MAX_PRIMS 512
#define STAC_RENDER_LAYERS 8 /* transparent hits composited per pixel (the nearest ones) */
enum { STAC_RENDER_TRANSPARENT = 1, STAC_RENDER_CHECKER = 2, STAC_RENDER_TEXUNIFORM = 4 };

/* HOST pointers, copied at stac_render_scene_create.  prim_type uses mjtGeom values: 0 plane, 2 sphere, 3 capsule,
 * 4 ellipsoid, 5 cylinder, 6 box, and 7 mesh (only through stac_render_scene_create_with_meshes; prim_size of a mesh
 * primitive is ignored). */
typedef struct stac_render_tables {
    int32_t nprim;               /* P */
    const int32_t *prim_type;    /* [P] */
    const int32_t *prim_body;    /* [P] body id (< nbody of the model) */
    const int32_t *prim_flags;   /* [P] STAC_RENDER_* bits */
    const float *prim_size;      /* [P,3] MuJoCo geom size */
    const float *prim_pos;       /* [P,3] in the body frame */
    const float *prim_quat;      /* [P,4] in the body frame, w,x,y,z */
    const float *prim_rgba;      /* [P,4] colour (rgb1 of a checker plane) */
    const float *prim_rgb2;      /* [P,3] second checker colour */
    const float *prim_texrepeat; /* [P,2] checker repeat */
    int32_t nkp;                 /* K: keypoints, markers and segments per frame */
    const float *kp_rgba;        /* [K,4] */
    float marker_rgba[4], segment_rgba[4];
    float marker_radius, segment_radius;
    int32_t nlight;
    const float *light_dir;      /* [nlight,3] world direction the light shines along (unit) */
    const float *light_diffuse;  /* [nlight,3] */
    float head_ambient[3], head_diffuse[3]; /* headlight (zero when it is off) */
    float alpha;                 /* opacity of STAC_RENDER_TRANSPARENT primitives */
    float background[3];
} stac_render_tables;

typedef struct stac_render_scene stac_render_scene; /* opaque */

/* Uploads the tables to the model's device.  Returns NULL on failure (see stac_last_error / stac_last_error_code). */
stac_render_scene *stac_render_scene_create(const stac_model *m, const stac_render_tables *t);
void stac_render_scene_destroy(stac_render_scene *s);

/* Triangle meshes.  A mesh instance (a primitive of type 7) is ONE primitive against STAC_RENDER_MAX_PRIMS, whatever its
 * triangle count; several primitives may share a mesh.  A mesh is two-sided and flat shaded: the hit of a ray is the
 * triangle with the smallest t > 0, ties to the lower triangle index (its position in tri_vertex), whatever the
 * hierarchy; zero-area triangles are never hit.  The triangle index travels in 20 bits of the pixel's 64-bit hit key,
 * next to the 10 bits of the primitive id, hence the limit per mesh: */
#define STAC_RENDER_MAX_MESH_TRIS 1048576
/* HOST pointers, copied to device global memory at stac_render_scene_create_with_meshes.  Mesh k owns the nodes
 * node_offset[k] .. node_offset[k+1]-1 and the triangles tri_offset[k] .. tri_offset[k+1]-1; node indices and triangle
 * indices inside a mesh are relative to those.  Nodes are in depth-first order, node 0 is the root.  The walk starts
 * at node 0; at node n: box missed -> n = skip; inner node (count 0) -> n = n + 1; leaf -> test the triangles
 * first .. first+count-1, then n = skip; it stops when n reaches the mesh's node count.  So every skip must lie in
 * n+1 .. node count (the walk only moves forward, it needs no stack), a leaf's skip is n + 1, and a leaf's range must
 * lie inside the mesh's triangles; STAC_ERR_INVALID otherwise.  Boxes must contain the triangles below them; the kernel
 * pads them per ray against float32 rounding.  Vertices are in the geom frame (prim_pos / prim_quat). */
typedef struct stac_render_meshes {
    int32_t nmesh;
    const int32_t *node_offset; /* [nmesh+1], node_offset[0] = 0, every mesh has at least one node */
    const int32_t *tri_offset;  /* [nmesh+1], tri_offset[0] = 0; at most STAC_RENDER_MAX_MESH_TRIS per mesh (STAC_ERR_CAPACITY) */
    const float *node_box;      /* [NN,6] lo[3], hi[3] */
    const int32_t *node_link;   /* [NN,3] skip, first, count */
    const float *tri_vertex;    /* [NT,3,3] */
    const int32_t *prim_mesh;   /* [P] mesh of a type-7 primitive (0 .. nmesh-1); ignored for the other types */
} stac_render_meshes;

/* stac_render_scene_create with meshes (meshes == NULL: exactly stac_render_scene_create, which refuses type 7).
 * A scene without a type-7 primitive renders with the mesh-free kernel, bit for bit and at its speed. */
stac_render_scene *stac_render_scene_create_with_meshes(const stac_model *m, const stac_render_tables *t,
                                                        const stac_render_meshes *meshes);

/* Renders N frames of width x height pixels, row 0 at the top.
 *   xpos[N,nbody,3], xquat[N,nbody,4]: body poses (stac_fk); kp[N,K,3] and markers[N,K,3] may be NULL (not drawn);
 *   show_error != 0 draws the segments (needs both).  cam[N,12] = {position[3], R[3,3] row-major whose columns are
 *   the camera's x, y, z axes in world}: the camera looks along -z with y up; tan_half_fovy = tan(fovy / 2), vertical.
 *   Outputs (each may be NULL): rgb_out[N,H,W,3] uint8, seg_out[N,H,W] int32 (id of the nearest opaque hit or -1),
 *   depth_out[N,H,W] float (distance along the ray to that hit, +inf for none). */
int32_t stac_render(const stac_render_scene *s, int32_t N, const float *xpos, const float *xquat, const float *kp,
                    const float *markers, int32_t show_error, const float *cam, float tan_half_fovy, int32_t width,
                    int32_t height, uint8_t *rgb_out, int32_t *seg_out, float *depth_out, void *stream);

/* ---- JPEG encoding of frames on the device (no stac_model needed; the current device is used) ----------------------
 * Baseline sequential JPEG exactly as libjpeg writes it with its default tables: 8 bit, YCbCr 4:2:0, one interleaved
 * scan, Annex K Huffman tables, IJG quality scaling, integer colour conversion and "slow integer" DCT, a restart marker
 * every restart_mcus MCUs (16 x 16 pixels).  The bytes equal what libjpeg produces for the same pixels, quality and
 * restart interval.  width, height: 1 .. 65535; quality: 1 .. 100. */

/* HOST.  Writes SOI .. SOS (everything in front of the entropy-coded data) to buf and returns its length (at most 640);
 * restart_mcus 0 .. 65535, 0 = no DRI segment.  buf == NULL: only the length.  Negative on error. */
int64_t stac_jpeg_header(int32_t width, int32_t height, int32_t quality, int32_t restart_mcus, uint8_t *buf, int64_t capacity);

/* Bytes of device workspace that stac_jpeg_encode needs for N frames (restart_mcus 1 .. 65535).  Negative on error. */
int64_t stac_jpeg_workspace_bytes(int64_t N, int32_t width, int32_t height, int32_t restart_mcus);

/* Encodes rgb[N,H,W,3] (device, uint8, any byte alignment) into N complete files (SOI .. EOI) written back to back into
 * out (device); frame f occupies out[frame_offset[f] .. frame_offset[f+1]).  frame_offset (device, [N+1]) always holds
 * the true sizes.  Nothing is written at or beyond out + out_capacity: when frame_offset[N] > out_capacity the output
 * is truncated there and the call is to be repeated with a larger buffer.  workspace: device, 8-byte aligned, at least
 * stac_jpeg_workspace_bytes(...) bytes, its contents do not matter; it may be reused once the call has finished on
 * `stream`.  restart_mcus: 1 .. 65535.  N == 0: nothing is done. */
int32_t stac_jpeg_encode(int64_t N, int32_t width, int32_t height, int32_t quality, int32_t restart_mcus, const uint8_t *rgb,
                         uint8_t *out, int64_t out_capacity, int64_t *frame_offset, void *workspace, int64_t workspace_bytes,
                         void *stream);

/* ---- Post-processing of a continuous run on the device (no stac_model needed; the current device is used) ----------
 * DESIGN.md "Post-processing on the GPU".  Row-major float32 arrays; D = the flattened trailing size of a frame. */

/* HOST.  Rows of the stitched array of C clip windows of F + overlap frames: R = F + overlap + max(C-2, 0) * F +
 * max(F - overlap, 0) (0 for C == 0); that is C * F when C >= 2 and F >= overlap.  Negative (STAC_ERR_INVALID) for C < 0,
 * F < 1 or overlap outside 1..32. */
int64_t stac_post_stitch_rows(int64_t C, int32_t F, int32_t overlap);

/* utils.handle_edge_effects on one array (stac_mjx/utils.py:393-461): src[C, F+overlap, D] -> dst[dst_rows, D], where
 * dst_rows must equal stac_post_stitch_rows(C, F, overlap).  Rows: clip 0 whole; clips 1..C-2 from frame `overlap` on;
 * clip C-1 frames overlap..F-1 (for C == 1 that is clip 0 again, as the reference slices).  A row from (c, t) with t >= F
 * and c < C-1 is (float)((1 - m[t-F]) * (double)src[c,t] + m[t-F] * (double)src[c+1,t-F]), every other row a copy; all
 * reads are of unfaded values.  mask_host: HOST double[overlap], the fade weights (copied during the call).  src and dst
 * must not overlap.  C == 0: nothing is done. */
int32_t stac_post_stitch(const float *src, int64_t C, int32_t F, int32_t overlap, int32_t D, const double *mask_host,
                         float *dst, int64_t dst_rows, void *stream);

/* utils.compute_velocity_from_kinematics on every clip of F frames (stac_mjx/utils.py:302-347, called per clip by
 * main.py:118-133): qpos[N, nq] with N % F == 0 -> qvel[N, nq - (freejoint ? 1 : 0)].  The last frame of a clip differences
 * against itself.  Free joint (nq >= 7): columns 0..2 translation, 3..5 the root gyro from the normalised quaternion
 * difference (float32 product and norm, axis-angle in double), 6.. joints clipped to +-max_qvel; without one every
 * column is a clipped difference.  dt and max_qvel are rounded to float32 as numpy does.  N == 0: nothing is done. */
int32_t stac_post_qvel(const float *qpos, int64_t N, int32_t nq, int32_t F, double dt, int32_t freejoint, double max_qvel,
                       float *qvel, void *stream);

/* Smoothing fitted poses along time (DESIGN.md "Smoothing fitted poses").  The reference has no counterpart: users of a
 * fitted trajectory low-pass qpos by hand in front of utils.compute_velocity_from_kinematics (stac_mjx/utils.py:302-347),
 * whose forward difference divides the frame-to-frame jitter of independent per-frame fits by dt.
 *
 * qpos[N, nq] -> out[N, nq], N whole clips of clip_len >= W = 2 * half_window + 1 rows; every element of out written once.
 * taps: HOST float[W * W], row p = the weights of an output at window position p (read before the call returns).  Frame t
 * of a clip uses the window that starts at s = clamp(t - half_window, 0, clip_len - W) of that clip and row p = t - s;
 * nothing is read from another clip.  quat_cols: HOST int32[n_quat], the first columns of the quaternion blocks (w, x, y,
 * z; columns 3 of a free joint, the four of a ball joint), read before the call returns; every other column is a scalar.
 * Scalar column: acc = taps[p][0] * x[s], then acc = acc + taps[p][j] * x[s + j] for j = 1 .. W-1, in float32 with one
 * rounding per operation, then clamped to [lb, ub] of the column with comparisons that keep a NaN (lb, ub: device
 * float[nq], both or neither; NULL = no clamp).  Quaternion block, c = the block of frame t itself: per j, y = x[s + j],
 * d = ((c0*y0 + c1*y1) + c2*y2) + c3*y3, sg = d < 0 ? -1 : +1, and per component acc_k (+)= taps[p][j] * (sg * y_k) in the
 * order of a scalar column; n = sqrt(((a0*a0 + a1*a1) + a2*a2) + a3*a3); the output is acc_k / n where n > 0, else the
 * bits of c; no clamp.  The output lies in the hemisphere of the frame's own quaternion.
 * half_window in 1 .. 16; n_quat in 0 .. 64 (kSmoothMaxQuat; the free joint's one block is all the models of
 * tests/golden/ have), blocks inside the row and disjoint; rows of nq floats must leave room for one window in 64 KiB of
 * LDS (nq <= 437 at half_window 16, <= 3 275 at 1); arrays 4-byte aligned; out must overlap none of qpos, lb, ub -- in
 * place is not possible (all of it STAC_ERR_INVALID, before anything is launched or written).  N == 0: nothing is done.
 * A stream-ordered allocation of W * W floats, one or two launches that fill it and one kernel on `stream`; no
 * synchronisation, no workgroup waits for another. */
int32_t stac_post_smooth(const float *qpos, int64_t N, int32_t nq, int32_t clip_len, int32_t half_window, const float *taps,
                         const int32_t *quat_cols, int32_t n_quat, const float *lb, const float *ub, float *out, void *stream);

/* Resampling fitted poses to another frame rate (stac.resample). */

/* HOST.  Output rows of one clip of clip_len input rows resampled up by `up` and down by `down`:
 * ((clip_len - 1) * up) / down + 1 -- output m sits at input position m * down / up and none lies beyond the last sample.
 * Negative (STAC_ERR_INVALID) for clip_len < 1 (or beyond 2^56), up outside 1 .. 32 or down outside 1 .. 64. */
int64_t stac_post_resample_rows(int64_t clip_len, int32_t up, int32_t down);

/* Resamples x [n_rows][n_cols], whole clips of clip_len rows, along time by up / down with a polyphase filter
 * (csrc/stac_resample.hpp states the rule) into out [out_rows][n_cols], out_rows =
 * (n_rows / clip_len) * stac_post_resample_rows(clip_len, up, down): the outputs of a clip follow those of the clip before.
 * Output m of a clip, at n = (m * down) / up and phase r = (m * down) % up, is the sum over j = 0 .. W - 1 of
 * taps_dev[r][j] * (input row n + j - H + 1 of the clip, the index clamped to 0 .. clip_len - 1), H = half / up + 1, W = 2 H,
 * in float32, one rounding per operation in the order of j.  No window reaches into another clip.
 * taps_dev [up][W], DEVICE memory (post.resample_taps makes it; `half` is the filter's half-length lobes * max(up, down)).
 * quat_cols [n_quat], HOST memory: the first columns of the quaternion blocks of a row (n_quat <= 64, blocks inside the row and
 * disjoint); the rows of a block's window are brought into the hemisphere of the block in input row n (a zero or NaN dot product
 * counts as +), weighted, summed and divided by the float32 norm, and where the norm is not > 0 the output is that block.
 * lb, ub [n_cols], both or neither (NULL): every other column is clamped to them with comparisons, so a NaN passes; a zero tap
 * is multiplied like any other, so a NaN in a window reaches the output.
 * W <= 256.  x, taps_dev, lb, ub, out 4-byte aligned; no two buffers may overlap -- in place is not possible.  A bad size or
 * ratio, W > 256, rows that are not whole clips, out_rows different from the rule's value, overlapping or misplaced quaternion
 * blocks, lb without ub, a bad pointer, alignment or overlap is STAC_ERR_INVALID before anything is launched.
 * One launch on `stream`; no copy from or to the host, no synchronisation, no workgroup waits for another, no atomics:
 * a second call gives the same bits, and the call can be captured. */
int32_t stac_post_resample(const float *x, int64_t n_rows, int32_t n_cols, int64_t clip_len, int32_t up, int32_t down, int32_t half,
                           const float *taps_dev, const int32_t *quat_cols, int32_t n_quat, const float *lb, const float *ub, float *out,
                           int64_t out_rows, void *stream);

/* ---- Filling missing keypoints before the fit (no stac_model needed; the current device is used) --------------------
 * DESIGN.md "Filling missing keypoints".  Replaces the gap filling that every user of the reference writes by hand in
 * front of stac_mjx.main.run_stac (stac_mjx/main.py:33-139 takes kp_data as it comes and has no answer to a NaN: the
 * residual of q_loss, stac_mjx/stac_core.py:27-62, times a zero weight stays NaN). */
enum { STAC_PREP_LINEAR = 0, STAC_PREP_HOLD = 1 };

/* HOST.  Bytes of device workspace that stac_prep_fill needs for a series of n_frames x n_kp keypoints; it grows with
 * both.  Negative (STAC_ERR_INVALID) for n_frames < 1 or n_kp < 1.  Replaces nothing in the reference: the workspace
 * belongs to the caller like every buffer of this ABI. */
int64_t stac_prep_fill_workspace(int64_t n_frames, int32_t n_kp);

/* kp[n_frames, 3 * n_kp] -> out[n_frames, 3 * n_kp], gap[n_frames, n_kp] (int32), every element of both written once.
 * Keypoint k is missing in frame t iff one of its three coordinates is NaN or +-inf.  Every track k on its own, with p
 * the last valid frame before t and n the first valid frame after it: a valid keypoint is copied bit for bit, gap 0;
 * a missing one becomes, per coordinate, (float)((double)a + ((double)b - (double)a) * ((double)(t-p) / (double)(n-p)))
 * of the values a at p and b at n (STAC_PREP_LINEAR) or the value at the nearer of p and n, a tie to p (STAC_PREP_HOLD);
 * with only one of p, n the value there; a track with no valid frame stays as it is.  gap = the length of the missing
 * run the frame belongs to (n - p - 1; n for a leading run; n_frames - 1 - p for a trailing one; n_frames for an empty
 * track; saturated to INT32_MAX).  workspace: device, 8-byte aligned, at least stac_prep_fill_workspace bytes, its
 * contents do not matter; it may be reused once the call has finished on `stream`.  kp, out, gap and workspace must
 * not overlap (STAC_ERR_INVALID).  Three launches on `stream`; no workgroup waits for another. */
int32_t stac_prep_fill(const float *kp, int64_t n_frames, int32_t n_kp, int32_t mode, float *out, int32_t *gap,
                       void *workspace, int64_t workspace_bytes, void *stream);

/* ---- Rejecting keypoint outliers before the fit (no stac_model needed; the current device is used) -------------------
 * DESIGN.md "Rejecting keypoint outliers".  The reference has no counterpart: stac_mjx.main.run_stac
 * (stac_mjx/main.py:33-139) fits kp_data as it comes, and q_loss (stac_mjx/stac_core.py:27-62) squares the residual of
 * a keypoint that is finite and wrong (an identity swap, a triangulation jump) like any other.
 *
 * kp[n_frames, 3 * n_kp] -> out[n_frames, 3 * n_kp], flag[n_frames, n_kp] (uint8), every element of both written once.
 * The Hampel identifier per track and coordinate.  Keypoint k is missing in frame t iff one of its three coordinates is
 * NaN or +-inf (as in stac_prep_fill).  For a keypoint that is not missing, per coordinate: the window is the frames
 * max(0, t - half_window) .. min(n_frames - 1, t + half_window) in which k is not missing, n their number; n < 3 decides
 * nothing; with s the window values in ascending order, med = 0.5 * ((double)s[(n-1)/2] + (double)s[n/2]),
 * d_j = fabs((double)x_j - med), D the d_j in ascending order, mad = 0.5 * (D[(n-1)/2] + D[n/2]): the coordinate is an
 * outlier iff d_centre > thr * mad and d_centre > min_dev (both strict).  A keypoint with an outlier coordinate is
 * rejected: its three coordinates leave as the quiet NaN 0x7FC00000 and its flag as 1.  Everything else passes bit for
 * bit with flag 0 (missing keypoints included).  Every decision reads kp only.  A run of wrong values longer than
 * half_window frames is its window's majority and is not rejected.
 * half_window in 1 .. 16; thr and min_dev finite and >= 0 (the conventional thr is 3 * 1.4826); kp and out 4-byte
 * aligned; kp, out and flag must not overlap -- in place is not possible (STAC_ERR_INVALID, before any launch).
 * One launch on `stream`, no workspace; no workgroup waits for another. */
int32_t stac_prep_reject(const float *kp, int64_t n_frames, int32_t n_kp, int32_t half_window, double thr, double min_dev,
                         float *out, uint8_t *flag, void *stream);

/* ---- Rejecting keypoints that break pairwise distances (stac.reject_pairwise; no stac_model needed) -----------------
 * DESIGN.md section 14. */

/* HOST.  Bytes of device workspace that stac_prep_pairwise needs for a series of n_frames x n_kp keypoints: 4 bytes per
 * pair of keypoints and frame (rounded up to whole tiles of 64 frames) plus 57 376 bytes per pair; 8 for n_kp == 1.
 * Negative (STAC_ERR_INVALID) for n_frames < 1 or n_kp < 1 or a size beyond int64, STAC_ERR_CAPACITY for n_kp > 64. */
int64_t stac_prep_pairwise_workspace(int64_t n_frames, int32_t n_kp);

/* Rejects the keypoints of kp [n_frames][3 n_kp] that break the distributions of the pairwise distances over the whole
 * series (csrc/stac_pairwise.hpp states the rule).  For the P = n_kp (n_kp - 1) / 2 pairs (a, b),
 * a < b, in lexicographic order: the float32 distance in every frame where both keypoints are present (no coordinate NaN
 * or infinite) and the distance is finite; its exact median and median absolute deviation over those n frames (n < 3: the
 * pair decides nothing); the pair is bad in a frame iff its deviation from the median exceeds both thr * mad and min_dev.
 * Per frame the keypoint in the most bad pairs (ties: the lowest index) is rejected while that count is at least `votes`,
 * and its pairs are removed before the next is looked for.
 * out [n_frames][3 n_kp]: a rejected keypoint is three quiet NaN 0x7FC00000, every other element is kp's bit for bit.
 * flag [n_frames][n_kp]: 1 where rejected.  pair_n [P] (n), pair_med [P], pair_mad [P] (quiet NaN where n < 3): room
 * for at least one element each, also for n_kp == 1.
 * thr and min_dev finite and >= 0 (the host passes thr = nsigma * 1.4826); votes >= 1; n_kp <= 64 (STAC_ERR_CAPACITY
 * above).  workspace: at least stac_prep_pairwise_workspace bytes, its contents do not matter; it may be reused once the
 * call has finished on `stream`.  kp, out 4-byte aligned, pair_n, pair_med, pair_mad, workspace 8-byte aligned; no two
 * buffers may overlap -- in place is not possible (all of it STAC_ERR_INVALID, before anything is launched).
 * Two memsets and 14 launches on `stream` (one launch for n_kp == 1); no copy to the host, no synchronisation, no
 * workgroup waits for another, no floating-point atomics: a second call gives the same bits. */
int32_t stac_prep_pairwise(const float *kp, int64_t n_frames, int32_t n_kp, double thr, double min_dev, int32_t votes,
                           float *out, uint8_t *flag, int64_t *pair_n, double *pair_med, double *pair_mad,
                           void *workspace, int64_t workspace_bytes, void *stream);

/* ---- Repairing left / right keypoint swaps before the fit (stac.repair_swaps; no stac_model needed) -----------------
 * DESIGN.md section 15. */

/* HOST.  Bytes of device workspace that stac_prep_swaps needs for a series of n_frames x n_kp keypoints: those of
 * stac_prep_pairwise_workspace, whatever the candidates.  Negative (STAC_ERR_INVALID) for
 * n_frames < 1 or n_kp < 1 or a size beyond int64, STAC_ERR_CAPACITY for n_kp > 64. */
int64_t stac_prep_swaps_workspace(int64_t n_frames, int32_t n_kp);

/* Exchanges, frame by frame, the two keypoints of a candidate pair of kp [n_frames][3 n_kp] where the pairwise distances
 * say that they carry each other's label (csrc/stac_swap.hpp states the rule).  The statistics are
 * those of stac_prep_pairwise over kp as given: for the P = n_kp (n_kp - 1) / 2 pairs, n, the exact median and the exact
 * median absolute deviation of the float32 distance; a distance d is bad for a pair iff its deviation from that pair's
 * median exceeds both thr * mad and min_dev.  For a candidate (a, b) in a frame, every third keypoint k whose pairs
 * {a, k} and {b, k} both have n >= 3 and are both valid in the frame adds to b0 whether d(a, k) is bad for {a, k} and
 * whether d(b, k) is bad for {b, k} (the frame as labelled), and to b1 whether d(b, k) is bad for {a, k} and whether
 * d(a, k) is bad for {b, k} (the labels exchanged).  The candidate swaps in the frame iff b0 >= min_bad and
 * 2 b1 <= b0.  Every decision is taken from the input frame alone.
 * cand: HOST memory, [n_cand][2] keypoint indices (a, b) in either order, a != b, both in 0 .. n_kp - 1, every keypoint
 * in at most one candidate (so n_cand <= n_kp / 2 <= 32); it is read before the call returns and may be NULL for
 * n_cand == 0.
 * out [n_frames][3 n_kp]: where a candidate swaps, the three words of a and of b exchanged bit for bit; every other
 * element is kp's bit for bit.  flag [n_frames][n_cand]: 1 where the candidate swaps (room for n_frames bytes also for
 * n_cand == 0, where nothing is written to it).  pair_n [P], pair_med [P], pair_mad [P]: as stac_prep_pairwise writes
 * them for the same kp, bit for bit (room for at least one element each).
 * thr and min_dev finite and >= 0 (the host passes thr = nsigma * 1.4826); min_bad >= 1; n_kp <= 64 (STAC_ERR_CAPACITY
 * above).  workspace: at least stac_prep_swaps_workspace bytes, its contents do not matter; it may be reused once the
 * call has finished on `stream`.  kp, out 4-byte aligned, pair_n, pair_med, pair_mad, workspace 8-byte aligned; no two
 * device buffers may overlap -- in place is not possible.  A bad candidate table, size, parameter, pointer, alignment
 * or overlap is STAC_ERR_INVALID before anything is launched.
 * Two memsets and 14 launches on `stream` (one launch for n_kp == 1): the statistics part of stac_prep_pairwise and one
 * decision launch that takes the candidate table by value.  No copy from or to the host, no synchronisation, no workgroup
 * waits for another, no floating-point atomics: a second call gives the same bits, and the call can be captured. */
int32_t stac_prep_swaps(const float *kp, int64_t n_frames, int32_t n_kp, const int32_t *cand /* HOST [n_cand][2] */,
                        int32_t n_cand, double thr, double min_dev, int32_t min_bad, float *out,
                        uint8_t *flag /* [n_frames][max(n_cand,1)] */, int64_t *pair_n, double *pair_med,
                        double *pair_mad, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- Filling long keypoint gaps from rigid neighbours (stac.fill_donors; no stac_model needed) ----------------------
 * DESIGN.md section 17. */

/* HOST.  Bytes of device workspace that stac_prep_donor needs for a series of n_frames x n_kp keypoints: those of
 * stac_prep_fill_workspace.  Negative (STAC_ERR_INVALID) for n_frames < 1 or n_kp < 1 or a size beyond int64,
 * STAC_ERR_CAPACITY for n_kp > 64. */
int64_t stac_prep_donor_workspace(int64_t n_frames, int32_t n_kp);

/* Fills the missing keypoints of kp [n_frames][3 n_kp] from the local frame of three other keypoints that are still
 * tracked (csrc/stac_donor.hpp states the rule).  Missing, and the frames p (the last valid one
 * before) and n (the first valid one after) of a missing keypoint k in frame t, are those of stac_prep_fill.
 * don [n_kp][n_triples][3], DEVICE memory: row d of keypoint k is a donor triple (a, b, c); the list of k ends at the
 * first row that is not three different indices in 0 .. n_kp - 1, all different from k (such a row is never used as an
 * address).  The first usable triple of the list fills: the coordinates of k in the frame of (a, b, c) -- origin a, axes
 * u = b - a, w = (c - a) less its part along u, m = u x w, not normalised -- are taken at p and at n, interpolated
 * linearly in time (one neighbour only: held), and carried back by the frame of (a, b, c) at t, all in double with one
 * rounding to float32.  A triple is usable iff a, b, c are not missing at t or at those of p, n that exist, the squared
 * lengths of u, w, m are > 0 at each of them, and the three rounded values are finite.  Every test reads kp only.
 * out [n_frames][3 n_kp]: the filled values; every other element is kp's bit for bit (what stays missing included).
 * gap [n_frames][n_kp]: as stac_prep_fill writes it for the same kp.  src [n_frames][n_kp]: 0 observed, d + 1 filled by
 * row d, 255 missing and left so (no usable triple, or a track without a valid frame).
 * n_triples in 1 .. 8; n_kp <= 64 (STAC_ERR_CAPACITY above).  workspace: at least stac_prep_donor_workspace bytes, its
 * contents do not matter; it may be reused once the call has finished on `stream`.  kp, don, out, gap 4-byte aligned,
 * workspace 8-byte aligned; no two buffers may overlap -- in place is not possible.  A bad size, n_triples, pointer,
 * workspace size, alignment or overlap is STAC_ERR_INVALID before anything is launched.
 * Three launches on `stream`; no copy from or to the host, no synchronisation, no workgroup waits for another, no atomics:
 * a second call gives the same bits, and the call can be captured. */
int32_t stac_prep_donor(const float *kp, int64_t n_frames, int32_t n_kp, const int32_t *don, int32_t n_triples, float *out,
                        int32_t *gap, uint8_t *src, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- Fit report: per-keypoint marker errors and exact quantiles (no stac_model needed; the current device is used) ----
 * DESIGN.md "Fit report".  The device counterpart of the reference's notebook graph_error.ipynb (per-frame summed squared
 * marker error, its mean / std and histogram), extended by per-keypoint statistics that count observed keypoints only.
 *
 * markers[n_frames, n_kp, 3] and kp[n_frames, 3 * n_kp] (float32; marker_sites and kp_data of a result), gap[n_frames, n_kp]
 * (int32, kp_gap; may be NULL = all zero).  Per pair (t, k): e = d0*d0 + d1*d1 + d2*d2 of d_c = (double)m_c - (double)y_c,
 * in double, left to right; sqerr = (float)e, or the quiet NaN 0x7FC00000 when one of the six inputs is not finite.  A
 * pair is COUNTED iff its six inputs are finite and its gap is 0; sqerr is written for every pair, everything below is
 * over counted pairs.  frame_n[t] = counted keypoints, frame_sse[t] = their e summed in ascending k from +0.0.  Per
 * keypoint: count, sum (of e; an order of summation that depends on (n_frames, n_kp) only: two calls give the same bits),
 * max (of sqerr; NaN without a counted frame), argmax (its smallest frame; -1), hist[k, 1024] (counted sqerr by
 * bits >> 21) and quant[k, q] = s[(permille[q] * (count - 1)) / 1000] of the counted sqerr s in ascending order (NaN
 * without a counted frame): exact, by a three-pass radix select over the bit patterns with digits of 11 / 11 / 10 bits.
 * No square root is taken.  Every element of every output is written; the inputs are only read.
 * permille: HOST int32[n_quant], read before the call returns, n_quant in 1 .. 8, each in 0 .. 1000.  Every other
 * pointer is a device pointer.  workspace: 8-byte aligned, at least stac_report_workspace bytes, its contents do not
 * matter; it may be reused once the call has finished on `stream`.  Arrays 4-byte aligned, those of 64-bit elements
 * 8-byte; no two buffers may overlap (STAC_ERR_INVALID, before anything is launched).  Two memsets and seven launches on
 * `stream`; no copy to the host, no synchronisation, no workgroup waits for another, no floating-point atomics. */
typedef struct stac_report_params {
    const float *markers;
    const float *kp;
    const int32_t *gap;      /* may be NULL */
    int64_t n_frames;
    int32_t n_kp;
    int32_t n_quant;
    const int32_t *permille; /* HOST */
    float *sqerr;            /* [n_frames, n_kp] */
    double *frame_sse;       /* [n_frames] */
    int32_t *frame_n;        /* [n_frames] */
    int64_t *count;          /* [n_kp] */
    double *sum;             /* [n_kp] */
    float *max;              /* [n_kp] */
    int64_t *argmax;         /* [n_kp] */
    int64_t *hist;           /* [n_kp, 1024] */
    float *quant;            /* [n_kp, n_quant] */
    void *workspace;
    int64_t workspace_bytes;
    void *stream;
} stac_report_params;

/* HOST.  Bytes of device workspace of stac_report_errors; grows with each of the three.  Negative (STAC_ERR_INVALID) for
 * n_frames < 1, n_kp < 1 or n_quant outside 1 .. 8. */
int64_t stac_report_workspace(int64_t n_frames, int32_t n_kp, int32_t n_quant);

int32_t stac_report_errors(const stac_report_params *p);

#ifdef __cplusplus
}
#endif
#endif /* STAC_HIP_H */
