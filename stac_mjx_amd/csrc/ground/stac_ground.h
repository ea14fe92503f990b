/*
 * stac_ground.h -- C ABI of libstac_ground.so, the companion library of libstac_hip.so that measures how far the geoms of fitted
 * poses are from the floor (stac.ground: report | level; Stac.ground_clearance; DESIGN.md "Ground clearance").
 *
 * The conventions are those of include/stac_hip.h: plain C types, DEVICE pointers owned by the caller unless a comment says
 * HOST, asynchronous on `stream` (a hipStream_t passed as void*; NULL = the default stream), 0 = OK and negative = error
 * (the STAC_ERR_* codes of include/stac_hip.h), no global state besides the thread-local error string.  No stac_model is
 * needed; the current device is used.
 */
#ifndef STAC_GROUND_H
#define STAC_GROUND_H

#include <stdint.h>

#include "../../../include/stac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Thread-local description of the last error that an entry point of THIS library returned on this thread ("" if none). */
const char *stac_ground_last_error(void);
/* Its status code (STAC_ERR_*; 0 if none). */
int32_t stac_ground_last_error_code(void);

/* The lowest world z of the geoms of a table in every frame of xpos [n_frames][nbody][3] and xquat [n_frames][nbody][4] (w, x, y, z)
 * (csrc/ground/stac_ground.hpp states the rule and every word below).
 * The table: geom_meta [n_geoms][6] (int32: type, body, include, slot, vert_first, vert_count), geom_data [n_geoms][15] (size[3],
 * pos[3], R[3][3] row-major: the geom's frame in its body's) and verts [n_verts][3], the mesh vertices in their geoms' frames.
 * geom_meta_host: HOST, the same words as geom_meta; it is what is checked, and the kernel passes over a device row that is out of
 * range.  Types: sphere 2, capsule 3, ellipsoid 4, cylinder 5, box 6, mesh 7.
 * Per frame: low_z [n_frames], the smallest z over the geoms with include = 1, and low_geom [n_frames] (int32), the smallest table
 * index that attains it (+inf and -1 without an included geom); track_z [n_frames][n_slots], the smallest z over the geoms of each
 * slot.  Per geom: geom_min [n_geoms], its smallest z over the frames (+inf without a finite one), and geom_below [n_geoms] (int64),
 * the number of frames in which it is below z_ref (strictly).  A z that is not finite makes low_z (with low_geom -1, for an included
 * geom) and the geom's slot of track_z the quiet NaN 0x7FC00000 in its frame and is skipped per geom.
 * 1 <= n_frames <= 2^40; 2 <= nbody <= 4096, 1 <= n_geoms <= 4096, 0 <= n_verts <= 2^20 (STAC_ERR_CAPACITY above); 0 <= n_slots <= 32;
 * every row of geom_meta_host with a known type, a body in 1 .. nbody - 1, include 0 or 1, a slot in -1 .. n_slots - 1 and, for a
 * mesh, a range of at least one vertex inside verts; every buffer non-null (track_z with n_slots > 0, verts with n_verts > 0),
 * 4-byte aligned (xquat 16, geom_below 8), no two overlapping (all of it STAC_ERR_INVALID, before anything is launched).
 * Two memsets and one launch on `stream`; no copy to the host, no synchronisation, no workspace, no workgroup waits for another.
 * The only atomics are integer minima / maxima on the bit patterns of geom_min and integer adds on geom_below: a second call gives
 * the same bits. */
int32_t stac_ground_clearance(const float *xpos, const float *xquat, int64_t n_frames, int32_t nbody, const int32_t *geom_meta_host,
                              const int32_t *geom_meta, const float *geom_data, int32_t n_geoms, const float *verts, int32_t n_verts,
                              int32_t n_slots, float z_ref, float *low_z, int32_t *low_geom, float *track_z, float *geom_min,
                              int64_t *geom_below, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* STAC_GROUND_H */
