/*
 * stac_hip_donor.h -- the fourth header of libstac_hip.so's C ABI: filling long keypoint gaps from rigid neighbours
 * (stac.fill_donors).  The conventions are those of stac_hip.h: plain C types, device pointers owned by the caller,
 * `stream` a hipStream_t passed as void* (NULL = the default stream), calls asynchronous on `stream`, return value 0 = OK
 * or a negative STAC_ERR_* status with its text in stac_last_error().  The functions of this header do not count into
 * STAC_HIP_ABI_VERSION.
 */
#ifndef STAC_HIP_DONOR_H
#define STAC_HIP_DONOR_H

#include <stdint.h>

#include "stac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif

#endif /* STAC_HIP_DONOR_H */
