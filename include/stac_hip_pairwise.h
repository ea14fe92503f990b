/*
 * stac_hip_pairwise.h -- the second header of libstac_hip.so's C ABI: rejecting keypoints that break pairwise distances
 * (stac.reject_pairwise).  The conventions are those of stac_hip.h: plain C types, device pointers owned by the caller,
 * `stream` a hipStream_t passed as void* (NULL = the default stream), calls asynchronous on `stream`, return value 0 = OK
 * or a negative STAC_ERR_* status with its text in stac_last_error().  The functions of this header do not count into
 * STAC_HIP_ABI_VERSION.
 */
#ifndef STAC_HIP_PAIRWISE_H
#define STAC_HIP_PAIRWISE_H

#include <stdint.h>

#include "stac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif

#endif /* STAC_HIP_PAIRWISE_H */
