/*
 * stac_hip_swaps.h -- the third header of libstac_hip.so's C ABI: repairing left / right keypoint swaps before the fit
 * (stac.repair_swaps).  The conventions are those of stac_hip.h: plain C types, device pointers owned by the caller,
 * `stream` a hipStream_t passed as void* (NULL = the default stream), calls asynchronous on `stream`, return value 0 = OK
 * or a negative STAC_ERR_* status with its text in stac_last_error().  The functions of this header do not count into
 * STAC_HIP_ABI_VERSION.
 */
#ifndef STAC_HIP_SWAPS_H
#define STAC_HIP_SWAPS_H

#include <stdint.h>

#include "stac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HOST.  Bytes of device workspace that stac_prep_swaps needs for a series of n_frames x n_kp keypoints: those of
 * stac_prep_pairwise_workspace (stac_hip_pairwise.h), whatever the candidates.  Negative (STAC_ERR_INVALID) for
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

#ifdef __cplusplus
}
#endif

#endif /* STAC_HIP_SWAPS_H */
