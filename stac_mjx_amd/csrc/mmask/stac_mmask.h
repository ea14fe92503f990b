/*
 * stac_mmask.h -- C ABI of libstac_mmask.so, the companion library of libstac_hip.so that runs the offset phase on observed
 * keypoints only (stac.offset_mask: observed; DESIGN.md "Offsets from observed keypoints").
 *
 * The conventions are those of include/stac_hip.h: plain C types, DEVICE pointers owned by the caller unless a comment says
 * HOST, asynchronous on `stream` (a hipStream_t passed as void*; NULL = the default stream), 0 = OK and negative = error
 * (the STAC_ERR_* codes of include/stac_hip.h), no global state besides the thread-local error string.  No stac_model is
 * needed; the current device is used.
 */
#ifndef STAC_MMASK_H
#define STAC_MMASK_H

#include <stdint.h>

#include "../../../include/stac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Thread-local description of the last error that an entry point of THIS library returned on this thread ("" if none). */
const char *stac_mmask_last_error(void);
/* Its status code (STAC_ERR_*; 0 if none). */
int32_t stac_mmask_last_error_code(void);

/* HOST.  Bytes of device workspace that stac_mmask_partial needs for n_frames frames of n_kp keypoints: 4 (3 n_kp + 1) bytes per
 * frame, rounded up to a multiple of 8, and 8 for an empty series.  Negative: STAC_ERR_INVALID for n_frames < 0, n_frames > 2^24
 * or n_kp < 1, STAC_ERR_CAPACITY for n_kp > 4096. */
int64_t stac_mmask_workspace(int64_t n_frames, int32_t n_kp);

/* The sums of the offset phase over the observed keypoints of n_frames frames (csrc/mmask/stac_mmask.hpp states the rule):
 * kp [n_frames][3 n_kp], xpos [n_frames][nbody][3] and xquat [n_frames][nbody][4] as stac_fk / stac_q_phase write them,
 * site_bodyid [n_kp] (int32), valid [n_frames][n_kp] (uint8, non-zero = observed).  (t, k) is observed iff valid[t][k] != 0 and
 * site_bodyid[k] is a body of the model; any other entry adds +0 everywhere and its three floats of kp are never used: a NaN or
 * an infinity there reaches no output.
 * partial [4 n_kp + 2]: s [n_kp][3], the sums of R^T z over the frames in ascending order; n [n_kp], the observed counts as
 * floats; z2, the sum over the frames in ascending order of every frame's subtotal of |z|^2 in keypoint order; n_frames.  Every
 * word is additive across shards of the frames.  With every entry observed s, z2 and n_frames are the bits of
 * stac_m_phase_partial.
 * 0 <= n_frames <= 2^24 (the counts are exact floats), 1 <= n_kp <= 4096 (STAC_ERR_CAPACITY above), 1 <= nbody <= 65536.
 * n_frames == 0 writes zeros and n_frames = 0; kp, xpos, xquat and valid may then be NULL.  workspace: at least
 * stac_mmask_workspace bytes, its contents do not matter; it may be reused once the call has finished on `stream`.  Every
 * float and int32 buffer and the workspace 4-byte aligned; no two buffers may overlap (all of it STAC_ERR_INVALID, before
 * anything is launched).
 * At most two launches on `stream`; no copy to the host, no synchronisation, no atomics: a second call gives the same bits. */
int32_t stac_mmask_partial(const float *kp, const float *xpos, const float *xquat, int32_t nbody, const int32_t *site_bodyid,
                           const uint8_t *valid, int64_t n_frames, int32_t n_kp, void *workspace, int64_t workspace_bytes, float *partial,
                           void *stream);

/* The closed form from the (summed) partial [4 n_kp + 2]: per coordinate i of keypoint k, with m0 [n_kp][3] the offsets to
 * regularise towards, dreg [n_kp][3] the regularisation weights and lam the coefficient: denom = n_k + lam dreg_i,
 * offsets_i = denom == 0 ? m0_i : (s_i + lam dreg_i m0_i) / denom -- a keypoint that was never observed keeps m0 where it is not
 * regularised -- and err = ((z2 - 2 sum v s) + sum n_k v^2) + lam sum (dreg (v - m0))^2.
 * offsets_out [n_kp][3]; err_out [1] and n_out [n_kp] (int32: the observed counts) may be NULL.  With every entry observed the
 * offsets are the bits of stac_m_phase_finish.  1 <= n_kp <= 4096; 4-byte alignment, no overlap (STAC_ERR_INVALID before the
 * launch).  One launch on `stream`. */
int32_t stac_mmask_finish(const float *partial, int32_t n_kp, const float *m0, const float *dreg, float lam, float *offsets_out,
                          float *err_out, int32_t *n_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* STAC_MMASK_H */
