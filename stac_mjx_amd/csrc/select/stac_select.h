/*
 * stac_select.h -- C ABI of libstac_select.so, the companion library of libstac_hip.so that chooses the calibration frames of
 * a recording by pose diversity (stac.fit_frames: diverse; DESIGN.md "Choosing calibration frames").
 *
 * The conventions are those of include/stac_hip.h: plain C types, DEVICE pointers owned by the caller unless a comment says
 * HOST, asynchronous on `stream` (a hipStream_t passed as void*; NULL = the default stream), 0 = OK and negative = error
 * (the STAC_ERR_* codes of include/stac_hip.h), no global state besides the thread-local error string.  No stac_model is
 * needed; the current device is used.
 */
#ifndef STAC_SELECT_H
#define STAC_SELECT_H

#include <stdint.h>

#include "../../../include/stac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Thread-local description of the last error that an entry point of THIS library returned on this thread ("" if none). */
const char *stac_select_last_error(void);
/* Its status code (STAC_ERR_*; 0 if none). */
int32_t stac_select_last_error_code(void);

/* HOST.  Bytes of device workspace that stac_select_diverse needs for a series of n_frames x n_kp keypoints: 4 bytes per
 * pair of keypoints and frame (rounded up to whole tiles of 64 frames), 5 bytes per frame and about 16 KiB.  Negative:
 * STAC_ERR_INVALID for n_frames < 1 or n_kp < 2, STAC_ERR_CAPACITY for n_kp > 64 or n_frames > 2^32 - 1. */
int64_t stac_select_workspace(int64_t n_frames, int32_t n_kp);

/* Chooses up to n_select frames of kp [n_frames][3 n_kp] greedily, each the farthest from all chosen before it
 * (csrc/select/stac_select.hpp states the rule).  The descriptor of a frame is its P = n_kp (n_kp - 1) / 2 float32 keypoint
 * distances, pairs (a, b), a < b, in lexicographic order; a frame is a candidate iff its 3 n_kp coordinates are finite and
 * cand[t] != 0 (cand: uint8 [n_frames], NULL = all ones).  The first pick is the lowest-index candidate with radius2 = +inf;
 * pick i is the candidate whose smallest squared float32 descriptor distance to the earlier picks is largest (ties: the lowest
 * index), and radius2[i] is that distance.  The selection stops before a pick whose distance is 0 and when there is no candidate.
 * sel [n_select] (int64, selection order), radius2 [n_select], n_selected [1] (int64): every element is written; behind
 * n_selected sel is -1 and radius2 the quiet NaN 0x7FC00000.
 * 2 <= n_kp <= 64 and n_frames <= 2^32 - 1 (STAC_ERR_CAPACITY above); 1 <= n_select <= n_frames.  workspace: at least
 * stac_select_workspace bytes, its contents do not matter; it may be reused once the call has finished on `stream`.  kp and
 * radius2 4-byte aligned, sel, n_selected and workspace 8-byte aligned; no two buffers may overlap (all of it
 * STAC_ERR_INVALID, before anything is launched).
 * 1 + 2 n_select launches on `stream`; no copy to the host, no synchronisation, no workgroup waits for another, no
 * floating-point atomics: a second call gives the same bits. */
int32_t stac_select_diverse(const float *kp, int64_t n_frames, int32_t n_kp, const uint8_t *cand, int64_t n_select, int64_t *sel,
                            float *radius2, int64_t *n_selected, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* STAC_SELECT_H */
