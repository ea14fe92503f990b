/*
 * stac_seam.h -- C ABI of libstac_seam.so, the companion library of libstac_hip.so that measures the pose steps of a fitted series
 * (stac.seam_report: on; Stac.seam_steps; DESIGN.md "Warm-started clips and pose steps").
 *
 * The conventions are those of include/stac_hip.h: plain C types, DEVICE pointers owned by the caller unless a comment says
 * HOST, asynchronous on `stream` (a hipStream_t passed as void*; NULL = the default stream), 0 = OK and negative = error
 * (the STAC_ERR_* codes of include/stac_hip.h), no global state besides the thread-local error string.  No stac_model is
 * needed; the current device is used.
 */
#ifndef STAC_SEAM_H
#define STAC_SEAM_H

#include <stdint.h>

#include "../../../include/stac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Thread-local description of the last error that an entry point of THIS library returned on this thread ("" if none). */
const char *stac_seam_last_error(void);
/* Its status code (STAC_ERR_*; 0 if none). */
int32_t stac_seam_last_error_code(void);

/* The pose steps of qpos [n_rows][nq], n_rows / clip_len clips of clip_len rows (csrc/seam/stac_seam.hpp states the rule).
 * quat_cols: HOST [n_quat], the first columns of the quaternion blocks of a row, in any order; n_lin: 0, or 3 where the first three
 * columns are the free joint's translation.
 * Per row t: step_joint [n_rows], the largest |qpos[t][j] - qpos[t - 1][j]| over the columns that are neither translation nor in a
 * block, and step_col [n_rows] (int32), the smallest such column that attains it (-1 without one); step_rot [n_rows], the largest
 * 1 - |<a, b>| over the blocks; step_lin2 [n_rows], the squared length of the translation's step.  Row 0 is +0 / -1 / +0 / +0.  A
 * row with a value that is not finite has the quiet NaN 0x7FC00000 (and -1) in the outputs that the value enters.
 * Per column: col_max_in [nq], the maximum of the column's measure over the rows with t % clip_len != 0, and col_max_seam [nq], over
 * the rows with t % clip_len == 0, t > 0; +0 where there is no such row, and a measure that is not finite is skipped.
 * 1 <= n_rows <= 2^32, 1 <= nq <= 4096 (STAC_ERR_CAPACITY above), clip_len >= 1 and a divisor of n_rows, 0 <= n_quat <= 64, every
 * block inside n_lin .. nq and no two overlapping, n_lin 0 or 3 and <= nq; every buffer non-null and 4-byte aligned, no two
 * overlapping (all of it STAC_ERR_INVALID, before anything is launched).
 * Two memsets and one launch on `stream`; no copy to the host, no synchronisation, no workspace, no workgroup waits for another.
 * The only atomics are integer maxima on the bit patterns of the non-negative column maxima: a second call gives the same bits. */
int32_t stac_seam_steps(const float *qpos, int64_t n_rows, int32_t nq, int64_t clip_len, const int32_t *quat_cols, int32_t n_quat,
                        int32_t n_lin, float *step_joint, int32_t *step_col, float *step_rot, float *step_lin2, float *col_max_in,
                        float *col_max_seam, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* STAC_SEAM_H */
