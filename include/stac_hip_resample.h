/*
 * stac_hip_resample.h -- the fifth header of libstac_hip.so's C ABI: resampling fitted poses to another frame rate
 * (stac.resample).  The conventions are those of stac_hip.h: plain C types, device pointers owned by the caller,
 * `stream` a hipStream_t passed as void* (NULL = the default stream), calls asynchronous on `stream`, return value 0 = OK
 * or a negative STAC_ERR_* status with its text in stac_last_error().  The functions of this header do not count into
 * STAC_HIP_ABI_VERSION.
 */
#ifndef STAC_HIP_RESAMPLE_H
#define STAC_HIP_RESAMPLE_H

#include <stdint.h>

#include "stac_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif

#endif /* STAC_HIP_RESAMPLE_H */
