// stac_launch.hpp -- the launchers of stac_kernels.hip and stac_lm.hip as the host units call them (stac_q.hip, stac_model.hip).
// The defining units include this header too: a signature that drifts is a compile error.
#pragma once
#include <hip/hip_runtime.h>

#include "stac_plan.hpp"
#include "stac_shapes.hpp"

namespace stac {
hipError_t launch_q_phase(const QArgs &a, const QInst &inst, int wpb, size_t lds_bytes, hipStream_t s);
hipError_t launch_q_phase_lm(const QArgs &a, const LmArgs &L, const QInst &inst, int wpb, size_t lds_bytes, hipStream_t s);
hipError_t launch_fk(const FullModel &M, const float *qpos, int N, float *qn, float *xpos, float *xquat, float *site_xpos, int normalize, hipStream_t s);
int fk_max_slots();
hipError_t launch_m_partial(const FullModel &M, const float *kp, const float *xpos, const float *xquat, int T, float *contrib, float *partial, hipStream_t s);
hipError_t launch_m_finish(int K, const float *partial, const float *m0, const float *dreg, float lam, float *out, float *err, hipStream_t s);
hipError_t launch_ctl_init(int32_t *ctl, int v0, int v1, int v2, int v3, int v4, hipStream_t s);
hipError_t launch_chain_order(const float *kp, int C, int F, int K, const float *rest_sites, const uint8_t *kpw, int root_kp_idx, float rx, float ry,
                              float rz, uint32_t *hist, uint32_t *keybits, int32_t *perm, int32_t *place, hipStream_t s);
extern thread_local int g_last_q_shape[4];  // the instantiation of the thread's most recent q_phase launch (stac_debug_last_q_kernel)
}  // namespace stac
