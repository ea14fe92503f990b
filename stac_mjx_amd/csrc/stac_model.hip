// stac_model.hip -- the model object of libstac_hip.so: the error state, stac_model_create / destroy (the plan of stac_planner.hip
// and the flat tables in device memory), the marker offsets, the stand-alone kinematics and the m-phase entry points.
#include "stac_host.hpp"
#include "stac_launch.hpp"

static thread_local std::string g_err;
static thread_local int32_t g_err_code = 0;
int fail(int code, const std::string &msg) {
    g_err = msg;
    g_err_code = code;
    return code;
}
void clear_error() { fail(STAC_OK, ""); }
int launch_result(const char *who, hipError_t e) {
    return e == hipSuccess ? STAC_OK : fail(STAC_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

bool find_overlap(const HostBuf *buf, int n, const HostBuf **a, const HostBuf **b) {
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (buf[i].bytes && buf[j].bytes && buf[i].lo < buf[j].lo + (uintptr_t)buf[j].bytes && buf[j].lo < buf[i].lo + (uintptr_t)buf[i].bytes) {
                *a = &buf[i]; *b = &buf[j];
                return true;
            }
    return false;
}

int check_buffers(const char *who, const HostBuf *buf, int n, const char *tail) {
    for (int i = 0; i < n; ++i)
        if (buf[i].lo % buf[i].align != 0)
            return fail(STAC_ERR_INVALID, std::string(who) + ": " + buf[i].name + " must be " + std::to_string(buf[i].align) + "-byte aligned");
    const HostBuf *a, *b;
    if (find_overlap(buf, n, &a, &b))
        return fail(STAC_ERR_INVALID, std::string(who) + ": " + a->name + " and " + b->name +
                                          " overlap: inputs, outputs and workspace are distinct buffers" + tail);
    return STAC_OK;
}

extern "C" const char *stac_last_error(void) { return g_err.c_str(); }
extern "C" int32_t stac_last_error_code(void) { return g_err_code; }
extern "C" int32_t stac_abi_version(void) { return STAC_HIP_ABI_VERSION; }
extern "C" int32_t stac_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" stac_model *stac_model_create(const stac_model_tables *t) {
    if (!t) { fail(STAC_ERR_INVALID, "null tables"); return nullptr; }
    if (stac_device_count() <= 0) {
        fail(STAC_ERR_NO_DEVICE, "no HIP device visible: the STAC engine has no CPU fallback");
        return nullptr;
    }
    stac_model *m = new stac_model();
    (void)hipGetDevice(&m->device);
    {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, m->device) == hipSuccess && n > 0) m->cus = n;
    }
    m->dbg.read_env();
    if (build_plan(m, t) != STAC_OK) { delete m; return nullptr; }
    if (m->dbg.flags >= 0 && (m->dbg.flags & 4)) m->h.fk_uniform = 0;  // A/B switch: run the program step by step through its flags and forms
    const int nb = t->nbody, nj = t->njnt, nq = t->nq, K = t->nsite;
    hipError_t e = hipSuccess;
    auto chk = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    chk(upload(&m->d_blob, m->blob_host.data(), m->blob_host.size()));
    chk(upload(&m->d_body_parentid, t->body_parentid, (size_t)nb));
    chk(upload(&m->d_body_jntadr, t->body_jntadr, (size_t)nb));
    chk(upload(&m->d_body_jntnum, t->body_jntnum, (size_t)nb));
    chk(upload(&m->d_body_pos, t->body_pos, (size_t)nb * 3));
    chk(upload(&m->d_body_quat, t->body_quat, (size_t)nb * 4));
    chk(upload(&m->d_jnt_type, t->jnt_type, (size_t)nj));
    chk(upload(&m->d_jnt_qposadr, t->jnt_qposadr, (size_t)nj));
    chk(upload(&m->d_jnt_pos, t->jnt_pos, (size_t)nj * 3));
    chk(upload(&m->d_jnt_axis, t->jnt_axis, (size_t)nj * 3));
    chk(upload(&m->d_qpos0, t->qpos0, (size_t)nq));
    chk(upload(&m->d_site_bodyid, t->site_bodyid, (size_t)K));
    chk(upload(&m->d_site_pos, t->site_pos, (size_t)K * 3));
    {
        const FkTables ft = build_fk_tables(t);
        m->fk_nslots = ft.nslots;
        chk(upload(&m->d_fk_brec, ft.brec.data(), ft.brec.size()));
        chk(upload(&m->d_fk_jrec, ft.jrec.data(), ft.jrec.size()));
        chk(upload(&m->d_fk_sites, ft.sites.data(), ft.sites.size()));
    }
    m->masks_bytes = (size_t)kMaxKinds * m->h.nqpad + 4 * (size_t)K + 64;
    chk(hipMalloc(reinterpret_cast<void **>(&m->d_masks), m->masks_bytes));
    chk(hipMalloc(reinterpret_cast<void **>(&m->d_bounds), 2 * (size_t)m->h.nqpad * sizeof(float)));
    chk(hipMalloc(reinterpret_cast<void **>(&m->d_ctl), 8 * sizeof(int32_t)));
    {   // hand-off buffer of the straggler hand-off at its maximum size (one entry per wavefront the latency kernel
        // can hold resident), so that no launch ever reallocates (= waits for the device)
        m->hand_cap = lat_one_wave_ok(m->h) ? (int)pick_spec_shape(m->h, kLatG, 1, m->cus, -1, kLatR).resident : 0;
        if (m->hand_cap > 0)
            chk(hipMalloc(reinterpret_cast<void **>(&m->d_hand), (size_t)m->hand_cap * (3 * (size_t)m->h.nqpad + 12) * sizeof(float)));
    }
    if (e != hipSuccess) {
        fail(STAC_ERR_HIP, std::string("model upload failed: ") + hipGetErrorString(e));
        stac_model_destroy(m);
        return nullptr;
    }
    clear_error();
    return m;
}

extern "C" void stac_model_destroy(stac_model *m) {
    if (!m) return;
    DeviceGuard dg(m->device);
    void *ptrs[] = {m->d_bounds, m->d_blob, m->d_body_parentid, m->d_body_jntadr, m->d_body_jntnum, m->d_body_pos,
                    m->d_body_quat, m->d_jnt_type, m->d_jnt_qposadr, m->d_jnt_pos, m->d_jnt_axis,
                    m->d_qpos0, m->d_site_bodyid, m->d_site_pos, m->d_fk_brec, m->d_fk_jrec, m->d_fk_sites, m->d_masks, m->d_scratch, m->d_lm_tab, m->d_ctl, m->d_hand, m->d_order};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete m;
}

extern "C" int32_t stac_model_info(const stac_model *m, int32_t *info) {
    if (!m || !info) return fail(STAC_ERR_INVALID, "null argument");
    info[0] = m->h.nbody; info[1] = m->h.njnt; info[2] = m->h.nq; info[3] = m->h.K;
    info[4] = m->h.nab; info[5] = m->h.naj; info[6] = m->h.nlev;
    int width = 0;
    const int *lev = reinterpret_cast<const int *>(m->blob_host.data()) + m->h.off_lev_adr;
    for (int l = 0; l < m->h.nlev; ++l) width = std::max(width, lev[l + 1] - lev[l]);
    info[7] = width;
    return STAC_OK;
}

extern "C" int32_t stac_set_site_pos(stac_model *m, const float *offsets, void *stream) {
    if (!m || !offsets) return fail(STAC_ERR_INVALID, "null argument");
    DeviceGuard dg(m->device);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(m->d_site_pos, offsets, sizeof(float) * 3 * m->h.K, hipMemcpyDeviceToDevice, s));
    // scatter into the plan's SiteRec.pos (stride 4 words)
    HIP_TRY(hipMemcpy2DAsync(m->d_blob + m->h.off_site, sizeof(SiteRec), offsets, 3 * sizeof(float), 3 * sizeof(float),
                             m->h.K, hipMemcpyDeviceToDevice, s));
    return STAC_OK;
}

extern "C" int32_t stac_get_site_pos(const stac_model *m, float *out, void *stream) {
    if (!m || !out) return fail(STAC_ERR_INVALID, "null argument");
    DeviceGuard dg(m->device);
    HIP_TRY(hipMemcpyAsync(out, m->d_site_pos, sizeof(float) * 3 * m->h.K, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return STAC_OK;
}

// fk_kernel holds the transforms that wait for a child further down the body list in LDS slots (build_fk_tables): a tree that
// parks more of them at once than a workgroup's LDS holds is refused here, on the host, before anything is launched.
static int fk_capacity(const stac_model *m, const char *who) {
    const int cap = stac::fk_max_slots();
    if (m->fk_nslots > cap)
        return fail(STAC_ERR_CAPACITY, std::string(who) + ": the body tree keeps " + std::to_string(m->fk_nslots) +
                                           " transforms parked at once (bodies with a child that does not follow them directly); "
                                           "the kinematics kernel's LDS holds " + std::to_string(cap));
    return STAC_OK;
}

int fk_impl(const stac_model *mc, const float *qpos, int32_t N, float *qn, float *xpos, float *xquat, float *site_xpos, int normalize, void *stream) {
    stac_model *m = const_cast<stac_model *>(mc);
    if (!m || !qpos || N < 0) return fail(STAC_ERR_INVALID, "stac_fk: bad argument");
    if (N == 0) return STAC_OK;
    if (const int rc = fk_capacity(m, "stac_fk")) return rc;
    DeviceGuard dg(m->device);
    // (outputs the caller does not want are not written: the body transforms live in the kernel's LDS rows)
    HIP_TRY(launch_fk(m->full(), qpos, N, qn, xpos, xquat, site_xpos, normalize, (hipStream_t)stream));
    return STAC_OK;
}

extern "C" int32_t stac_fk(const stac_model *m, const float *qpos, int32_t N, float *qn, float *xpos,
                           float *xquat, float *site_xpos, void *stream) {
    return fk_impl(m, qpos, N, qn, xpos, xquat, site_xpos, 1, stream);
}

extern "C" int64_t stac_m_phase_workspace_floats(const stac_model *m, int32_t T) {
    if (!m || T < 0) return -1;
    return (int64_t)T * ((int64_t)m->h.nbody * 7 + 3 * m->h.K + 1);
}

extern "C" int32_t stac_m_phase_partial(const stac_model *m, const float *kp, const float *q, int32_t T,
                                        float *workspace, float *partial, void *stream) {
    if (!m || !workspace || !partial || T < 0 || (T > 0 && (!kp || !q)))  // T = 0: kp / q may be empty (null) arrays
        return fail(STAC_ERR_INVALID, "stac_m_phase_partial: bad argument");
    DeviceGuard dg(m->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t nb = m->h.nbody;
    float *xpos = workspace, *xquat = workspace + (size_t)T * nb * 3, *contrib = workspace + (size_t)T * nb * 7;
    if (T > 0) {
        if (const int rc = fk_capacity(m, "stac_m_phase_partial")) return rc;
        HIP_TRY(launch_fk(m->full(), q, T, nullptr, xpos, xquat, nullptr, 1, s));
    }
    HIP_TRY(launch_m_partial(m->full(), kp, xpos, xquat, T, contrib, partial, s));
    return STAC_OK;
}

extern "C" int32_t stac_m_phase_finish(const stac_model *m, const float *partial, const float *initial_offsets,
                                       const float *is_regularized, float reg_coef, float *offsets_out,
                                       float *err_out, void *stream) {
    if (!m || !partial || !initial_offsets || !is_regularized || !offsets_out)
        return fail(STAC_ERR_INVALID, "stac_m_phase_finish: bad argument");
    DeviceGuard dg(m->device);
    HIP_TRY(launch_m_finish(m->h.K, partial, initial_offsets, is_regularized, reg_coef, offsets_out, err_out,
                            (hipStream_t)stream));
    return STAC_OK;
}
