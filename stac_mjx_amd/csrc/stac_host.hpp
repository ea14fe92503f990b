// stac_host.hpp -- what the host units of libstac_hip.so share (host only; every unit with C ABI entry points includes it): the
// error state, small HIP helpers, struct stac_model and the host functions that cross units.  The entry points of include/stac_hip.h
// live beside what they drive: stac_model.hip (model, kinematics, m-phase), stac_q.hip (q_phase), stac_planner.hip (plan construction,
// no HIP call) and, for the stateless features, the unit that holds their kernels.
// No CPU fallback exists: every compute entry point needs a GPU and fails loudly without one.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/stac_hip.h"
#include "stac_plan.hpp"
#include "stac_shapes.hpp"

using namespace stac;
#pragma GCC visibility push(hidden)  // what follows crosses units, not the library's boundary (its ABI: include/stac_hip.h)

// ---- error state of the calling thread (defined in stac_model.hip) -----------------------------------------------------------
int fail(int code, const std::string &msg);  // records the error, returns code
void clear_error();
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return fail(STAC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));       \
    } while (0)
// The tail of an entry point that has launched: STAC_OK, or fail() with "<who>: <HIP's message>"
int launch_result(const char *who, hipError_t e);

template <typename T>
hipError_t upload(T **dst, const T *src, size_t n) {
    hipError_t e = hipMalloc(reinterpret_cast<void **>(dst), std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) return e;
    if (n) e = hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

// Makes a device current for the duration of an entry point (a caller may have switched devices since the model or scene was
// created: allocations and launches must still land on its GPU), then restores the caller's.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int device) { if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = hipSetDevice(device) == hipSuccess; }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

// A caller's buffer as the argument checks see it (align: for the checks that report alignment per buffer).  find_overlap visits the
// pairs i < j in order and returns whether two buffers share a byte (*a, *b: the first such pair); a buffer of zero bytes (an optional
// one that was not given) overlaps nothing.
struct HostBuf { const char *name; uintptr_t lo; int64_t bytes; int align; };
bool find_overlap(const HostBuf *buf, int n, const HostBuf **a, const HostBuf **b);
// The check of a whole argument list: STAC_OK, or fail(STAC_ERR_INVALID, ...) for the first buffer whose address is not a multiple of its
// align ("<who>: <name> must be <align>-byte aligned"), else for the first overlapping pair ("<who>: <a> and <b> overlap: inputs, outputs
// and workspace are distinct buffers" + tail)
int check_buffers(const char *who, const HostBuf *buf, int n, const char *tail = "");

// Developer switches: read from the environment ONCE, at stac_model_create, so that a variable
// set later cannot change the launch shape of a model in use.  -1 = not set.
struct DebugSwitches {
    int flags = -1, spec = -1, specg = -1, specr = -1, wpe = -1, wpb = -1, handoff = -1, queue = -1, stride_add = -1, rsplit = -1;
    bool noprune = false, verbose = false, nofast = false, nofree0 = false, noorder = false, nodiet = false, nolean = false, nofk3 = false, nofk3bq = false, nowsum = false;
    static int geti(const char *name) {
        const char *v = getenv(name);
        return v ? atoi(v) : -1;
    }
    void read_env() {
        flags = geti("STAC_HIP_FLAGS"); spec = geti("STAC_HIP_SPEC"); wpe = geti("STAC_HIP_WPE"); wpb = geti("STAC_HIP_WPB");
        handoff = geti("STAC_HIP_HANDOFF"); queue = geti("STAC_HIP_QUEUE"); specg = geti("STAC_HIP_SPECG"); specr = geti("STAC_HIP_SPECR"); stride_add = geti("STAC_HIP_STRIDE_ADD"); rsplit = geti("STAC_HIP_RSPLIT");
        noprune = getenv("STAC_HIP_NOPRUNE") != nullptr; nofast = getenv("STAC_HIP_NOFAST") != nullptr; nofree0 = getenv("STAC_HIP_NOFREE0") != nullptr; noorder = getenv("STAC_HIP_NOORDER") != nullptr; nolean = getenv("STAC_HIP_NOLEAN") != nullptr; nodiet = getenv("STAC_HIP_NODIET") != nullptr; verbose = getenv("STAC_HIP_VERBOSE") != nullptr;
        nofk3 = getenv("STAC_HIP_NOFK3") != nullptr; nofk3bq = getenv("STAC_HIP_NOFK3BQ") != nullptr; nowsum = getenv("STAC_HIP_NOWSUM") != nullptr;
    }
};

// The wrench-sum program of a model (WsumRec, stac_plan.hpp): which of its distinct site ranges come out of row sweeps, which are
// component tasks (with which checkpoint) and which whole ranges.  `ranges` are sorted longest first (build_plan).  parts: bit 0 = plan
// sweeps, bit 1 = plan checkpoints; with neither the program is PlanHeader::rsplit's split (ntask_fixed) in the program's form.
struct WsumProgram {
    int ntask = 0, nwhole = 0, nrows = 0, depth = 0;
    int row_start[3] = {0, 0, 0};  // rows [row_start[i], row_start[i + 1]) of sorted sites
    std::vector<WsumRec> recs;     // the tasks, then the whole ranges
    std::vector<int32_t> rows;     // per (row, lane): {kXf * sorted site (a lane behind the row's end: the row's last), capture bytes:
                                   // byte s = the range whose sum the lane holds after step s, kWsumNone = nobody's}
    double cost = 0.0;
    // the table as the kernel reads it; c_rw: where the range sums stand in a chain's region, dump: six words of it that a full trip
    // neither reads nor keeps -- where a lane stores a sum that is nobody's
    std::vector<int32_t> table(int c_rw, int dump) const {
        std::vector<int32_t> w;
        for (const WsumRec &r : recs) { w.push_back(r.lo); w.push_back(r.mid); w.push_back(r.hi); w.push_back(r.rids); }
        for (size_t i = 0; i < rows.size(); i += 2) {
            uint32_t at[kWsumMaxDepth];
            for (int s2 = 0; s2 < kWsumMaxDepth; ++s2) {
                const int rid = (rows[i + 1] >> (8 * s2)) & 0xFF;
                at[s2] = (uint32_t)(rid == kWsumNone ? dump : c_rw + kXf * rid) & 0xFFFFu;
            }
            w.push_back(rows[i]); w.push_back((int32_t)(at[0] | at[1] << 16)); w.push_back((int32_t)(at[2] | at[3] << 16)); w.push_back(rows[i + 1]);
        }
        return w;
    }
    int32_t counts() const { return ntask | nwhole << 8 | nrows << 16 | depth << 24; }
};
struct stac_model {
    int device = 0;   // the HIP device the model lives on: every entry point runs with it current (and restores)
    int cus = 256;    // its compute units (hipDeviceAttributeMultiprocessorCount: 256 on a whole MI355X; fewer on a partition or under a CU mask):
                      // the launch heuristics (resident chains, chain queue, placement by SIMD load) count with them
    DebugSwitches dbg;
    float *d_bounds = nullptr;          // [2 nqpad] per-call lb / ub of stac_q_solve
    std::vector<float> bounds_cache;    // what d_bounds holds
    PlanHeader h{};
    std::vector<float> blob_host;  // plan blob (host mirror)
    float *d_blob = nullptr;       // device plan blob
    // full tables on device
    int32_t *d_body_parentid = nullptr, *d_body_jntadr = nullptr, *d_body_jntnum = nullptr;
    float *d_body_pos = nullptr, *d_body_quat = nullptr;
    int32_t *d_jnt_type = nullptr, *d_jnt_qposadr = nullptr;
    float *d_jnt_pos = nullptr, *d_jnt_axis = nullptr, *d_qpos0 = nullptr;
    int32_t *d_site_bodyid = nullptr;
    int32_t *d_fk_brec = nullptr, *d_fk_jrec = nullptr, *d_fk_sites = nullptr;  // packed tables of fk_kernel (build_fk_tables)
    int fk_nslots = 0;
    float *d_site_pos = nullptr;  // [K,3] offsets for the stand-alone FK / m-phase kernels (mirrors the plan's SiteRec.pos)
    uint32_t *d_order = nullptr;  // chain order / placement work space: [3K floats rest sites][4096 buckets][kPlaceWords][C key bits][C perm]
    size_t order_chains = 0;
    uint8_t *d_masks = nullptr;  // [kMaxKinds, nqpad] + [K] + [3K]
    std::vector<uint8_t> masks_cache;  // what d_masks currently holds (uploads + their sync happen only on change)
    // host copies of the plan's structure, used to build the LM solver's per-kind tables
    std::vector<int> h_ab_parent, h_aj_type, h_aj_qadr, h_aj_slot, h_aj_slo, h_aj_shi, h_sortpos;
    // what build_fk_program needs (the root passes get a pruned program per call)
    std::vector<BodyRec> h_brec;
    std::vector<int> h_lev_adr, h_ab_jadr, h_ab_jnum, h_xf, h_site_slot;
    std::vector<float> h_aj_pos;
    int n_mlev_root = 0;        // micro-levels of the root-pass program currently in the blob (0 = none)
    int n_run_root = 0;         // of which the leading ones have work (n_mlev_root is padded to an even count)
    WsumProgram wsum;           // the wrench-sum program of the lean 16-lane throughput kernels
    int off_wsum = 0;           // ... and where its table stands in the blob (0: the model has none)
    PlanHeader h3{};            // h with the chain layout of a lean launch (split kinematics, PlanHeader::fk3); valid when h.fk3
    int fk3r = 0;  // the pruned FK3 program currently in the blob: its counts packed like PlanHeader::fk3_n (0: none)
    std::vector<float> h_bpos;  // body_pos of the active bodies, by slot
    int32_t *d_lm_tab = nullptr;
    size_t lm_tab_words = 0;
    std::vector<int32_t> lm_tab_cache;
    LmArgs lm_args{};
    size_t masks_bytes = 0;
    int32_t *d_ctl = nullptr;    // straggler hand-off: {finished, threshold, handed off, capacity}
    float *d_hand = nullptr;     // [hand_cap][3 nqpad + 12] solver states in transit
    int hand_cap = 0;
    float *d_scratch = nullptr;  // unused: fk_kernel keeps the outputs a caller does not want in LDS, nothing grows this any more
    size_t scratch_floats = 0;
    int max_depth = 0;
    FullModel full() const {
        FullModel M{};
        M.nbody = h.nbody; M.njnt = h.njnt; M.nq = h.nq; M.K = h.K;
        M.body_parentid = d_body_parentid; M.body_jntadr = d_body_jntadr; M.body_jntnum = d_body_jntnum;
        M.body_pos = d_body_pos; M.body_quat = d_body_quat;
        M.jnt_type = d_jnt_type; M.jnt_qposadr = d_jnt_qposadr;
        M.jnt_pos = d_jnt_pos; M.jnt_axis = d_jnt_axis; M.qpos0 = d_qpos0;
        M.site_bodyid = d_site_bodyid;
        M.site_pos = d_site_pos;
        M.fk_brec = d_fk_brec; M.fk_jrec = d_fk_jrec; M.fk_sites = d_fk_sites; M.fk_nslots = fk_nslots;
        return M;
    }
};

// ---- plan construction and shape arithmetic (stac_planner.hip: no HIP call) ----------------------------------------------------
struct FkTables {  // the packed tables of fk_kernel (build_fk_tables)
    std::vector<int32_t> brec, jrec, sites;
    int nslots = 0;
};
struct Fk3Program {  // the three tables of a split-kinematics program (build_fk3_program)
    std::vector<int32_t> words;   // T1 [16 (cap1 + 2)] (cap1 / 2 + 3 records of 24 words), T2 [cap2][4], T3 [cap3 * 4] (cap3 + 12 used), site words [K], joint words [naj]
    int n1 = 0, n2 = 0, n3 = 0;
    int nrot = 0;                 // rotations of P2 before the padding (n2: with the no-op tasks that fill its last round)
};
struct QShape { int wpb, wpe, waves_per_cu; };
struct SpecShape { int G, chains_per_block, waves_per_block; long resident; };  // resident = chains the chip holds at once
constexpr size_t kLdsPerCu = 160 * 1024;
constexpr int kFullCus = 256;  // a whole MI355X (the placement kernel's SIMD census is laid out for it)
// latency mode: up to this many chains a chain is spread over 8 / 4 wavefronts of a workgroup (else one per chain)
// (measured, rodent, 250-frame clips, profiles/r02/lat_sweep.txt: with the four-lanes-per-position kinematics four
// wavefronts per chain are 6-12 % ahead of eight from 40 to 256 chains and hold twice as many chains: eight are kept
// behind STAC_HIP_SPECG=64)
constexpr long kSpec64MaxChains = 0, kSpec32MaxChains = 512;
// one wavefront per chain: FOUR roles of 16 lanes (two candidates and their momentum points per trip: 1.16 trips per
// iteration, but the four-lanes-per-position kinematics and fewer rounds in every per-item phase): measured 229 k against
// 179 k frames/s on 1 000 x 250 clips for eight roles of 8 lanes (which stay behind STAC_HIP_SPECG=8)
constexpr int kLatG = 16, kLatR = 4;
constexpr int kOrderMinChains = 2048, kOrderMaxFrames = 8;  // stac_q_phase: chains ordered by expected length and placed by SIMD load
// latency mode with 4 roles per chain from this many chains on (never auto-selected below: developer switch STAC_HIP_SPECR)
constexpr long kSpec4MinChains = 1L << 40;

FkTables build_fk_tables(const stac_model_tables *t);
int build_plan(stac_model *m, const stac_model_tables *t);
std::vector<int32_t> build_fk_program(const stac_model *m, const char *need, int *n_mlev_out, int *uniform_out = nullptr,
                                      int ja_keep = 1 << 30,  // joints >= ja_keep park their anchor / pre-joint entry in the sink
                                      int *n_run_out = nullptr);
bool build_fk3_program(const stac_model *m, const PlanHeader &h3, const char *need, int cap1, int cap2, int cap3, Fk3Program &out);
int root_pass_bodies(const stac_model *m, const uint8_t *trunk_kps, std::vector<char> &need);
void rebase_plan_offsets(PlanHeader &h);
int q_mb_words(int nkinds, int G);
int q_chain_stride(const PlanHeader &h, int G);
size_t q_lds_bytes(const PlanHeader &h, int G, int nkinds, int wpb);
int blocks_per_cu(size_t lds_bytes, int wpb, int waves_per_simd);
QShape pick_shape(const PlanHeader &h, int G, int nkinds, int cus, long waves_needed, QKind kind);
size_t spec_lds_bytes(const PlanHeader &h, int G, int nkinds, int chains, int nr = 8);  // nr = evaluation roles per chain
bool lat_one_wave_ok(const PlanHeader &h);
SpecShape pick_spec_shape(const PlanHeader &h, int G, int nkinds, int cus, long nchains = -1, int nr = 8);
bool lean_holds(const PlanHeader &h, QKind kind, int G, int third);
bool thr_lean_holds(const PlanHeader &h, int G);

// stac_model.hip: the kinematics of N poses behind stac_fk (normalize = 0: the quaternions of qpos are taken as they are)
int fk_impl(const stac_model *mc, const float *qpos, int32_t N, float *qn, float *xpos, float *xquat, float *site_xpos, int normalize, void *stream);
#pragma GCC visibility pop
