// Ground clearance of fitted poses (rule: stac_ground.hpp; entry point: below the kernel; C ABI: stac_ground.h).
//
// One kernel, one wavefront per workgroup, ground_tiles_per_group consecutive tiles of kGroundTile frames per workgroup:
//   ground_clearance_kernel   lane l owns frame l of the tile.  The bodies pass through LDS kGroundBodyChunk at a time: the chunk's
//                             quaternions of the tile's frames are one run of consecutive 16-byte loads per frame, a lane turns each
//                             into the z row of its rotation, adds xpos' z and stores the four words at [word][body][frame], rows
//                             of kGroundTilePitch words (a store's lanes differ in the body, a load's in the frame: both meet every
//                             bank once).  Then every lane walks the geom table together: the table row, the type switch and a
//                             mesh's vertices are the same for the wavefront (scalar loads, no divergence), geoms of other chunks
//                             are passed over.  A lane keeps its frame's lowest included geom as a key and an index and the slots'
//                             keys in LDS words that it alone reads and writes; per geom the wavefront reduces the key (__shfl_xor)
//                             and counts the frames below z_ref (__ballot), and lane 0 folds both into the workgroup's two LDS words
//                             of the geom.  After its tiles lane l merges the geoms l, l + 64, ... into geom_min -- an integer
//                             atomic on the float's bits, a signed minimum for a value >= +0 and an unsigned maximum for one below,
//                             which together are the minimum in ground_key's order, and only where a plain read shows a larger value
//                             -- and into geom_below with an integer atomic add.
// Offsets are 64-bit element offsets.  Nothing returns to the host, no workgroup waits for another, no workspace, no scratch.
#include <hip/hip_runtime.h>

#include <string>

#include "stac_ground.h"
#include "stac_ground.hpp"

using namespace stac;

namespace {

constexpr int kGroundThreads = kGroundTile;

__device__ inline void ground_merge_min(float *dst, uint32_t key) {
    const uint32_t cur = __atomic_load_n((const uint32_t *)dst, __ATOMIC_RELAXED);  // (stale at worst: the word only ever falls)
    if (key >= ground_key(ground_float(cur))) return;
    const uint32_t bits = ground_bits(ground_unkey(key));
    if (bits & 0x80000000u) atomicMax((unsigned int *)dst, bits);
    else atomicMin((int *)dst, (int)bits);
}

__global__ __launch_bounds__(kGroundThreads) void ground_clearance_kernel(
    const float *__restrict__ xpos, const float *__restrict__ xquat, int64_t N, int32_t nbody, const int32_t *__restrict__ meta,
    const float *__restrict__ data, int32_t G, const float *__restrict__ verts, int32_t V, int32_t S, float z_ref, int64_t tiles_per_group,
    float *__restrict__ low_z, int32_t *__restrict__ low_geom, float *__restrict__ track_z, float *__restrict__ geom_min,
    unsigned long long *__restrict__ geom_below) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int32_t chunk = nbody < kGroundBodyChunk ? nbody : kGroundBodyChunk;
    float *body = (float *)smem;                                    // [4][chunk][kGroundTilePitch]: bz0, bz1, bz2, xpos z
    uint32_t *track = (uint32_t *)(body + 4 * chunk * kGroundTilePitch);  // [S][64] keys, a lane's own column
    uint32_t *gmin = track + S * kGroundTile;                        // [G] keys
    uint32_t *gcnt = gmin + G;                                       // [G]
    const int lane = threadIdx.x;
    for (int32_t g = lane; g < G; g += kGroundThreads) gmin[g] = kGroundKeyInf, gcnt[g] = 0;
    const int64_t n_tiles = (N + kGroundTile - 1) / kGroundTile;
    const int64_t tile0 = (int64_t)blockIdx.x * tiles_per_group;
    const int64_t tile1 = tile0 + tiles_per_group < n_tiles ? tile0 + tiles_per_group : n_tiles;
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t t0 = tile * kGroundTile;
        const int32_t nf = N - t0 < kGroundTile ? (int32_t)(N - t0) : kGroundTile;  // frames of this tile
        const bool active = lane < nf;
        uint32_t low = kGroundKeyInf, tbad = 0;
        int32_t low_g = -1;
        bool bad = false;
        for (int32_t s = 0; s < S; ++s) track[s * kGroundTile + lane] = kGroundKeyInf;
        for (int32_t b0 = 0; b0 < nbody; b0 += kGroundBodyChunk) {
            const int32_t cb = nbody - b0 < kGroundBodyChunk ? nbody - b0 : kGroundBodyChunk;  // bodies of this chunk
            __syncthreads();  // (one wavefront: orders the walk of the chunk before against the stores below)
            // item e = f * cb + b of the chunk: lane, lane + 64, ...; f and b advance without a division
            const int32_t q64 = kGroundThreads / cb, r64 = kGroundThreads % cb;
            int32_t f = lane / cb, b = lane % cb;
            for (int32_t e = lane; e < nf * cb; e += kGroundThreads) {
                const int64_t row = (t0 + f) * nbody + b0 + b;
                const float4 q = *(const float4 *)(xquat + row * 4);
                float bz[3];
                ground_body_row(q.x, q.y, q.z, q.w, bz);
                body[(0 * chunk + b) * kGroundTilePitch + f] = bz[0];
                body[(1 * chunk + b) * kGroundTilePitch + f] = bz[1];
                body[(2 * chunk + b) * kGroundTilePitch + f] = bz[2];
                body[(3 * chunk + b) * kGroundTilePitch + f] = xpos[row * 3 + 2];
                f += q64, b += r64;
                if (b >= cb) b -= cb, ++f;
            }
            __syncthreads();
            for (int32_t g = 0; g < G; ++g) {
                const int32_t *m = meta + (int64_t)g * kGroundMetaWords;
                const int32_t gb = m[kGroundBody] - b0, type = m[kGroundType], slot = m[kGroundSlot];
                if (gb < 0 || gb >= cb) continue;  // a body of another chunk
                // the entry point checked the host copy of the table; a device copy that differs from it is passed over, never followed
                const int32_t vf = m[kGroundVertFirst], vc = m[kGroundVertCount];
                if (type < kGroundSphere || type > kGroundMesh || slot >= S) continue;
                if (type == kGroundMesh && (vc < 1 || vf < 0 || (int64_t)vf + vc > V)) continue;
                const float bz[3] = {body[(0 * chunk + gb) * kGroundTilePitch + lane], body[(1 * chunk + gb) * kGroundTilePitch + lane],
                                     body[(2 * chunk + gb) * kGroundTilePitch + lane]};
                const float z = ground_geom_z(body[(3 * chunk + gb) * kGroundTilePitch + lane], bz, type, data + (int64_t)g * kGroundDataWords,
                                              verts, vf, vc);
                const bool fin = active && ground_finite(z);
                const uint32_t k = fin ? ground_key(z) : 0xFFFFFFFFu;
                if (m[kGroundInclude]) {
                    bad |= active && !fin;
                    if (k < low) low = k, low_g = g;  // (within a chunk g ascends; across chunks the smaller index wins below)
                    else if (fin && k == low && g < low_g) low_g = g;
                }
                if (slot >= 0) {
                    if (!fin) tbad |= 1u << slot;
                    else if (k < track[slot * kGroundTile + lane]) track[slot * kGroundTile + lane] = k;
                }
                uint32_t kmin = k;
#pragma unroll
                for (int s = 1; s < kGroundThreads; s <<= 1) {
                    const uint32_t o = __shfl_xor(kmin, s, kGroundThreads);
                    kmin = o < kmin ? o : kmin;
                }
                const uint32_t below = (uint32_t)__popcll(__ballot(fin && z < z_ref));
                if (lane == 0) {
                    if (kmin < gmin[g]) gmin[g] = kmin;
                    gcnt[g] += below;
                }
            }
        }
        if (active) {
            low_z[t0 + lane] = bad ? ground_quiet_nan() : ground_unkey(low);
            low_geom[t0 + lane] = bad ? -1 : low_g;
            for (int32_t s = 0; s < S; ++s)
                track_z[(t0 + lane) * S + s] = ((tbad >> s) & 1u) ? ground_quiet_nan() : ground_unkey(track[s * kGroundTile + lane]);
        }
    }
    __syncthreads();
    for (int32_t g = lane; g < G; g += kGroundThreads) {
        if (gmin[g] < kGroundKeyInf) ground_merge_min(geom_min + g, gmin[g]);
        if (gcnt[g]) atomicAdd(geom_below + g, (unsigned long long)gcnt[g]);
    }
}

// ---- error state of the calling thread (this library's own: it does not link against libstac_hip.so) ------------------------------
thread_local std::string g_err;
thread_local int32_t g_err_code = 0;
int fail(int code, const std::string &msg) {
    g_err = msg;
    g_err_code = code;
    return code;
}

struct Buf { const char *name; uintptr_t lo; int64_t bytes; int align; };

// Null, then alignment, then overlap, one text each
int check_buffers(const char *who, const Buf *buf, int n) {
    for (int i = 0; i < n; ++i)
        if (!buf[i].lo) return fail(STAC_ERR_INVALID, std::string(who) + ": null " + buf[i].name);
    for (int i = 0; i < n; ++i)
        if (buf[i].lo % buf[i].align != 0)
            return fail(STAC_ERR_INVALID, std::string(who) + ": " + buf[i].name + " must be " + std::to_string(buf[i].align) + "-byte aligned");
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (buf[i].lo < buf[j].lo + (uintptr_t)buf[j].bytes && buf[j].lo < buf[i].lo + (uintptr_t)buf[i].bytes)
                return fail(STAC_ERR_INVALID, std::string(who) + ": " + buf[i].name + " and " + buf[j].name +
                                                  " overlap: the inputs and the five outputs are distinct buffers");
    return STAC_OK;
}

}  // namespace

// ---- C ABI entry points (stac_ground.h): every argument is checked before the device is touched -----------------------------------
extern "C" const char *stac_ground_last_error(void) { return g_err.c_str(); }
extern "C" int32_t stac_ground_last_error_code(void) { return g_err_code; }

extern "C" int32_t stac_ground_clearance(const float *xpos, const float *xquat, int64_t n_frames, int32_t nbody, const int32_t *geom_meta_host,
                                         const int32_t *geom_meta, const float *geom_data, int32_t n_geoms, const float *verts, int32_t n_verts,
                                         int32_t n_slots, float z_ref, float *low_z, int32_t *low_geom, float *track_z, float *geom_min,
                                         int64_t *geom_below, void *stream) {
    const std::string who = "stac_ground_clearance";
    if (n_frames < 1 || n_frames > kGroundMaxFrames)
        return fail(STAC_ERR_INVALID, who + ": n_frames = " + std::to_string(n_frames) + " is outside 1 .. 2^40");
    if (nbody < 2) return fail(STAC_ERR_INVALID, who + ": nbody >= 2 (the world and a body), got " + std::to_string(nbody));
    if (nbody > kGroundMaxBodies)
        return fail(STAC_ERR_CAPACITY, who + ": nbody = " + std::to_string(nbody) + " exceeds the " + std::to_string(kGroundMaxBodies) + " bodies of a call");
    if (n_geoms < 1) return fail(STAC_ERR_INVALID, who + ": n_geoms >= 1, got " + std::to_string(n_geoms));
    if (n_geoms > kGroundMaxGeoms)
        return fail(STAC_ERR_CAPACITY, who + ": n_geoms = " + std::to_string(n_geoms) + " exceeds the " + std::to_string(kGroundMaxGeoms) + " geoms of a table");
    if (n_verts < 0) return fail(STAC_ERR_INVALID, who + ": n_verts >= 0, got " + std::to_string(n_verts));
    if (n_verts > kGroundMaxVerts)
        return fail(STAC_ERR_CAPACITY, who + ": n_verts = " + std::to_string(n_verts) + " exceeds the " + std::to_string(kGroundMaxVerts) + " vertices of a table");
    if (n_slots < 0 || n_slots > kGroundMaxSlots)
        return fail(STAC_ERR_INVALID, who + ": n_slots = " + std::to_string(n_slots) + " is outside 0 .. " + std::to_string(kGroundMaxSlots));
    if (!geom_meta_host) return fail(STAC_ERR_INVALID, who + ": null geom_meta_host (host memory)");
    for (int32_t g = 0; g < n_geoms; ++g) {
        const int32_t *m = geom_meta_host + (int64_t)g * kGroundMetaWords;
        const std::string geom = who + ": geom " + std::to_string(g) + ": ";
        switch (ground_check_geom(m, nbody, n_slots, n_verts)) {
            case 0: break;
            case 1: return fail(STAC_ERR_INVALID, geom + "unknown type " + std::to_string(m[kGroundType]) + " (sphere 2 .. mesh 7)");
            case 2: return fail(STAC_ERR_INVALID, geom + "body " + std::to_string(m[kGroundBody]) + " is outside 1 .. nbody - 1 = " + std::to_string(nbody - 1));
            case 3: return fail(STAC_ERR_INVALID, geom + "include must be 0 or 1, got " + std::to_string(m[kGroundInclude]));
            case 4: return fail(STAC_ERR_INVALID, geom + "slot " + std::to_string(m[kGroundSlot]) + " is outside -1 .. n_slots - 1 = " + std::to_string(n_slots - 1));
            default: return fail(STAC_ERR_INVALID, geom + "mesh range " + std::to_string(m[kGroundVertFirst]) + " + " + std::to_string(m[kGroundVertCount]) +
                                                       " is empty or outside the " + std::to_string(n_verts) + " vertices");
        }
    }
    Buf buf[10] = {{"xpos", (uintptr_t)xpos, n_frames * nbody * 12, 4},
                   {"xquat", (uintptr_t)xquat, n_frames * nbody * 16, 16},
                   {"geom_meta", (uintptr_t)geom_meta, (int64_t)n_geoms * kGroundMetaWords * 4, 4},
                   {"geom_data", (uintptr_t)geom_data, (int64_t)n_geoms * kGroundDataWords * 4, 4},
                   {"low_z", (uintptr_t)low_z, n_frames * 4, 4},
                   {"low_geom", (uintptr_t)low_geom, n_frames * 4, 4},
                   {"geom_min", (uintptr_t)geom_min, (int64_t)n_geoms * 4, 4},
                   {"geom_below", (uintptr_t)geom_below, (int64_t)n_geoms * 8, 8}};
    int n = 8;
    if (n_slots > 0) buf[n++] = {"track_z", (uintptr_t)track_z, n_frames * n_slots * 4, 4};
    if (n_verts > 0) buf[n++] = {"verts", (uintptr_t)verts, (int64_t)n_verts * 12, 4};
    if (const int rc = check_buffers(who.c_str(), buf, n)) return rc;
    const int32_t chunk = nbody < kGroundBodyChunk ? nbody : kGroundBodyChunk;
    const size_t lds = ((size_t)4 * chunk * kGroundTilePitch + (size_t)n_slots * kGroundTile + 2 * (size_t)n_geoms) * 4;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (lds > 64 * 1024)  // (a large table: more than the default bound of a launch's dynamic LDS)
        e = hipFuncSetAttribute((const void *)ground_clearance_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)geom_min, (int)0x7F800000, (size_t)n_geoms, s);  // +inf
    if (e == hipSuccess) e = hipMemsetAsync(geom_below, 0, (size_t)n_geoms * 8, s);
    if (e != hipSuccess) return fail(STAC_ERR_HIP, who + ": " + hipGetErrorString(e));
    const int64_t per_group = ground_tiles_per_group(n_frames);
    const int64_t tiles = (n_frames + kGroundTile - 1) / kGroundTile;
    const unsigned groups = (unsigned)((tiles + per_group - 1) / per_group);
    hipLaunchKernelGGL(ground_clearance_kernel, dim3(groups), dim3(kGroundThreads), lds, s, xpos, xquat, n_frames, nbody, geom_meta, geom_data,
                       n_geoms, verts, n_verts, n_slots, z_ref, per_group, low_z, low_geom, track_z, geom_min, (unsigned long long *)geom_below);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(STAC_ERR_HIP, who + ": " + hipGetErrorString(e));
    return fail(STAC_OK, "");
}
