// Shared layout of the render kernel (stac_render.hip) and its host entry points (below the kernel).
#pragma once

#include <stdint.h>

namespace stac {

constexpr int kRenderTile = 16;       // one workgroup = one 16 x 16 tile of one frame
constexpr int kRenderRecWords = 20;   // per-frame primitive record in LDS (80 B): see build_prim
constexpr int kRenderMaxPrims = 512;  // STAC_RENDER_MAX_PRIMS: 512 x 80 B records + the 2 KB culled list = 42 KB of LDS
constexpr int kRenderLayers = 8;      // STAC_RENDER_LAYERS
constexpr int kRenderNodeWords = 8;   // mesh hierarchy node (32 B): lo[3], hi[3], then the bit patterns of (first, count) of a
                                      // leaf (count > 0) or (skip, 0) of an inner node; a leaf's skip is the next node
constexpr int kRenderTriBits = 20;    // STAC_RENDER_MAX_MESH_TRIS = 2^20: the triangle index in the pixel's hit key

// Scene tables on the device (stac_render_scene_create uploads stac_render_tables into one int and one float block).
struct RenderScene {
    int P, K, nbody, nlight;
    const int32_t *prim_type, *prim_body, *prim_flags;
    const float *prim_size, *prim_pos, *prim_quat, *prim_rgba, *prim_rgb2, *prim_tex;
    const float *kp_rgba, *light_dir, *light_diff;
    float marker_rgba[4], seg_rgba[4];
    float marker_r, seg_r;
    float head_amb[3], head_diff[3];
    float alpha;
    float bg[3];
    // meshes (stac_render_scene_create_with_meshes; all null / 0 in a scene without a type-7 primitive)
    int nmesh;
    const int32_t *prim_mesh, *mesh_node_off, *mesh_tri_off;  // [P], [nmesh+1], [nmesh+1]
    const float *mesh_nodes, *mesh_tris;                      // [NN,kRenderNodeWords], [NT,3,3] in device global memory
};

struct RenderCall {
    int N, W, H, show_error;
    const float *xpos, *xquat, *kp, *markers, *cam;
    float tanh;
    uint8_t *rgb;
    int32_t *seg;
    float *depth;
};

}  // namespace stac
