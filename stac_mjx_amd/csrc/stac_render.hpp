// Shared layout of the render kernel (stac_render.hip) and its host entry points (stac_abi.hip).
#pragma once

#include <stdint.h>

namespace stac {

constexpr int kRenderTile = 16;       // one workgroup = one 16 x 16 tile of one frame
constexpr int kRenderRecWords = 20;   // per-frame primitive record in LDS (80 B): see build_prim
constexpr int kRenderMaxPrims = 512;  // STAC_RENDER_MAX_PRIMS: 512 x 80 B records + the 2 KB culled list = 42 KB of LDS
constexpr int kRenderLayers = 8;      // STAC_RENDER_LAYERS

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
