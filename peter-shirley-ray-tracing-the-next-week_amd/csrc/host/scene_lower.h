// scene_lower.h — lowering of a scene descriptor to the device's records (scene_lower.cpp):
// host arithmetic only, no HIP, so that it runs, and is tested, without a GPU.
#pragma once
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rt_hip.h"

// sets the thread-local message rt_last_error() returns (capi_util.cpp)
int rt_internal_fail(int code, const std::string &msg);

namespace rtnw {

// What a scene's launches need to know of it besides its arrays.
struct SceneInfo {
    bool scan = false;            // flat scan of the primitive groups instead of the BVH (small scenes)
    int nprescan = 0;             // BVH scenes: largest primitives tested in lockstep before the BVH
    // medium cell: primitives [cell_first, cell_first + cell_n) are copies of those near the ball
    int cell_first = 0, cell_n = 0;
    float cell_c[3] = {0, 0, 0}, cell_r2 = 0, cell_rin2 = 0;
    // the ball waves' fused in-ball step (rt_megakernel.h stage 3) may run: a medium cell, at most
    // two media, each with an isotropic material whose texture the host resolved to a constant
    // (material flag 2); ball_alb: those constants, in list order
    bool ball_fast = false;
    float ball_alb[2][3] = {{0, 0, 0}, {0, 0, 0}};
    int ngroups = 0;
    uint32_t root = 0;
    int has_bvh = 0, nmedia = 0, bvh_depth = 0, nnodes = 0, nprims = 0, bvh_width = 2, ninstances = 0;
    bool has_moving = false;
    bool has_uv = false;       // a material reads (u, v)
    bool has_checker = false;  // a checker_texture exists
    bool has_specular = false; // a metal or dielectric material exists
    float time0 = 0, time1 = 1;
    std::vector<float> deep_balls;          // dense media's boundary balls (cx, cy, cz, r)
    // what the empty-pixel classifier reads (empty_pixels.cpp): every surface primitive's padded
    // world box (prim_bounds: lo xyz, hi xyz), and five floats per primitive: for a plain sphere
    // (no instance chain, not moving) its centre and |radius|, radius -1 for every other
    // primitive; then |radius| for a sphere of any kind, 0 for a rectangle
    std::vector<float> surf_boxes, surf_spheres;
    bool media_plain = true;   // every medium is bounded by one plain sphere (none: true)
};

// The scene's arrays share one image, uploaded by one copy into one device allocation: each
// array starts at its byte offset, 256-B aligned.
struct LoweredScene : SceneInfo {
    std::vector<uint8_t> image;
    size_t nodes = 0, prims = 0, bprims = 0, media = 0, mats = 0, texs = 0, insts = 0, groups = 0, ranvec = 0, perm = 0,
           texels = 0;
};

int validate_desc(const rt_scene_desc *d);

// `d` has passed validate_desc.  RT_OK, or the error of rt_last_error().
int lower_scene(const rt_scene_desc *d, LoweredScene *out);

}  // namespace rtnw

// Diagnostics, exported from the library but not part of rt_hip.h (capi_scene.cpp; the prototype
// tests/test_ball_fast.py binds): 1 when lower_scene enables the ball waves' fused in-ball step
// for `d` (SceneInfo.ball_fast), 0 when not, or the error code (negative).  No HIP call.
extern "C" int rt_scene_desc_ball_fast(const rt_scene_desc *d);

namespace rtnw {

inline double clock_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// RTNW_TRACE: per-phase times of `who` on stderr (diagnostics)
struct PhaseTrace {
    const char *who;
    bool on = std::getenv("RTNW_TRACE") != nullptr;
    double last = clock_ms();
    void operator()(const char *what) {
        if (!on) return;
        const double now = clock_ms();
        std::fprintf(stderr, "%s: %-28s %8.3f ms\n", who, what, now - last);
        last = now;
    }
};

}  // namespace rtnw
