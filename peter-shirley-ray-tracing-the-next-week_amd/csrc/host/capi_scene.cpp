// capi_scene.cpp — rt_scene_create / rt_scene_destroy: the lowered scene (scene_lower.cpp)
// uploaded to HBM, and what its launches need from the device (grid, LDS variant).
#include <memory>
#include <mutex>

#include "capi_internal.h"

namespace {

// the cache slot of a width (rt_megakernel_occupancy's: 0 is the flat scan): BVH2, BVH4, flat
// scan, BVH8, compressed BVH8
int width_slot(int width) {
    switch (width) {
    case 4: return 1;
    case 0: return 2;
    case 8: return 3;
    case RT_BVH_CW8: return 4;
    default: return 0;
    }
}
// Resident workgroups per CU of the megakernel, per launch mode and BVH width: a
// property of the code objects, queried once per process.
hipError_t occupancy(int *mega, int mode, int width) {
    static std::mutex mu;
    static int cache[3][5] = {};   // [mode][width_slot]
    std::lock_guard<std::mutex> lock(mu);
    int &c = cache[mode][width_slot(width)];
    if (!c) {
        hipError_t e;
        if ((e = rt_megakernel_occupancy(&c, mode, width)) != hipSuccess) { c = 0; return e; }
    }
    *mega = c;
    return hipSuccess;
}

}  // namespace

// The kernel features (RT_FEAT_*) a scene's launches carry code for: the launcher runs the
// smallest compiled variant covering them (rt_kernel_launch.h with_variant).  RTNW_FEAT_ALL=1
// runs the all-feature variant (the one the wide BVHs use): A/B runs only.
int scene_features(const rt_scene *s) {
    if (const char *e = std::getenv("RTNW_FEAT_ALL"))
        if (std::atoi(e)) return RT_FEAT_ALL;
    return (s->ninstances > 0 ? RT_FEAT_INST : 0) | (s->has_uv ? RT_FEAT_UV : 0) |
           (s->has_checker ? RT_FEAT_CHECKER : 0) | (s->nprescan > 0 ? RT_FEAT_PRESCAN : 0) |
           (s->nmedia > 0 ? RT_FEAT_MEDIA : 0);
}

// the scene's own stream (the host-buffer paths) is created on first use: creating a
// stream next to a framework's can take milliseconds
int ensure_own_stream(rt_scene *s) {
    if (!s->own_stream) HIP_TRY(hipStreamCreateWithFlags(&s->own_stream, hipStreamNonBlocking));
    return RT_OK;
}

// Grid and LDS variant of the scene's launches on its device.
static int device_attributes(rt_scene *s) {
    hipError_t e;
    if ((e = hipDeviceGetAttribute(&s->cus, hipDeviceAttributeMultiprocessorCount, s->device)) != hipSuccess)
        return hip_fail(e, "hipDeviceGetAttribute");
    for (int mode = 0; mode < 3; mode++) {
        int bpc = 0;
        if ((e = occupancy(&bpc, mode, s->scan ? 0 : s->bvh_width)) != hipSuccess) return hip_fail(e, "occupancy query");
        // RTNW_BLOCKS_PER_CU caps the resident workgroups per CU (occupancy experiments only)
        if (const char *e = std::getenv("RTNW_BLOCKS_PER_CU")) bpc = std::min(bpc, std::max(1, std::atoi(e)));
        s->grid[mode] = std::max(1, bpc) * s->cus;
    }
    // LDS-resident BVH2 (rt_kernel.h): nodes as 4 planes + one stack per lane of the
    // scene's own depth, if both fit the CU's LDS beside the variant's static arrays.
    // RTNW_LDS_BVH=0 keeps the nodes in HBM (A/B, tests).  Primitive heads in LDS as
    // well (with 16-bit stack entries to make room) measured no faster: 60.27 vs
    // 60.29 ms on c4, both behind 32-bit entries with the nodes alone.
    s->stack_depth = s->bvh_depth + 1;
    // the variant this scene launches (its static arrays and node layout: rt_lds_need_bytes)
    const long need_actual = rt_lds_need_bytes(scene_features(s), s->stack_depth);
    bool want = true;
    if (const char *e = std::getenv("RTNW_LDS_BVH")) want = std::atoi(e) != 0;
    // the budget is this device's LDS per CU (160 KiB on gfx950), and the static part
    // the compiled variant's own (hipFuncGetAttributes) if larger than the estimate:
    // a scene that does not fit keeps its nodes in HBM instead of failing to launch
    int lds_cu = RT_LDS_BUDGET;
    if (hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, s->device) != hipSuccess ||
        lds_cu <= 0)
        lds_cu = 0;
    s->lds_nodes = want && !s->scan && s->bvh_width == 2 && s->has_bvh && !(s->root & RT_LEAF_BIT) &&
                   s->nnodes <= RT_LDS_NODE_CAP && s->nprims < RT_LDS_MAX_PRIMS &&
                   need_actual <= std::min<long>(RT_LDS_BUDGET, lds_cu);
    if (s->lds_nodes)
        for (int mode = 0; mode < 3; mode++) s->grid[mode] = s->cus;
    return RT_OK;
}

extern "C" {

void rt_scene_destroy(rt_scene *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

int rt_scene_create(const rt_scene_desc *d, int device, rt_scene **out) {
    if (!out) return fail(RT_ERR_INVALID, "rt_scene_create: null out");
    *out = nullptr;
    if (int rc = rtnw::validate_desc(d)) return rc;
    rtnw::PhaseTrace trace{"rt_scene_create"};
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return fail(RT_ERR_HIP, "no HIP device available (the path tracer has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(RT_ERR_INVALID, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    trace("device check");

    rtnw::LoweredScene low;
    if (int rc = rtnw::lower_scene(d, &low)) return rc;   // (traces "BVH build" and "device records")
    trace.last = rtnw::clock_ms();

    std::unique_ptr<rt_scene> s(new rt_scene());   // an error return below frees what it holds by then
    static_cast<rtnw::SceneInfo &>(*s) = low;
    s->device = device;
    if (int rc = s->arena.reserve(low.image.size())) return rc;
    if ((e = hipMemcpy(s->arena.p, low.image.data(), low.image.size(), hipMemcpyHostToDevice)) != hipSuccess)
        return hip_fail(e, "hipMemcpy scene arena");
    uint8_t *base = (uint8_t *)s->arena.p;
    s->nodes = base + low.nodes;
    s->prims = base + low.prims;
    s->bprims = base + low.bprims;
    s->media = base + low.media;
    s->mats = base + low.mats;
    s->texs = base + low.texs;
    s->insts = base + low.insts;
    s->groups = base + low.groups;
    s->ranvec = base + low.ranvec;
    s->perm = base + low.perm;
    s->texels = base + low.texels;
    trace("upload (one allocation)");

    if (int rc = device_attributes(s.get())) return rc;
    trace("device attributes");
    // the work counter (64 B) and the statistics counters in one allocation
    if (int rc = s->counter.reserve(64 + RT_STATS_LEN * sizeof(unsigned long long))) return rc;
    s->stats = (uint8_t *)s->counter.p + 64;
    trace("counters");
    for (int k = 0; k < 3; k++)
        if ((e = hipEventCreate(&s->ev[k])) != hipSuccess) return hip_fail(e, "hipEventCreate");
    trace("events");
    *out = s.release();
    return RT_OK;
}

// Diagnostics (declared in scene_lower.h, not in rt_hip.h): whether scene lowering enables the
// ball waves' fused in-ball step for `d` (scene_lower.cpp ball_fast_media).  Host arithmetic only.
int rt_scene_desc_ball_fast(const rt_scene_desc *d) {
    if (int rc = rtnw::validate_desc(d)) return rc;
    rtnw::LoweredScene low;
    if (int rc = rtnw::lower_scene(d, &low)) return rc;
    return low.ball_fast ? 1 : 0;
}

}  // extern "C"
