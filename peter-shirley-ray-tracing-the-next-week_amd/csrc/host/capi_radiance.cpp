// capi_radiance.cpp — radiance queries on caller-supplied rays (rt_hip.h rt_radiance_rays and
// its _dev form; rt_megakernel.h kRays, rt_kernel_rays.hip): the argument checks
// and the launch of the megakernel's ray-source variant.
#include <cmath>

#include "capi_internal.h"

// the rays unit's launchers, set by its static initialiser (rt_kernel.h)
RtRaysLaunch rt_rays_launch = {nullptr, nullptr};

#define RT_PATH_RAY_BYTES 48
#define RT_RADIANCE_BYTES 16
static_assert(sizeof(rt_path_ray) == RT_PATH_RAY_BYTES && sizeof(rt_radiance) == RT_RADIANCE_BYTES,
              "rt_path_ray is three 16-B words, rt_radiance one");

// The argument checks of both entry points in rt_hip.h's order, the scene's last: all before
// any HIP call.  RT_OK with *empty set: n == 0, nothing to do (whatever the other arguments are).
static int radiance_check(const char *fn, const rt_scene *s, const rt_render_params *p, const void *rays, int64_t n,
                          const void *out, bool *empty) {
    const std::string f(fn);
    RT_TRY(ray_count_check(f, n, empty));
    if (*empty) return RT_OK;
    if (!p) return fail(RT_ERR_INVALID, f + ": null parameters");
    if (!rays) return fail(RT_ERR_INVALID, f + ": null rays");
    if (!out) return fail(RT_ERR_INVALID, f + ": null output");
    if (p->max_depth < 0) return fail(RT_ERR_INVALID, f + ": max_depth < 0");
    if (!std::isfinite(p->t_min)) return fail(RT_ERR_INVALID, f + ": t_min is not finite");
    if (p->background != RT_BG_BLACK && p->background != RT_BG_SKY) return fail(RT_ERR_INVALID, f + ": background outside RT_BG_*");
    if (p->flags != 0) return fail(RT_ERR_INVALID, f + ": no flag applies (there are no right-fold, counting or profiling forms)");
    RT_TRY(scene_check(f, s));
    if (!rt_rays_launch.launch) return unit_missing(f, "rays", "rt_kernel_rays.o");
    return RT_OK;
}

// One launch over n records.  The search mode is the one the scene's renders use (flat scan, BVH2
// in LDS, BVH in HBM), except that a BVH2 the ray-source variant's LDS has no room for stays in
// HBM; the claim sizes are a render's of n one-sample items (rtnw::plan_batch).
int radiance_launch(rt_scene *s, const rt_render_params *p, const void *rays_dev, uint32_t n, void *out_dev,
                           hipStream_t stream) {
    RtKernelArgs a{};
    fill_scene_args(s, a);
    const int search_want = s->scan ? 2 : (s->lds_nodes ? 1 : 0);
    int bpc = 0, block = 0;
    HIP_TRY(rt_rays_launch.plan(search_want, s->stack_depth, &bpc, &block));
    int search = search_want;
    if (search == 1 && bpc == 0) {
        search = 0;
        HIP_TRY(rt_rays_launch.plan(0, s->stack_depth, &bpc, &block));
    }
    a.lds_nodes = search == 1 ? 1 : 0;
    const int grid = std::max(1, bpc) * s->cus;
    a.features = RT_FEAT_ALL;
    a.need_dlen = s->nmedia > 0 || s->has_specular || p->background == RT_BG_SKY;
    fill_sampler_args(a);
    a.nx = a.ny = 1;
    a.rnx = a.rny = 1.0f;
    a.ns = 1;
    a.chunk = 1;
    a.nchunks = 1;
    a.max_depth = p->max_depth;
    a.tmin = p->t_min;
    a.background = p->background;
    a.seed = p->seed;
    a.npix = n;
    rtnw::BatchPlan plan{1, 1, 1};
    const rtnw::BatchLaunch l = rtnw::plan_batch(plan, 0, n, 1, 1, 0, (uint64_t)grid * (block / 64), 0, -1, -1);
    a.nitems = l.nitems;
    a.claim = l.claim;
    a.claim_tail = l.claim_tail;
    a.nbig = l.nbig;
    a.counter = (uint32_t *)s->counter.p;
    a.rays = (const float4 *)rays_dev;
    a.radiance = (float4 *)out_dev;
    a.rays_moving = s->has_moving ? 1 : 0;
    a.rays_t0 = s->time0;
    a.rays_t1 = s->time1;
    HIP_TRY(hipMemsetAsync(s->counter.p, 0, 64, stream));
    HIP_TRY(rt_rays_launch.launch(&a, grid, stream));
    return RT_OK;
}

extern "C" {

int rt_radiance_rays(rt_scene *s, const rt_render_params *p, const rt_path_ray *rays, int64_t n, rt_radiance *out, double *ms) {
    bool empty;
    if (int rc = radiance_check("rt_radiance_rays", s, p, rays, n, out, &empty)) return rc;
    if (empty) return RT_OK;
    return ray_batches(s, rays, RT_PATH_RAY_BYTES, out, RT_RADIANCE_BYTES, n, "RTNW_RADIANCE_BATCH", ms,
                       [&](const void *rays_dev, uint32_t m, void *out_dev, hipStream_t stream) {
                           return radiance_launch(s, p, rays_dev, m, out_dev, stream);
                       });
}

int rt_radiance_rays_dev(rt_scene *s, const rt_render_params *p, const rt_path_ray *rays_dev, int64_t n, rt_radiance *out_dev,
                         void *stream) {
    bool empty;
    if (int rc = radiance_check("rt_radiance_rays_dev", s, p, rays_dev, n, out_dev, &empty)) return rc;
    if (empty) return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    return radiance_launch(s, p, rays_dev, (uint32_t)n, out_dev, (hipStream_t)stream);
}

}  // extern "C"
