// capi_radiance.cpp — radiance queries on caller-supplied rays (rt_hip.h rt_radiance_rays and
// its _dev form; rt_kernel.hip kRays, rt_kernel_rays.hip): the argument checks,
// the host form's batches and the launch of the megakernel's ray-source variant.
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
    *empty = false;
    if (!rtnw::ray_count_ok(n)) return fail(RT_ERR_INVALID, f + ": n must be in 0..2^31 - 1");
    if (n == 0) {
        *empty = true;
        return RT_OK;
    }
    if (!p) return fail(RT_ERR_INVALID, f + ": null parameters");
    if (!rays) return fail(RT_ERR_INVALID, f + ": null rays");
    if (!out) return fail(RT_ERR_INVALID, f + ": null output");
    if (p->max_depth < 0) return fail(RT_ERR_INVALID, f + ": max_depth < 0");
    if (!std::isfinite(p->t_min)) return fail(RT_ERR_INVALID, f + ": t_min is not finite");
    if (p->background != RT_BG_BLACK && p->background != RT_BG_SKY) return fail(RT_ERR_INVALID, f + ": background outside RT_BG_*");
    if (p->flags != 0) return fail(RT_ERR_INVALID, f + ": no flag applies (there are no right-fold, counting or profiling forms)");
    if (!s) return fail(RT_ERR_INVALID, f + ": null scene");
    if (s->bvh_width != 2) return fail(RT_ERR_UNSUPPORTED, f + " needs a scene with a 2-wide BVH (RTNW_BVH_WIDTH=2)");
    if (!rt_rays_launch.launch)
        return fail(RT_ERR_UNSUPPORTED, f + ": this library was linked without the rays unit (rt_kernel_rays.o)");
    return RT_OK;
}

// One launch over n records.  The search mode is the one the scene's renders use (flat scan, BVH2
// in LDS, BVH in HBM), except that a BVH2 the ray-source variant's LDS has no room for stays in
// HBM; the claim sizes are a render's of n one-sample items (rtnw::plan_batch).
static int radiance_launch(rt_scene *s, const rt_render_params *p, const void *rays_dev, uint32_t n, void *out_dev,
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
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = ensure_own_stream(s)) return rc;
    // batches of rays through the scene's workspace (rays, then records), each copied in, traced
    // and copied out on the scene's stream; a ray's record depends on that ray alone
    const uint64_t per = rtnw::plan_trace_batch((uint64_t)n, std::getenv("RTNW_RADIANCE_BATCH"));
    if (int rc = s->trace_ws.reserve((size_t)per * (RT_PATH_RAY_BYTES + RT_RADIANCE_BYTES))) return rc;
    char *rays_dev = (char *)s->trace_ws.p, *out_dev = rays_dev + (size_t)per * RT_PATH_RAY_BYTES;
    Events<2> ev;
    HIP_TRY(hipEventCreate(&ev[0]));
    HIP_TRY(hipEventCreate(&ev[1]));
    double total = 0.0;
    for (uint64_t k0 = 0; k0 < (uint64_t)n; k0 += per) {
        const uint64_t m = std::min<uint64_t>(per, (uint64_t)n - k0);
        HIP_TRY(hipMemcpyAsync(rays_dev, rays + k0, (size_t)m * RT_PATH_RAY_BYTES, hipMemcpyHostToDevice, s->own_stream));
        HIP_TRY(hipEventRecord(ev[0], s->own_stream));
        if (int rc = radiance_launch(s, p, rays_dev, (uint32_t)m, out_dev, s->own_stream)) return rc;
        HIP_TRY(hipEventRecord(ev[1], s->own_stream));
        HIP_TRY(hipMemcpyAsync(out + k0, out_dev, (size_t)m * RT_RADIANCE_BYTES, hipMemcpyDeviceToHost, s->own_stream));
        HIP_TRY(hipStreamSynchronize(s->own_stream));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
        total += (double)t;
    }
    if (ms) *ms = total;
    return RT_OK;
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
