// capi_trace.cpp — ray queries on caller-supplied rays (rt_hip.h rt_trace_rays, rt_occluded
// and their _dev forms; rt_trace.hip).
#include "capi_internal.h"
#include "../hip/rt_trace.h"

// the unit's launcher, set by its static initialiser (rt_trace.h)
RtTraceLaunch rt_trace_launch = {nullptr};

static_assert(sizeof(rt_ray) == RT_RAY_BYTES && sizeof(rt_hit) == RT_HIT_BYTES, "rt_ray / rt_hit are three 16-B words");

// The argument checks of the four entry points, the scene's last: all before any HIP call.
// RT_OK with *empty set: n == 0, nothing to do (whatever the other arguments are).
static int trace_check(const char *fn, const rt_scene *s, const void *rays, int64_t n, const void *out, bool *empty) {
    const std::string f(fn);
    RT_TRY(ray_count_check(f, n, empty));
    if (*empty) return RT_OK;
    if (!rays) return fail(RT_ERR_INVALID, f + ": null rays");
    if (!out) return fail(RT_ERR_INVALID, f + ": null output");
    RT_TRY(scene_check(f, s));
    if (!rt_trace_launch.trace) return unit_missing(f, "trace", "rt_trace.o");
    return RT_OK;
}

int trace_launch(const rt_scene *s, const void *rays_dev, uint32_t n, bool any, void *out_dev, hipStream_t stream) {
    RtKernelArgs a{};   // the scene's arrays only (rt_trace.h)
    fill_scene_args(s, a);
    HIP_TRY(rt_trace_launch.trace(&a, rays_dev, n, s->has_moving ? 1 : 0, s->time0, s->time1, any ? 1 : 0, any ? nullptr : out_dev,
                                  any ? (uint8_t *)out_dev : nullptr, stream));
    return RT_OK;
}

// The host forms: batches of rays through the scene's workspace (ray_batches).
static int trace_host(rt_scene *s, const rt_ray *rays, int64_t n, bool any, void *out, double *ms) {
    return ray_batches(s, rays, RT_RAY_BYTES, out, any ? 1 : RT_HIT_BYTES, n, "RTNW_TRACE_BATCH", ms,
                       [&](const void *rays_dev, uint32_t m, void *out_dev, hipStream_t stream) {
                           return trace_launch(s, rays_dev, m, any, out_dev, stream);
                       });
}

extern "C" {

int rt_trace_rays(rt_scene *s, const rt_ray *rays, int64_t n, rt_hit *hits, double *ms) {
    bool empty;
    if (int rc = trace_check("rt_trace_rays", s, rays, n, hits, &empty)) return rc;
    if (empty) return RT_OK;
    return trace_host(s, rays, n, false, hits, ms);
}

int rt_occluded(rt_scene *s, const rt_ray *rays, int64_t n, uint8_t *out, double *ms) {
    bool empty;
    if (int rc = trace_check("rt_occluded", s, rays, n, out, &empty)) return rc;
    if (empty) return RT_OK;
    return trace_host(s, rays, n, true, out, ms);
}

int rt_trace_rays_dev(rt_scene *s, const rt_ray *rays_dev, int64_t n, rt_hit *hits_dev, void *stream) {
    bool empty;
    if (int rc = trace_check("rt_trace_rays_dev", s, rays_dev, n, hits_dev, &empty)) return rc;
    if (empty) return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    return trace_launch(s, rays_dev, (uint32_t)n, false, hits_dev, (hipStream_t)stream);
}

int rt_occluded_dev(rt_scene *s, const rt_ray *rays_dev, int64_t n, uint8_t *out_dev, void *stream) {
    bool empty;
    if (int rc = trace_check("rt_occluded_dev", s, rays_dev, n, out_dev, &empty)) return rc;
    if (empty) return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    return trace_launch(s, rays_dev, (uint32_t)n, true, out_dev, (hipStream_t)stream);
}

}  // extern "C"
