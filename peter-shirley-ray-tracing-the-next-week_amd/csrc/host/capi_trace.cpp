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
    *empty = false;
    if (!rtnw::ray_count_ok(n)) return fail(RT_ERR_INVALID, f + ": n must be in 0..2^31 - 1");
    if (n == 0) {
        *empty = true;
        return RT_OK;
    }
    if (!rays) return fail(RT_ERR_INVALID, f + ": null rays");
    if (!out) return fail(RT_ERR_INVALID, f + ": null output");
    if (!s) return fail(RT_ERR_INVALID, f + ": null scene");
    if (s->bvh_width != 2) return fail(RT_ERR_UNSUPPORTED, f + " needs a scene with a 2-wide BVH (RTNW_BVH_WIDTH=2)");
    if (!rt_trace_launch.trace)
        return fail(RT_ERR_UNSUPPORTED, f + ": this library was linked without the trace unit (rt_trace.o)");
    return RT_OK;
}

static int trace_launch(const rt_scene *s, const void *rays_dev, uint32_t n, bool any, void *out_dev, hipStream_t stream) {
    RtKernelArgs a{};   // the scene's arrays only (rt_trace.h)
    fill_scene_args(s, a);
    HIP_TRY(rt_trace_launch.trace(&a, rays_dev, n, s->has_moving ? 1 : 0, s->time0, s->time1, any ? 1 : 0, any ? nullptr : out_dev,
                                  any ? (uint8_t *)out_dev : nullptr, stream));
    return RT_OK;
}

// The host forms: batches of rays through the scene's workspace (rays, then results), each
// copied in, traced and copied out on the scene's stream.  A ray's result depends on that ray
// alone, so not on the batches.
static int trace_host(rt_scene *s, const rt_ray *rays, int64_t n, bool any, void *out, double *ms) {
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = ensure_own_stream(s)) return rc;
    const size_t out_bytes = any ? 1 : RT_HIT_BYTES;
    const uint64_t per = rtnw::plan_trace_batch((uint64_t)n, std::getenv("RTNW_TRACE_BATCH"));
    if (int rc = s->trace_ws.reserve((size_t)per * (RT_RAY_BYTES + out_bytes))) return rc;
    char *rays_dev = (char *)s->trace_ws.p, *out_dev = rays_dev + (size_t)per * RT_RAY_BYTES;
    Events<2> ev;
    HIP_TRY(hipEventCreate(&ev[0]));
    HIP_TRY(hipEventCreate(&ev[1]));
    double total = 0.0;
    for (uint64_t k0 = 0; k0 < (uint64_t)n; k0 += per) {
        const uint64_t m = std::min<uint64_t>(per, (uint64_t)n - k0);
        HIP_TRY(hipMemcpyAsync(rays_dev, rays + k0, (size_t)m * RT_RAY_BYTES, hipMemcpyHostToDevice, s->own_stream));
        HIP_TRY(hipEventRecord(ev[0], s->own_stream));
        if (int rc = trace_launch(s, rays_dev, (uint32_t)m, any, out_dev, s->own_stream)) return rc;
        HIP_TRY(hipEventRecord(ev[1], s->own_stream));
        HIP_TRY(hipMemcpyAsync((char *)out + (size_t)k0 * out_bytes, out_dev, (size_t)m * out_bytes, hipMemcpyDeviceToHost,
                               s->own_stream));
        HIP_TRY(hipStreamSynchronize(s->own_stream));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
        total += (double)t;
    }
    if (ms) *ms = total;
    return RT_OK;
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
