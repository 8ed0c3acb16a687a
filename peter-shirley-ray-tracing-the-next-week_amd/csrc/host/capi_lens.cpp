// capi_lens.cpp — lens renders (rt_hip.h rt_lens_rays, rt_render_lens and their _dev forms;
// rt_lens.hip): the argument checks, the batches (job_plan.cpp plan_lens) and,
// per batch, generate -> radiance query (-> ray query for the guides) -> in-order resolve.
#include <cmath>

#include "capi_internal.h"
#include "../hip/rt_lens.h"
#include "../hip/rt_trace.h"

// the unit's launchers, set by its static initialiser (rt_lens.h)
RtLensLaunch rt_lens_launch = {nullptr, nullptr};

#define RT_PATH_RAY_BYTES 48
#define RT_RADIANCE_BYTES 16
static_assert(sizeof(rt_lens_params) == 32, "rt_lens_params is 32 bytes");
static_assert(sizeof(rt_path_ray) == RT_PATH_RAY_BYTES && sizeof(rt_ray) == RT_RAY_BYTES && sizeof(rt_hit) == RT_HIT_BYTES &&
                  sizeof(rt_radiance) == RT_RADIANCE_BYTES,
              "the records are three 16-B words, rt_radiance one");

// The argument checks that need no scene, in rt_hip.h's order: all before any HIP call.
static int lens_check(const std::string &f, const rt_camera_desc *cam, const rt_lens_params *lens, const rt_render_params *p,
                      int x0, int y0, int w, int h, bool have_out) {
    if (!cam) return fail(RT_ERR_INVALID, f + ": null camera");
    if (!lens) return fail(RT_ERR_INVALID, f + ": null lens");
    if (!p) return fail(RT_ERR_INVALID, f + ": null parameters");
    if (!have_out) return fail(RT_ERR_INVALID, f + ": null output");
    if (lens->model < RT_LENS_PERSPECTIVE || lens->model > RT_LENS_EQUIRECT)
        return fail(RT_ERR_INVALID, f + ": lens model outside RT_LENS_*");
    for (int k = 0; k < 6; k++)
        if (lens->pad[k] != 0) return fail(RT_ERR_INVALID, f + ": lens pad must be zero");
    if (lens->model == RT_LENS_FISHEYE && !(lens->fov_deg > 0.0f && lens->fov_deg <= 360.0f))
        return fail(RT_ERR_INVALID, f + ": fov_deg must be in (0, 360] (and not NaN)");
    if (p->nx < 1 || p->ny < 1 || p->nx > 65535 || p->ny > 65535) return fail(RT_ERR_INVALID, f + ": nx and ny must be in 1..65535");
    if (p->spp < 1) return fail(RT_ERR_INVALID, f + ": spp must be at least 1");
    if (!rtnw::sample_range_ok(p->sample_offset, p->spp))
        return fail(RT_ERR_INVALID, f + ": sample_offset + spp must not pass 0xFFFFFFFF (32-bit sample indices)");
    if (w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || x0 > p->nx - w || y0 > p->ny - h)
        return fail(RT_ERR_INVALID, f + ": rectangle (x0, y0, w, h) empty or outside the image");
    if (p->flags != 0) return fail(RT_ERR_INVALID, f + ": no flag applies (there are no sum, right-fold, counting or profiling forms)");
    if (p->max_depth < 0) return fail(RT_ERR_INVALID, f + ": max_depth < 0");
    if (!std::isfinite(p->t_min)) return fail(RT_ERR_INVALID, f + ": t_min is not finite");
    if (p->background != RT_BG_BLACK && p->background != RT_BG_SKY) return fail(RT_ERR_INVALID, f + ": background outside RT_BG_*");
    return RT_OK;
}

// ... and those of the renders, the scene's last
static int lens_render_check(const char *fn, const rt_scene *s, const rt_camera_desc *cam, const rt_lens_params *lens,
                             const rt_render_params *p, int x0, int y0, int w, int h, const void *out_rgb, bool guides) {
    const std::string f(fn);
    RT_TRY(lens_check(f, cam, lens, p, x0, y0, w, h, out_rgb != nullptr));
    RT_TRY(scene_check(f, s));
    if (!rt_lens_launch.generate) return unit_missing(f, "lens", "rt_lens.o");
    if (!rt_rays_launch.launch) return unit_missing(f, "rays", "rt_kernel_rays.o");
    if (guides && !rt_trace_launch.trace) return unit_missing(f, "trace", "rt_trace.o");
    if (s->has_moving && (cam->time0 < s->time0 || cam->time1 > s->time1))
        return fail(RT_ERR_INVALID, f + ": camera shutter outside the scene's time span (moving-sphere bounds)");
    return RT_OK;
}

static int lens_rays_check(const char *fn, const rt_camera_desc *cam, const rt_lens_params *lens, const rt_render_params *p,
                           int x0, int y0, int w, int h, const void *rays) {
    const std::string f(fn);
    RT_TRY(lens_check(f, cam, lens, p, x0, y0, w, h, rays != nullptr));
    if (!rt_lens_launch.generate) return unit_missing(f, "lens", "rt_lens.o");
    return RT_OK;
}

namespace {

// What the generator reads: the camera and image part of RtKernelArgs, and rt_lens.h's own.
struct LensJob {
    RtKernelArgs a{};
    RtLensArgs l{};
    int x0, y0, w;
    uint64_t npix;
    uint32_t sample_offset;
    LensJob(const rt_camera_desc *cam, const rt_lens_params *lens, const rt_render_params *p, int x0_, int y0_, int w_, int h_)
        : x0(x0_), y0(y0_), w(w_), npix((uint64_t)w_ * (uint64_t)h_), sample_offset(p->sample_offset) {
        fill_camera_args(cam, p, a);
        l.model = lens->model;
        for (int k = 0; k < 3; k++) l.cw[k] = cam->w[k];
        l.fov_k = lens->fov_deg * (float)(M_PI / 360.0);   // one float32 product (tests/test_lens_spec.py)
    }
    // batch b's records: sample planes `stride` records apart, from rays (and trace_rays, when non-null)
    int generate(const rtnw::LensBatch &b, uint64_t stride, void *rays, void *trace_rays, hipStream_t stream) {
        a.sample_offset = sample_offset + (uint32_t)b.s0;
        HIP_TRY(rt_lens_launch.generate(&a, &l, x0, y0, w, (uint32_t)b.p0, (uint32_t)b.np, (int)b.ns, stride, rays, trace_rays,
                                        stream));
        return RT_OK;
    }
};

// The generator into the caller's device buffers: record (sample, pixel) at sample * npix + pixel.
int lens_rays_run(LensJob &job, int spp, char *rays_dev, char *trace_dev, hipStream_t stream) {
    const rtnw::LensPlan pl = rtnw::plan_lens(job.npix, (uint64_t)spp, 0x7FFFFFFFull);   // one launch below 2^31 lanes
    for (uint64_t b = 0; b < pl.nbatches; b++) {
        const rtnw::LensBatch l = rtnw::lens_batch(pl, b, job.npix, (uint64_t)spp);
        const size_t at = (size_t)(l.s0 * job.npix + l.p0);
        RT_TRY(job.generate(l, job.npix, rays_dev + at * RT_PATH_RAY_BYTES, trace_dev ? trace_dev + at * RT_RAY_BYTES : nullptr,
                            stream));
    }
    return RT_OK;
}

// The render into device buffers.  times (null in the _dev form): the batches' summed event
// times, each batch waited for.
int lens_render_run(rt_scene *s, const rt_camera_desc *cam, const rt_lens_params *lens, const rt_render_params *p, int x0, int y0,
                    int w, int h, float *rgb, float *mom, float *guides, hipStream_t stream, double *ms) {
    LensJob job(cam, lens, p, x0, y0, w, h);
    const rtnw::LensPlan pl = rtnw::plan_lens(job.npix, (uint64_t)p->spp, rtnw::lens_batch_limit(std::getenv("RTNW_LENS_BATCH")));
    const size_t per = (size_t)pl.rays_per;
    RT_TRY(s->lens_ws.reserve(per * (RT_PATH_RAY_BYTES + RT_RADIANCE_BYTES + (guides ? RT_RAY_BYTES + RT_HIT_BYTES : 0))));
    char *rays = (char *)s->lens_ws.p, *rad = rays + per * RT_PATH_RAY_BYTES;
    char *trays = guides ? rad + per * RT_RADIANCE_BYTES : nullptr, *hits = guides ? trays + per * RT_RAY_BYTES : nullptr;
    const float k = (float)(1.0 / (double)(float)p->spp);   // vec3.h:134-141, as rt_resolve
    Events<2> ev;
    if (ms) {
        HIP_TRY(hipEventCreate(&ev[0]));
        HIP_TRY(hipEventCreate(&ev[1]));
        *ms = 0.0;
    }
    for (uint64_t b = 0; b < pl.nbatches; b++) {
        const rtnw::LensBatch l = rtnw::lens_batch(pl, b, job.npix, (uint64_t)p->spp);
        const uint32_t n = (uint32_t)(l.np * l.ns);
        if (ms) HIP_TRY(hipEventRecord(ev[0], stream));
        RT_TRY(job.generate(l, l.np, rays, trays, stream));
        RT_TRY(radiance_launch(s, p, rays, n, rad, stream));
        if (guides) RT_TRY(trace_launch(s, trays, n, false, hits, stream));
        HIP_TRY(rt_lens_launch.resolve(rad, hits, (uint32_t)l.np, (int)l.ns, k, l.s0 == 0, l.s0 + l.ns == (uint64_t)p->spp,
                                       rgb + 3 * l.p0, mom ? mom + 2 * l.p0 : nullptr, guides ? guides + 8 * l.p0 : nullptr,
                                       stream));
        if (ms) {
            HIP_TRY(hipEventRecord(ev[1], stream));
            HIP_TRY(hipEventSynchronize(ev[1]));
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
            *ms += (double)t;
        }
    }
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_lens_rays_dev(int device, const rt_camera_desc *cam, const rt_lens_params *lens, const rt_render_params *p, int x0, int y0,
                     int w, int h, rt_path_ray *rays_dev, rt_ray *trace_rays_dev, void *stream) {
    RT_TRY(lens_rays_check("rt_lens_rays_dev", cam, lens, p, x0, y0, w, h, rays_dev));
    HIP_TRY(hipSetDevice(device));
    LensJob job(cam, lens, p, x0, y0, w, h);
    return lens_rays_run(job, p->spp, (char *)rays_dev, (char *)trace_rays_dev, (hipStream_t)stream);
}

int rt_lens_rays(int device, const rt_camera_desc *cam, const rt_lens_params *lens, const rt_render_params *p, int x0, int y0,
                 int w, int h, rt_path_ray *rays, rt_ray *trace_rays) {
    RT_TRY(lens_rays_check("rt_lens_rays", cam, lens, p, x0, y0, w, h, rays));
    HIP_TRY(hipSetDevice(device));
    LensJob job(cam, lens, p, x0, y0, w, h);
    // a batch of records (and of trace rays) in a buffer that lives for the call; synchronous copies
    const rtnw::LensPlan pl = rtnw::plan_lens(job.npix, (uint64_t)p->spp, rtnw::lens_batch_limit(std::getenv("RTNW_LENS_BATCH")));
    const size_t per = (size_t)pl.rays_per;
    DevBuf buf;
    RT_TRY(buf.reserve(per * (RT_PATH_RAY_BYTES + (trace_rays ? RT_RAY_BYTES : 0))));
    char *rays_dev = (char *)buf.p, *trace_dev = trace_rays ? rays_dev + per * RT_PATH_RAY_BYTES : nullptr;
    for (uint64_t b = 0; b < pl.nbatches; b++) {
        const rtnw::LensBatch l = rtnw::lens_batch(pl, b, job.npix, (uint64_t)p->spp);
        RT_TRY(job.generate(l, l.np, rays_dev, trace_dev, nullptr));
        for (uint64_t c = 0; c < l.ns; c++) {   // plane c of the batch to its place in the call's order
            const size_t to = (size_t)((l.s0 + c) * job.npix + l.p0), from = (size_t)(c * l.np);
            HIP_TRY(hipMemcpy((char *)rays + to * RT_PATH_RAY_BYTES, rays_dev + from * RT_PATH_RAY_BYTES,
                              (size_t)l.np * RT_PATH_RAY_BYTES, hipMemcpyDeviceToHost));
            if (trace_rays)
                HIP_TRY(hipMemcpy((char *)trace_rays + to * RT_RAY_BYTES, trace_dev + from * RT_RAY_BYTES,
                                  (size_t)l.np * RT_RAY_BYTES, hipMemcpyDeviceToHost));
        }
    }
    return RT_OK;
}

int rt_render_lens_dev(rt_scene *s, const rt_camera_desc *cam, const rt_lens_params *lens, const rt_render_params *p, int x0,
                       int y0, int w, int h, float *out_rgb_dev, float *out_moments_dev, float *out_guides_dev, void *stream) {
    RT_TRY(lens_render_check("rt_render_lens_dev", s, cam, lens, p, x0, y0, w, h, out_rgb_dev, out_guides_dev != nullptr));
    HIP_TRY(hipSetDevice(s->device));
    return lens_render_run(s, cam, lens, p, x0, y0, w, h, out_rgb_dev, out_moments_dev, out_guides_dev, (hipStream_t)stream,
                           nullptr);
}

int rt_render_lens(rt_scene *s, const rt_camera_desc *cam, const rt_lens_params *lens, const rt_render_params *p, int x0, int y0,
                   int w, int h, float *out_rgb, float *out_moments, float *out_guides, double *ms) {
    RT_TRY(lens_render_check("rt_render_lens", s, cam, lens, p, x0, y0, w, h, out_rgb, out_guides != nullptr));
    HIP_TRY(hipSetDevice(s->device));
    RT_TRY(ensure_own_stream(s));
    const size_t npix = (size_t)w * h;
    Staging st;   // guides first (16-B loads and stores), then colour and moments
    const auto r_g = st.floats(out_guides ? npix * 8 : 0), r_c = st.floats(npix * 3), r_m = st.floats(out_moments ? npix * 2 : 0);
    RT_TRY(st.reserve());
    double total = 0.0;
    RT_TRY(lens_render_run(s, cam, lens, p, x0, y0, w, h, st.ptr(r_c), st.ptr_if(out_moments, r_m), st.ptr_if(out_guides, r_g),
                           s->own_stream, &total));
    HIP_TRY(hipStreamSynchronize(s->own_stream));
    RT_TRY(st.download(out_rgb, r_c));
    RT_TRY(st.download(out_moments, r_m));
    RT_TRY(st.download(out_guides, r_g));
    if (ms) *ms = total;
    return RT_OK;
}

}  // extern "C"
