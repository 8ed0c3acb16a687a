// capi_post.cpp — what runs beside a render: the first-hit feature buffers (rt_features.hip),
// the à-trous denoiser (rt_denoise.hip) and the firefly clamp ahead of it (rt_firefly.hip).
#include <cmath>
#include <map>
#include <mutex>

#include "capi_internal.h"
#include "../hip/rt_features.h"
#include "../hip/rt_denoise.h"
#include "../hip/rt_firefly.h"

// the units' launchers, set by their static initialisers (rt_features.h, rt_denoise.h, rt_firefly.h)
RtFeaturesLaunch rt_features_launch = {nullptr, nullptr};
RtDenoiseLaunch rt_denoise_launch = {nullptr, nullptr};
RtFireflyLaunch rt_firefly_launch = {nullptr};

// ------------------------------------------------ first-hit features (rt_hip.h)
// The argument checks of both entry points, the scene's last: all before any HIP call.
static int features_check(const char *fn, const rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p, int x0,
                          int y0, int w, int h, bool have_out) {
    const std::string f(fn);
    if (!cam || !p) return fail(RT_ERR_INVALID, f + ": null argument (cam or params)");
    if (!have_out) return fail(RT_ERR_INVALID, f + ": null output (at least one feature buffer is needed)");
    if (p->nx < 1 || p->ny < 1 || p->nx > 65535 || p->ny > 65535)
        return fail(RT_ERR_INVALID, f + ": nx and ny must be in 1..65535");
    if (p->spp < 1) return fail(RT_ERR_INVALID, f + ": spp must be at least 1");
    if (!rtnw::sample_range_ok(p->sample_offset, p->spp))
        return fail(RT_ERR_INVALID, f + ": sample_offset + spp must not pass 0xFFFFFFFF (32-bit sample indices)");
    if (p->flags & (RT_FLAG_COUNT | RT_FLAG_PROFILE | RT_FLAG_SUM_IN | RT_FLAG_SUM_OUT))
        return fail(RT_ERR_INVALID, f + ": RT_FLAG_COUNT, RT_FLAG_PROFILE, RT_FLAG_SUM_IN and RT_FLAG_SUM_OUT are not supported");
    if (w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || x0 > p->nx - w || y0 > p->ny - h)
        return fail(RT_ERR_INVALID, f + ": rectangle (x0, y0, w, h) empty or outside the image");
    RT_TRY(scene_check(f, s));
    if (!rt_features_launch.sample) return unit_missing(f, "features", "rt_features.o");
    if (s->has_moving && (cam->time0 < s->time0 || cam->time1 > s->time1))
        return fail(RT_ERR_INVALID, f + ": camera shutter outside the scene's time span (moving-sphere bounds)");
    return RT_OK;
}

// Slab bytes of one feature launch: the samples of a job run in batches of whole samples
// that fit it, each batch added to the running sums in guides_dev in sample order.
#define RT_FEATURE_SLAB_BYTES (256ull << 20)

static int features_run(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p, int x0, int y0, int w, int h,
                        float *guides_dev, hipStream_t stream) {
    const uint32_t npix = (uint32_t)w * (uint32_t)h;   // <= 65535^2
    const uint64_t sample_bytes = (uint64_t)npix * RT_GUIDE_FLOATS * sizeof(float);
    uint64_t per = 0;
    if (int rc = rtnw::plan_feature_batches(npix, p->spp, RT_GUIDE_FLOATS * sizeof(float), RT_FEATURE_SLAB_BYTES, &per)) return rc;
    if (int rc = s->slab.reserve((size_t)(sample_bytes * per))) return rc;
    // the pass reads the scene's arrays and the camera (rt_features.hip), none of the
    // megakernel's launch knobs
    RtKernelArgs a{};
    fill_scene_args(s, a);
    fill_camera_args(cam, p, a);
    a.npix = npix;
    const float k = (float)(1.0 / (double)(float)p->spp);   // vec3.h:134-141, as rt_resolve
    for (uint64_t s0 = 0; s0 < (uint64_t)p->spp; s0 += per) {
        const uint64_t s1 = std::min<uint64_t>(s0 + per, (uint64_t)p->spp);
        a.ns = (int)(s1 - s0);
        a.sample_offset = p->sample_offset + (uint32_t)s0;
        HIP_TRY(rt_features_launch.sample(&a, x0, y0, w, (float *)s->slab.p, stream));
        HIP_TRY(rt_features_launch.resolve((const float *)s->slab.p, npix, a.ns, k, s0 == 0, s1 == (uint64_t)p->spp,
                                           guides_dev, stream));
    }
    return RT_OK;
}

// ------------------------------------------------ denoiser (rt_hip.h)
static int denoise_check(const char *fn, int nx, int ny, bool nulls, const rt_denoise_params *dp, bool moments, bool spp) {
    const std::string f(fn);
    if (nulls || !dp) return fail(RT_ERR_INVALID, f + ": null argument");
    RT_TRY(image_size_check(f, nx, ny));
    if (dp->iterations < 0 || dp->iterations > 8) return fail(RT_ERR_INVALID, f + ": iterations must be in 0..8");
    if (!(dp->sigma_color >= 0.0f)) return fail(RT_ERR_INVALID, f + ": sigma_color must not be negative or NaN");
    if (!(dp->sigma_depth >= 0.0f)) return fail(RT_ERR_INVALID, f + ": sigma_depth must not be negative or NaN");
    if (moments && !spp && dp->uniform_spp < 1)
        return fail(RT_ERR_INVALID, f + ": uniform_spp must be at least 1 when moments come without an spp map");
    if (dp->variance_filter != 0 && dp->variance_filter != 1)
        return fail(RT_ERR_INVALID, f + ": variance_filter must be 0 or 1");
    if (!rt_denoise_launch.prepare) return unit_missing(f, "denoise", "rt_denoise.o");
    return RT_OK;
}

// The filter's planes (G, E ping, E pong: 48 B per pixel), one buffer per device, grown on
// demand.  A call holds g_dn_mu from the lookup until its last launch is enqueued: a concurrent
// call that must grow the buffer then frees it only after that, and hipFree waits for the
// device, so no enqueued launch reads freed memory.  The map lives as long as the process and
// is leaked on purpose: destroying it would call hipFree during static destruction, after the
// HIP runtime may have shut down.
namespace {
std::mutex g_dn_mu;
std::map<int, DevBuf> &denoise_workspaces() {
    static auto *ws = new std::map<int, DevBuf>;
    return *ws;
}
}

static int denoise_run(int device, int nx, int ny, const float *color, const float *guides, const float *moments,
                       const int32_t *spp, const rt_denoise_params *dp, float *out, hipStream_t stream) {
    const size_t npix = (size_t)nx * ny;
    if (dp->iterations == 0) {   // the input, as it is
        HIP_TRY(hipMemcpyAsync(out, color, npix * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream));
        return RT_OK;
    }
    std::lock_guard<std::mutex> lock(g_dn_mu);
    DevBuf &ws = denoise_workspaces()[device];
    if (int rc = ws.reserve(npix * 48)) return rc;
    float4 *planes = (float4 *)ws.p;
    float4 *G = planes, *E[2] = {planes + npix, planes + 2 * npix};
    HIP_TRY(rt_denoise_launch.prepare((uint32_t)npix, color, guides, moments, spp, dp->uniform_spp, dp->demodulate != 0, G,
                                      E[0], stream));
    for (int i = 0; i < dp->iterations; i++) {
        const bool last = i + 1 == dp->iterations;
        HIP_TRY(rt_denoise_launch.atrous(nx, ny, 1 << i, dp->sigma_color, dp->sigma_depth, moments != nullptr,
                                         dp->variance_filter, G, E[i & 1], E[(i + 1) & 1], guides, dp->demodulate != 0,
                                         last ? out : nullptr, stream));
    }
    return RT_OK;
}

// ------------------------------------------------ firefly clamp (rt_hip.h)
// `nulls`: a required pointer is missing; `same`: out is color.  All before any HIP call.
static int firefly_check(const char *fn, int nx, int ny, bool nulls, const rt_firefly_params *fp, bool moments,
                         bool out_moments, bool same) {
    const std::string f(fn);
    if (nulls || !fp) return fail(RT_ERR_INVALID, f + ": null argument");
    RT_TRY(image_size_check(f, nx, ny));
    if (fp->demodulate != 0 && fp->demodulate != 1) return fail(RT_ERR_INVALID, f + ": demodulate must be 0 or 1");
    if (fp->radius < 1 || fp->radius > 3) return fail(RT_ERR_INVALID, f + ": radius must be in 1..3");
    const int window = (2 * fp->radius + 1) * (2 * fp->radius + 1) - 1;
    if (fp->min_similar < 1 || fp->min_similar > window)
        return fail(RT_ERR_INVALID, f + ": min_similar must be in 1..(2 radius + 1)^2 - 1");
    if (!(fp->k >= 1.0f)) return fail(RT_ERR_INVALID, f + ": k must be at least 1 (and not NaN)");
    if (!(fp->floor >= 0.0f) || !std::isfinite(fp->floor))
        return fail(RT_ERR_INVALID, f + ": floor must be finite and not negative");
    if (!(fp->cos_normal >= -1.0f && fp->cos_normal <= 1.0f))
        return fail(RT_ERR_INVALID, f + ": cos_normal must be in -1..1");
    if (!(fp->sigma_depth >= 0.0f)) return fail(RT_ERR_INVALID, f + ": sigma_depth must not be negative or NaN");
    if (!(fp->sigma_albedo >= 0.0f)) return fail(RT_ERR_INVALID, f + ": sigma_albedo must not be negative or NaN");
    if (out_moments && !moments) return fail(RT_ERR_INVALID, f + ": out_moments needs moments");
    if (same) return fail(RT_ERR_INVALID, f + ": out must not be color (neighbours are read: not in place)");
    if (!rt_firefly_launch.clamp) return unit_missing(f, "firefly", "rt_firefly.o");
    return RT_OK;
}

// The packed guides of the host forms (8 floats per pixel: albedo.rgb, coverage, normal.xyz,
// depth) from their planes, and back.  The filter and the clamp do not read the coverage: 0.
static std::vector<float> pack_guides(size_t npix, const float *albedo, const float *normal, const float *depth) {
    std::vector<float> g(npix * RT_GUIDE_FLOATS);
    for (size_t q = 0; q < npix; q++) {
        float *v = g.data() + q * RT_GUIDE_FLOATS;
        v[0] = albedo[3 * q]; v[1] = albedo[3 * q + 1]; v[2] = albedo[3 * q + 2]; v[3] = 0.f;
        v[4] = normal[3 * q]; v[5] = normal[3 * q + 1]; v[6] = normal[3 * q + 2]; v[7] = depth[q];
    }
    return g;
}
static void unpack_guides(const std::vector<float> &g, float *albedo, float *normal, float *depth, float *coverage) {
    for (size_t q = 0; q < g.size() / RT_GUIDE_FLOATS; q++) {   // a null plane is not wanted
        const float *v = g.data() + q * RT_GUIDE_FLOATS;
        if (albedo) { albedo[3 * q] = v[0]; albedo[3 * q + 1] = v[1]; albedo[3 * q + 2] = v[2]; }
        if (coverage) coverage[q] = v[3];
        if (normal) { normal[3 * q] = v[4]; normal[3 * q + 1] = v[5]; normal[3 * q + 2] = v[6]; }
        if (depth) depth[q] = v[7];
    }
}

extern "C" {

int rt_render_features_dev(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p, int x0, int y0, int w, int h,
                           float *guides_dev, void *stream) {
    if (int rc = features_check("rt_render_features_dev", s, cam, p, x0, y0, w, h, guides_dev != nullptr)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    return features_run(s, cam, p, x0, y0, w, h, guides_dev, (hipStream_t)stream);
}

int rt_render_features(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p, int x0, int y0, int w, int h,
                       float *albedo, float *normal, float *depth, float *coverage) {
    RT_TRY(features_check("rt_render_features", s, cam, p, x0, y0, w, h, albedo || normal || depth || coverage));
    HIP_TRY(hipSetDevice(s->device));
    const size_t npix = (size_t)w * h, bytes = npix * RT_GUIDE_FLOATS * sizeof(float);
    if (int rc = s->host_out.reserve(bytes)) return rc;
    if (int rc = ensure_own_stream(s)) return rc;
    if (int rc = features_run(s, cam, p, x0, y0, w, h, (float *)s->host_out.p, s->own_stream)) return rc;
    std::vector<float> g(npix * RT_GUIDE_FLOATS);
    HIP_TRY(hipMemcpyAsync(g.data(), s->host_out.p, bytes, hipMemcpyDeviceToHost, s->own_stream));
    HIP_TRY(hipStreamSynchronize(s->own_stream));
    unpack_guides(g, albedo, normal, depth, coverage);
    return RT_OK;
}

int rt_denoise_dev(int device, int nx, int ny, const float *color_dev, const float *guides_dev, const float *moments_dev,
                   const int32_t *spp_dev, const rt_denoise_params *dp, float *out_dev, void *stream) {
    RT_TRY(denoise_check("rt_denoise_dev", nx, ny, !color_dev || !guides_dev || !out_dev, dp, moments_dev != nullptr,
                         spp_dev != nullptr));
    HIP_TRY(hipSetDevice(device));
    return denoise_run(device, nx, ny, color_dev, guides_dev, moments_dev, spp_dev, dp, out_dev, (hipStream_t)stream);
}

int rt_denoise(int device, int nx, int ny, const float *color, const float *albedo, const float *normal, const float *depth,
               const float *moments, const int32_t *spp, const rt_denoise_params *dp, float *out, double *ms) {
    RT_TRY(denoise_check("rt_denoise", nx, ny, !color || !albedo || !normal || !depth || !out, dp, moments != nullptr,
                         spp != nullptr));
    HIP_TRY(hipSetDevice(device));
    const size_t npix = (size_t)nx * ny;
    const std::vector<float> g = pack_guides(npix, albedo, normal, depth);
    Staging st;   // colour, guides, moments, spp, out
    const auto r_c = st.floats(npix * 3), r_g = st.floats(g.size()), r_m = st.floats(npix * 2), r_s = st.floats(npix),
               r_o = st.floats(npix * 3);
    RT_TRY(st.reserve());
    RT_TRY(st.upload(r_c, color));
    RT_TRY(st.upload(r_g, g.data()));
    RT_TRY(st.upload(r_m, moments));
    RT_TRY(st.upload(r_s, spp));
    RT_TRY(st.begin());
    RT_TRY(denoise_run(device, nx, ny, st.ptr(r_c), st.ptr(r_g), st.ptr_if(moments, r_m), (const int32_t *)st.ptr_if(spp, r_s),
                       dp, st.ptr(r_o), nullptr));
    RT_TRY(st.end());
    RT_TRY(st.download(out, r_o));
    return st.elapsed(ms);
}

int rt_firefly_dev(int device, int nx, int ny, const float *color_dev, const float *guides_dev, const float *moments_dev,
                   const rt_firefly_params *fp, float *out_dev, float *out_moments_dev, float *ratio_dev, void *stream) {
    RT_TRY(firefly_check("rt_firefly_dev", nx, ny, !color_dev || !guides_dev || !out_dev, fp, moments_dev != nullptr,
                         out_moments_dev != nullptr, out_dev == color_dev));
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(rt_firefly_launch.clamp(nx, ny, color_dev, guides_dev, moments_dev, fp, out_dev, out_moments_dev, ratio_dev,
                                    (hipStream_t)stream));
    return RT_OK;
}

int rt_firefly(int device, int nx, int ny, const float *color, const float *albedo, const float *normal, const float *depth,
               const float *moments, const rt_firefly_params *fp, float *out, float *out_moments, float *ratio, double *ms) {
    RT_TRY(firefly_check("rt_firefly", nx, ny, !color || !albedo || !normal || !depth || !out, fp, moments != nullptr,
                         out_moments != nullptr, out == color));
    HIP_TRY(hipSetDevice(device));
    const size_t npix = (size_t)nx * ny;
    const std::vector<float> g = pack_guides(npix, albedo, normal, depth);
    Staging st;   // guides, colour, moments, out, out moments, ratio (the guides first: 16-B loads)
    const auto r_g = st.floats(g.size()), r_c = st.floats(npix * 3), r_m = st.floats(npix * 2), r_o = st.floats(npix * 3),
               r_om = st.floats(npix * 2), r_r = st.floats(npix);
    RT_TRY(st.reserve());
    RT_TRY(st.upload(r_g, g.data()));
    RT_TRY(st.upload(r_c, color));
    RT_TRY(st.upload(r_m, moments));
    RT_TRY(st.begin());
    HIP_TRY(rt_firefly_launch.clamp(nx, ny, st.ptr(r_c), st.ptr(r_g), st.ptr_if(moments, r_m), fp, st.ptr(r_o),
                                    st.ptr_if(out_moments, r_om), st.ptr_if(ratio, r_r), nullptr));
    RT_TRY(st.end());
    RT_TRY(st.download(out, r_o));
    RT_TRY(st.download(out_moments, r_om));
    RT_TRY(st.download(ratio, r_r));
    return st.elapsed(ms);
}

}  // extern "C"
