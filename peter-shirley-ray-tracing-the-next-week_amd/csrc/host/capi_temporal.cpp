// capi_temporal.cpp — the reprojected frame history that runs ahead of the denoiser
// (rt_temporal.hip; rt_hip.h): the argument checks, rt_temporal_dev and the host form.
#include <cmath>
#include <cstring>

#include "capi_internal.h"
#include "../hip/rt_features.h"
#include "../hip/rt_temporal.h"

// the unit's launcher, set by its static initialiser (rt_temporal.h)
RtTemporalLaunch rt_temporal_launch = {nullptr};

// All before any HIP call, the parameter named in the message.
static int temporal_check(const char *fn, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                          const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                          const rt_temporal_frame *out) {
    const std::string f(fn);
    if (!cur) return fail(RT_ERR_INVALID, f + ": null argument (cur)");
    if (!cam) return fail(RT_ERR_INVALID, f + ": null argument (cam)");
    if (!tp) return fail(RT_ERR_INVALID, f + ": null argument (tp)");
    if (!out) return fail(RT_ERR_INVALID, f + ": null argument (out)");
    if (!cur->color) return fail(RT_ERR_INVALID, f + ": null argument (cur->color)");
    if (!cur->guides) return fail(RT_ERR_INVALID, f + ": null argument (cur->guides)");
    if (!out->color) return fail(RT_ERR_INVALID, f + ": null argument (out->color)");
    if (!out->len) return fail(RT_ERR_INVALID, f + ": null argument (out->len)");
    if (hist) {
        if (!prev_cam) return fail(RT_ERR_INVALID, f + ": null argument (prev_cam, needed with a history)");
        if (!hist->color) return fail(RT_ERR_INVALID, f + ": null argument (hist->color)");
        if (!hist->guides) return fail(RT_ERR_INVALID, f + ": null argument (hist->guides)");
        if (!hist->len) return fail(RT_ERR_INVALID, f + ": null argument (hist->len)");
    }
    if (nx < 1 || ny < 1 || (uint64_t)nx * (uint64_t)ny > 0x7FFFFFFFull)
        return fail(RT_ERR_INVALID, f + ": nx and ny must be at least 1 (and nx * ny below 2^31)");
    if (tp->max_history < 0 || tp->max_history > (1 << 23))
        return fail(RT_ERR_INVALID, f + ": max_history must be in 0..2^23");
    if (!(tp->cos_normal >= -1.0f && tp->cos_normal <= 1.0f)) return fail(RT_ERR_INVALID, f + ": cos_normal must be in -1..1");
    if (!(tp->sigma_depth >= 0.0f)) return fail(RT_ERR_INVALID, f + ": sigma_depth must not be negative or NaN");
    if (tp->frame_spp < 1 || tp->frame_spp > 65535) return fail(RT_ERR_INVALID, f + ": frame_spp must be in 1..65535");
    if (tp->pad[0] || tp->pad[1] || tp->pad[2] || tp->pad[3]) return fail(RT_ERR_INVALID, f + ": pad must be zero");
    if (hist && (cur->moments != nullptr) != (hist->moments != nullptr))
        return fail(RT_ERR_INVALID, f + ": cur->moments and hist->moments come together or not at all");
    if (out->moments && !cur->moments) return fail(RT_ERR_INVALID, f + ": out->moments needs cur->moments");
    if (out->color == cur->color)
        return fail(RT_ERR_INVALID, f + ": out->color must not be cur->color (not in place)");
    if (hist && out->color == hist->color)
        return fail(RT_ERR_INVALID, f + ": out->color must not be hist->color (neighbours are read: not in place)");
    if (hist && out->moments && out->moments == hist->moments)
        return fail(RT_ERR_INVALID, f + ": out->moments must not be hist->moments (neighbours are read: not in place)");
    if (hist && out->len == hist->len)
        return fail(RT_ERR_INVALID, f + ": out->len must not be hist->len (neighbours are read: not in place)");
    if (!rt_temporal_launch.accumulate)
        return fail(RT_ERR_UNSUPPORTED, f + ": this library was linked without the temporal unit (rt_temporal.o)");
    return RT_OK;
}

// Bytewise equal cameras: a pixel's history is its own pixel (rt_hip.h).
static int temporal_mode(const rt_temporal_frame *hist, const rt_camera_desc *cam, const rt_camera_desc *prev_cam) {
    if (!hist) return RT_TEMPORAL_FIRST;
    return std::memcmp(cam, prev_cam, sizeof(rt_camera_desc)) == 0 ? RT_TEMPORAL_STATIC : RT_TEMPORAL_REPROJECT;
}

extern "C" {

int rt_temporal_dev(int device, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                    const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                    const rt_temporal_frame *out, void *stream) {
    if (int rc = temporal_check("rt_temporal_dev", nx, ny, cur, cam, hist, prev_cam, tp, out)) return rc;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(rt_temporal_launch.accumulate(nx, ny, temporal_mode(hist, cam, prev_cam), cur, cam, hist, prev_cam, tp, out,
                                          (hipStream_t)stream));
    return RT_OK;
}

int rt_temporal(int device, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                const rt_temporal_frame *out, double *ms) {
    if (int rc = temporal_check("rt_temporal", nx, ny, cur, cam, hist, prev_cam, tp, out)) return rc;
    HIP_TRY(hipSetDevice(device));
    const size_t npix = (size_t)nx * ny;
    const bool mom = cur->moments != nullptr, out_mom = out->moments != nullptr;
    // one allocation, in floats (an int32 count takes a float's room); the guides first: 16-B loads
    const size_t g = npix * RT_GUIDE_FLOATS, c = npix * 3, m = npix * 2, l = npix;
    const size_t off_cg = 0, off_hg = off_cg + g, off_cc = off_hg + g, off_hc = off_cc + c, off_oc = off_hc + c,
                 off_cm = off_oc + c, off_hm = off_cm + m, off_om = off_hm + m, off_hl = off_om + m, off_ol = off_hl + l,
                 total = off_ol + l;
    DevBuf staging;
    Events<2> ev;
    if (int rc = staging.reserve(total * sizeof(float))) return rc;
    float *d = (float *)staging.p;
    HIP_TRY(hipMemcpy(d + off_cg, cur->guides, g * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d + off_cc, cur->color, c * sizeof(float), hipMemcpyHostToDevice));
    if (mom) HIP_TRY(hipMemcpy(d + off_cm, cur->moments, m * sizeof(float), hipMemcpyHostToDevice));
    if (hist) {
        HIP_TRY(hipMemcpy(d + off_hg, hist->guides, g * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d + off_hc, hist->color, c * sizeof(float), hipMemcpyHostToDevice));
        if (mom) HIP_TRY(hipMemcpy(d + off_hm, hist->moments, m * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d + off_hl, hist->len, l * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    const rt_temporal_frame dcur = {d + off_cc, d + off_cg, mom ? d + off_cm : nullptr, nullptr};
    const rt_temporal_frame dhist = {d + off_hc, d + off_hg, mom ? d + off_hm : nullptr, (const int32_t *)(d + off_hl)};
    const rt_temporal_frame dout = {d + off_oc, nullptr, out_mom ? d + off_om : nullptr, (const int32_t *)(d + off_ol)};
    HIP_TRY(hipEventCreate(&ev[0]));
    HIP_TRY(hipEventCreate(&ev[1]));
    HIP_TRY(hipEventRecord(ev[0], nullptr));
    HIP_TRY(rt_temporal_launch.accumulate(nx, ny, temporal_mode(hist, cam, prev_cam), &dcur, cam, hist ? &dhist : nullptr,
                                          prev_cam, tp, &dout, nullptr));
    HIP_TRY(hipEventRecord(ev[1], nullptr));
    // the output frame's pointers are written through (rt_hip.h)
    HIP_TRY(hipMemcpy((float *)out->color, d + off_oc, c * sizeof(float), hipMemcpyDeviceToHost));
    if (out_mom) HIP_TRY(hipMemcpy((float *)out->moments, d + off_om, m * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy((int32_t *)out->len, d + off_ol, l * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (ms) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
        *ms = (double)t;
    }
    return RT_OK;
}

}  // extern "C"
