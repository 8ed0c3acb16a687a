// capi_temporal.cpp — the reprojected frame history that runs ahead of the denoiser
// (rt_temporal.hip; rt_hip.h): the argument checks, rt_temporal_dev and the host
// form, the same two over the clamped launcher (rt_temporal_clamped) and over the one that also
// serves background and edge pixels (rt_temporal_cover).
#include <cmath>
#include <cstring>

#include "capi_internal.h"
#include "../hip/rt_features.h"
#include "../hip/rt_temporal.h"

// the unit's launcher, set by its static initialiser (rt_temporal.h)
RtTemporalLaunch rt_temporal_launch = {nullptr, nullptr, nullptr, nullptr};

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
    RT_TRY(image_size_check(f, nx, ny));
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
    if (!rt_temporal_launch.accumulate) return unit_missing(f, "temporal", "rt_temporal.o");
    return RT_OK;
}

// rt_temporal_clamped's checks: rt_temporal's, then the clamp's own.
static int temporal_clamp_check(const char *fn, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                                const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                                const rt_temporal_clamp_params *cp, const rt_temporal_frame *out, const int32_t *clipped) {
    if (int rc = temporal_check(fn, nx, ny, cur, cam, hist, prev_cam, tp, out)) return rc;
    const std::string f(fn);
    if (!cp) return fail(RT_ERR_INVALID, f + ": null argument (cp)");
    if (cp->radius < 0 || cp->radius > RT_TEMPORAL_CLAMP_MAX_RADIUS) return fail(RT_ERR_INVALID, f + ": radius must be in 0..3");
    if (!(cp->gamma >= 0.0f) || std::isinf(cp->gamma))
        return fail(RT_ERR_INVALID, f + ": gamma must not be negative, NaN or infinite");
    for (int32_t w : cp->pad)
        if (w) return fail(RT_ERR_INVALID, f + ": pad of the clamp's parameters must be zero");
    if (clipped) {   // written while the frames are read and `out` is written: a buffer of its own
        const void *c = clipped;
        const rt_temporal_frame none = {nullptr, nullptr, nullptr, nullptr};
        for (const rt_temporal_frame *fr : {cur, hist ? hist : &none, out})
            if (c == fr->color || c == fr->guides || c == fr->moments || c == fr->len)
                return fail(RT_ERR_INVALID, f + ": clipped must not be one of the frames' arrays");
    }
    if (!rt_temporal_launch.accumulate_clamped) return unit_missing(f, "temporal", "rt_temporal.o");
    return RT_OK;
}

// rt_temporal_cover's checks: rt_temporal_clamped's, then the cover's own.
static int temporal_cover_check(const char *fn, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                                const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                                const rt_temporal_clamp_params *cp, const rt_temporal_cover_params *vp,
                                const rt_temporal_frame *out, const int32_t *clipped, const int32_t *source) {
    if (int rc = temporal_clamp_check(fn, nx, ny, cur, cam, hist, prev_cam, tp, cp, out, clipped)) return rc;
    const std::string f(fn);
    if (!vp) return fail(RT_ERR_INVALID, f + ": null argument (vp)");
    if (vp->background != 0 && vp->background != 1) return fail(RT_ERR_INVALID, f + ": background must be 0 or 1");
    if (vp->edges != 0 && vp->edges != 1) return fail(RT_ERR_INVALID, f + ": edges must be 0 or 1");
    if (!(vp->sigma_coverage >= 0.0f) || std::isinf(vp->sigma_coverage))
        return fail(RT_ERR_INVALID, f + ": sigma_coverage must not be negative, NaN or infinite");
    for (int32_t w : vp->pad)
        if (w) return fail(RT_ERR_INVALID, f + ": pad of the cover's parameters must be zero");
    if (source) {   // written like `clipped`: a buffer of its own
        const void *c = source;
        if (c == clipped) return fail(RT_ERR_INVALID, f + ": source must not be clipped");
        const rt_temporal_frame none = {nullptr, nullptr, nullptr, nullptr};
        for (const rt_temporal_frame *fr : {cur, hist ? hist : &none, out})
            if (c == fr->color || c == fr->guides || c == fr->moments || c == fr->len)
                return fail(RT_ERR_INVALID, f + ": source must not be one of the frames' arrays");
    }
    if (!rt_temporal_launch.accumulate_cover || !rt_temporal_launch.mark_same) return unit_missing(f, "temporal", "rt_temporal.o");
    return RT_OK;
}

// Bytewise equal cameras: a pixel's history is its own pixel (rt_hip.h).
static int temporal_mode(const rt_temporal_frame *hist, const rt_camera_desc *cam, const rt_camera_desc *prev_cam) {
    if (!hist) return RT_TEMPORAL_FIRST;
    return std::memcmp(cam, prev_cam, sizeof(rt_camera_desc)) == 0 ? RT_TEMPORAL_STATIC : RT_TEMPORAL_REPROJECT;
}

// rt_temporal_cover where rt_temporal's kernel runs (a first frame, equal cameras): no channel is
// clipped, and a history comes from the pixel itself or from nowhere.  Device pointers, on `stream`.
static int temporal_cover_fill(int nx, int ny, int mode, const int32_t *hist_len, const rt_temporal_params *tp, int32_t *clipped,
                               int32_t *source, hipStream_t stream) {
    const size_t bytes = (size_t)nx * ny * sizeof(int32_t);
    if (clipped) HIP_TRY(hipMemsetAsync(clipped, 0, bytes, stream));
    if (source && mode == RT_TEMPORAL_FIRST) HIP_TRY(hipMemsetAsync(source, 0, bytes, stream));
    if (source && mode == RT_TEMPORAL_STATIC) HIP_TRY(rt_temporal_launch.mark_same(nx, ny, hist_len, tp->max_history, source, stream));
    return RT_OK;
}

// The host form of the entry points, the checks made: every array staged in one allocation, the
// kernel timed alone.  `cp` null is rt_temporal; with it, `clipped` (or null) is staged back too;
// with `vp` besides it is rt_temporal_cover, and so is `source` (or null).
static int temporal_host(int device, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                         const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                         const rt_temporal_clamp_params *cp, const rt_temporal_cover_params *vp, const rt_temporal_frame *out,
                         int32_t *clipped, int32_t *source, double *ms) {
    HIP_TRY(hipSetDevice(device));
    const size_t npix = (size_t)nx * ny;
    // in floats (an int32 count takes a float's room); the guides first: 16-B loads
    const size_t g = npix * RT_GUIDE_FLOATS, c = npix * 3, m = npix * 2, l = npix;
    Staging st;
    const auto cur_g = st.floats(g), hist_g = st.floats(g), cur_c = st.floats(c), hist_c = st.floats(c), out_c = st.floats(c),
               cur_m = st.floats(m), hist_m = st.floats(m), out_m = st.floats(m), hist_l = st.floats(l), out_l = st.floats(l),
               clip = st.floats(clipped ? l : 0), src = st.floats(source ? l : 0);
    RT_TRY(st.reserve());
    RT_TRY(st.upload(cur_g, cur->guides));
    RT_TRY(st.upload(cur_c, cur->color));
    RT_TRY(st.upload(cur_m, cur->moments));
    if (hist) {
        RT_TRY(st.upload(hist_g, hist->guides));
        RT_TRY(st.upload(hist_c, hist->color));
        RT_TRY(st.upload(hist_m, cur->moments ? hist->moments : nullptr));
        RT_TRY(st.upload(hist_l, hist->len));
    }
    const rt_temporal_frame dcur = {st.ptr(cur_c), st.ptr(cur_g), st.ptr_if(cur->moments, cur_m), nullptr};
    const rt_temporal_frame dhist = {st.ptr(hist_c), st.ptr(hist_g), st.ptr_if(cur->moments, hist_m),
                                     (const int32_t *)st.ptr(hist_l)};
    const rt_temporal_frame dout = {st.ptr(out_c), nullptr, st.ptr_if(out->moments, out_m), (const int32_t *)st.ptr(out_l)};
    const int mode = temporal_mode(hist, cam, prev_cam);
    if (vp && mode != RT_TEMPORAL_REPROJECT)
        RT_TRY(temporal_cover_fill(nx, ny, mode, dhist.len, tp, (int32_t *)st.ptr_if(clipped, clip),
                                   (int32_t *)st.ptr_if(source, src), nullptr));
    else if (!vp && cp && clipped && !rt_temporal_clamps(mode, cp))   // rt_temporal's kernel runs: no channel is clipped
        HIP_TRY(hipMemsetAsync(st.ptr(clip), 0, npix * sizeof(int32_t), nullptr));
    RT_TRY(st.begin());   // the events bracket the kernel alone
    if (vp)
        HIP_TRY(rt_temporal_launch.accumulate_cover(nx, ny, mode, &dcur, cam, hist ? &dhist : nullptr, prev_cam, tp, cp, vp, &dout,
                                                    (int32_t *)st.ptr_if(clipped, clip), (int32_t *)st.ptr_if(source, src),
                                                    nullptr));
    else if (cp)
        HIP_TRY(rt_temporal_launch.accumulate_clamped(nx, ny, mode, &dcur, cam, hist ? &dhist : nullptr, prev_cam, tp, cp, &dout,
                                                      (int32_t *)st.ptr_if(clipped, clip), nullptr));
    else
        HIP_TRY(rt_temporal_launch.accumulate(nx, ny, mode, &dcur, cam, hist ? &dhist : nullptr, prev_cam, tp, &dout, nullptr));
    RT_TRY(st.end());
    // the output frame's pointers are written through (rt_hip.h)
    RT_TRY(st.download((float *)out->color, out_c));
    RT_TRY(st.download((float *)out->moments, out_m));
    RT_TRY(st.download((int32_t *)out->len, out_l));
    RT_TRY(st.download(clipped, clip));
    RT_TRY(st.download(source, src));
    return st.elapsed(ms);
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
    return temporal_host(device, nx, ny, cur, cam, hist, prev_cam, tp, nullptr, nullptr, out, nullptr, nullptr, ms);
}

int rt_temporal_clamped_dev(int device, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                            const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                            const rt_temporal_clamp_params *cp, const rt_temporal_frame *out, int32_t *clipped_dev,
                            void *stream) {
    if (int rc = temporal_clamp_check("rt_temporal_clamped_dev", nx, ny, cur, cam, hist, prev_cam, tp, cp, out, clipped_dev)) return rc;
    HIP_TRY(hipSetDevice(device));
    const int mode = temporal_mode(hist, cam, prev_cam);
    if (clipped_dev && !rt_temporal_clamps(mode, cp))   // rt_temporal's kernel runs: no channel is clipped
        HIP_TRY(hipMemsetAsync(clipped_dev, 0, (size_t)nx * ny * sizeof(int32_t), (hipStream_t)stream));
    HIP_TRY(rt_temporal_launch.accumulate_clamped(nx, ny, mode, cur, cam, hist, prev_cam, tp, cp, out, clipped_dev,
                                                  (hipStream_t)stream));
    return RT_OK;
}

int rt_temporal_clamped(int device, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                        const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                        const rt_temporal_clamp_params *cp, const rt_temporal_frame *out, int32_t *clipped, double *ms) {
    if (int rc = temporal_clamp_check("rt_temporal_clamped", nx, ny, cur, cam, hist, prev_cam, tp, cp, out, clipped)) return rc;
    return temporal_host(device, nx, ny, cur, cam, hist, prev_cam, tp, cp, nullptr, out, clipped, nullptr, ms);
}

int rt_temporal_cover_dev(int device, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                          const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                          const rt_temporal_clamp_params *cp, const rt_temporal_cover_params *vp,
                          const rt_temporal_frame *out, int32_t *clipped_dev, int32_t *source_dev, void *stream) {
    if (int rc = temporal_cover_check("rt_temporal_cover_dev", nx, ny, cur, cam, hist, prev_cam, tp, cp, vp, out, clipped_dev,
                                      source_dev))
        return rc;
    HIP_TRY(hipSetDevice(device));
    const int mode = temporal_mode(hist, cam, prev_cam);
    if (mode != RT_TEMPORAL_REPROJECT)
        RT_TRY(temporal_cover_fill(nx, ny, mode, hist ? hist->len : nullptr, tp, clipped_dev, source_dev, (hipStream_t)stream));
    HIP_TRY(rt_temporal_launch.accumulate_cover(nx, ny, mode, cur, cam, hist, prev_cam, tp, cp, vp, out, clipped_dev, source_dev,
                                                (hipStream_t)stream));
    return RT_OK;
}

int rt_temporal_cover(int device, int nx, int ny, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                      const rt_temporal_frame *hist, const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                      const rt_temporal_clamp_params *cp, const rt_temporal_cover_params *vp, const rt_temporal_frame *out,
                      int32_t *clipped, int32_t *source, double *ms) {
    if (int rc = temporal_cover_check("rt_temporal_cover", nx, ny, cur, cam, hist, prev_cam, tp, cp, vp, out, clipped, source))
        return rc;
    return temporal_host(device, nx, ny, cur, cam, hist, prev_cam, tp, cp, vp, out, clipped, source, ms);
}

}  // extern "C"
