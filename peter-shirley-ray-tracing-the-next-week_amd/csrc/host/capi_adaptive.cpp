// capi_adaptive.cpp — rt_render_adaptive and rt_render_adaptive_guarded: error-driven renders
// over the moments kernels (rt_moments.hip) and the tile renders' job body (capi_render.cpp).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "capi_internal.h"
#include "../hip/rt_moments.h"

// rt_moments.hip's launchers, set by that unit's static initialiser (rt_moments.h)
RtMomentsLaunch rt_moments_launch = {nullptr, nullptr, nullptr, nullptr, nullptr};

// Adaptive sampling (rt_hip.h).  Every pixel of the frame keeps, in device
// buffers in slot order (y * w + x), its running sums, its two moments, its sample count
// and an active flag.  The first pass renders min_spp samples of every pixel; after each
// pass rt_adaptive_select retires the converged pixels, and the next pass is a job of the
// pixels still active — 8 x 8 blocks of the frame in raster order, each block column by
// column, so that a wave's 64 items stay neighbours — which continues their sums and
// moments in place (RT_FLAG_SUM_IN at sample_offset = the samples they have).  Every
// active pixel has the same count, so the cap is the host's to check.  The argument checks
// come before any HIP call.  rt_render_adaptive and rt_render_adaptive_guarded share this
// body: with `guarded`, rt_adaptive_test marks the active pixels that fail their own test and
// rt_adaptive_guard retires an active pixel only if no pixel of its window, clipped to the
// rectangle, is marked.
static int render_adaptive(const char *fn, rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p,
                           const rt_adaptive_params *ap, bool guarded, int guard_radius, int x0, int y0, int w, int h,
                           float *out_rgb, int32_t *out_spp, float *out_moments, rt_adaptive_stats *ast) {
    using rtnw::clock_ms;
    const std::string f(fn);
    if (!cam || !p || !ap || !out_rgb) return fail(RT_ERR_INVALID, f + ": null argument");
    if (ap->min_spp < 2) return fail(RT_ERR_INVALID, f + ": min_spp must be at least 2 (a variance needs two samples)");
    if (ap->step_spp < 1) return fail(RT_ERR_INVALID, f + ": step_spp must be at least 1");
    if (p->spp < ap->min_spp) return fail(RT_ERR_INVALID, f + ": spp (the cap) is below min_spp");
    if (!(ap->floor >= 0.0f) || !std::isfinite(ap->floor))
        return fail(RT_ERR_INVALID, f + ": floor must be finite and not negative");
    if (std::isnan(ap->tolerance)) return fail(RT_ERR_INVALID, f + ": tolerance is NaN");
    if (p->sample_offset != 0) return fail(RT_ERR_INVALID, f + ": sample_offset must be 0");
    if (p->flags & (RT_FLAG_COUNT | RT_FLAG_PROFILE | RT_FLAG_SUM_IN | RT_FLAG_SUM_OUT))
        return fail(RT_ERR_INVALID, f + ": RT_FLAG_COUNT, RT_FLAG_PROFILE, RT_FLAG_SUM_IN and RT_FLAG_SUM_OUT are not supported");
    if (w <= 0 || h <= 0 || (uint64_t)w * (uint64_t)h > 0x7FFFFFFFull) return fail(RT_ERR_INVALID, f + ": empty or oversized frame");
    if (p->nx > 65535 || p->ny > 65535) return fail(RT_ERR_INVALID, f + ": nx and ny must be in 1..65535");
    if (guarded && (guard_radius < 0 || guard_radius > 8)) return fail(RT_ERR_INVALID, f + ": guard_radius must be in 0..8");
    if (!s) return fail(RT_ERR_INVALID, f + ": null scene");
    if (!rt_moments_launch.resolve)
        return fail(RT_ERR_UNSUPPORTED, f + ": this library was linked without the moments unit (rt_moments.o)");

    HIP_TRY(hipSetDevice(s->device));
    if (int rc = ensure_own_stream(s)) return rc;
    hipStream_t stream = s->own_stream;
    const uint32_t npix = (uint32_t)w * (uint32_t)h;
    // RTNW_TRACE: where the call's host time went, on stderr (diagnostics)
    const bool trace_on = std::getenv("RTNW_TRACE") != nullptr;
    const double t_begin = clock_ms();
    double t_first = 0, t_jobs = 0, t_lists = 0, t_select = 0;
    // one allocation, kept with the scene: sums (3 floats), moments (2 floats), counts (int32),
    // the select's two counters (in 16 B), active flags (1 byte) per pixel and, for the guard,
    // fail flags (1 byte)
    const size_t off_mom = (size_t)npix * 12, off_spp = off_mom + (size_t)npix * 8, off_cnt = off_spp + (size_t)npix * 4,
                 off_act = off_cnt + 16, off_fail = off_act + npix, total = off_fail + (guarded ? npix : 0);
    if (int rc = s->frame.reserve(total)) return rc;
    // pinned host memory, kept as well: the select's counters (16 B), a pass's pixel list and
    // its slots (uint32 per pixel each, and one entry of slack), the active flags.  Copies to
    // and from it are true stream copies; with per-pass pageable vectors instead, the first
    // HIP allocation of the call after a render of many large passes took 14-30 ms.
    if (int rc = s->pin.reserve(16 + ((size_t)npix + 1) * 8 + npix)) return rc;
    uint32_t *c = (uint32_t *)s->pin.p, *xy = c + 4, *slot = xy + npix + 1;
    uint8_t *flags = (uint8_t *)(slot + npix + 1);
    uint8_t *base = (uint8_t *)s->frame.p;
    float *sums = (float *)base, *mom = (float *)(base + off_mom);
    int32_t *spp = (int32_t *)(base + off_spp);
    uint32_t *counters = (uint32_t *)(base + off_cnt);
    uint8_t *active = base + off_act, *failing = base + off_fail;
    HIP_TRY(hipMemsetAsync(spp, 0, (size_t)npix * 4, stream));
    HIP_TRY(hipMemsetAsync(active, 1, npix, stream));

    rt_render_params q = *p;
    q.chunk = 1;
    q.flags = (p->flags & RT_FLAG_RIGHT_FOLD) | RT_FLAG_SUM_OUT;
    q.spp = ap->min_spp;
    q.sample_offset = 0;
    rt_adaptive_stats st{};
    rt_stats rs;
    const int32_t tile[4] = {x0, y0, w, h};
    if (int rc = render_job(s, cam, &q, tile, 1, nullptr, sums, mom, stream, &rs)) return rc;
    t_first = clock_ms() - t_begin;
    st.kernel_ms += rs.kernel_ms;
    st.resolve_ms += rs.resolve_ms;

    const int cap = p->spp;
    int done = ap->min_spp, added = ap->min_spp;
    uint32_t nactive = npix;
    rtnw::ActiveJobState order;   // the deep map (deep pixels go first, as in a tile job) and the sweep's scratch lists
    const bool deep_front = deep_first(s);
    for (;;) {
        st.passes += 1;
        st.samples += (double)nactive * (double)added;
        double t0 = clock_ms();
        HIP_TRY(hipMemsetAsync(counters, 0, 2 * sizeof(uint32_t), stream));
        HIP_TRY(hipEventRecord(s->ev[0], stream));
        if (guarded) {   // the own-pixel test for everyone, then the windows
            HIP_TRY(rt_moments_launch.test(npix, added, ap->tolerance, ap->floor, mom, spp, active, failing, stream));
            HIP_TRY(rt_moments_launch.guard(w, h, guard_radius, failing, active, counters, stream));
        } else {
            HIP_TRY(rt_moments_launch.select(npix, added, ap->tolerance, ap->floor, mom, spp, active, counters, stream));
        }
        HIP_TRY(hipEventRecord(s->ev[1], stream));
        HIP_TRY(hipMemcpyAsync(c, counters, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        const bool more = done < cap;
        if (more) HIP_TRY(hipMemcpyAsync(flags, active, npix, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
        st.select_ms += ms;
        st.pixels_converged += (double)c[1];
        nactive = c[0];
        t_select += clock_ms() - t0;
        if (!more || nactive == 0) break;
        t0 = clock_ms();
        if (deep_front && order.deep.empty()) rtnw::fill_deep_map(*s, cam, x0, y0, w, h, p->nx, p->ny, &order.deep);
        uint32_t ndeep = 0;
        if (int rc = rtnw::active_job_order(f, flags, x0, y0, w, h, nactive, &order, xy, slot, &ndeep)) return rc;
        added = std::min(ap->step_spp, cap - done);
        q.spp = added;
        q.sample_offset = (uint32_t)done;
        q.flags |= RT_FLAG_SUM_IN;
        const JobSlots js{xy, slot, nactive, ndeep};
        t_lists += clock_ms() - t0;
        t0 = clock_ms();
        if (int rc = render_job(s, cam, &q, nullptr, 0, &js, sums, mom, stream, &rs)) return rc;
        t_jobs += clock_ms() - t0;
        st.kernel_ms += rs.kernel_ms;
        st.resolve_ms += rs.resolve_ms;
        done += added;
    }
    st.pixels_capped = (double)nactive;   // still active at the cap
    if (out_moments) HIP_TRY(hipMemcpyAsync(out_moments, mom, (size_t)npix * 8, hipMemcpyDeviceToHost, stream));
    if (out_spp) HIP_TRY(hipMemcpyAsync(out_spp, spp, (size_t)npix * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(rt_moments_launch.finish(npix, spp, sums, stream));
    HIP_TRY(hipMemcpyAsync(out_rgb, sums, (size_t)npix * 12, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (trace_on)
        std::fprintf(stderr,
                     "%s: %.0f passes, %.3f ms: first pass %.3f, later passes %.3f, their pixel lists %.3f, "
                     "selects and flag copies %.3f; kernels %.3f, resolves %.3f, select kernels %.3f\n",
                     fn, st.passes, clock_ms() - t_begin, t_first, t_jobs, t_lists, t_select, st.kernel_ms, st.resolve_ms,
                     st.select_ms);
    if (ast) *ast = st;
    return RT_OK;
}

extern "C" {

int rt_render_adaptive(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p, const rt_adaptive_params *ap,
                       int x0, int y0, int w, int h, float *out_rgb, int32_t *out_spp, float *out_moments,
                       rt_adaptive_stats *ast) {
    return render_adaptive("rt_render_adaptive", s, cam, p, ap, false, 0, x0, y0, w, h, out_rgb, out_spp, out_moments, ast);
}

int rt_render_adaptive_guarded(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p,
                               const rt_adaptive_params *ap, int guard_radius, int x0, int y0, int w, int h,
                               float *out_rgb, int32_t *out_spp, float *out_moments, rt_adaptive_stats *ast) {
    return render_adaptive("rt_render_adaptive_guarded", s, cam, p, ap, true, guard_radius, x0, y0, w, h, out_rgb, out_spp,
                           out_moments, ast);
}

}  // extern "C"
