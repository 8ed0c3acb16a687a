// capi_render.cpp — the tile renders of the C ABI: job setup, launch knobs, the megakernel +
// resolve launches over sample batches, timing and statistics.
#include <cstdio>
#include <cstring>

#include "capi_internal.h"
#include "../hip/rt_moments.h"

namespace {

// SURVEY §8d byte model (bytes the algorithm must read or write, independent of
// this implementation's record padding):
//   node fetch: the bytes loaded per visit (BVH2 64 B, BVH4 112 B, BVH8 224 B, compressed
//   BVH8 96 B); sphere 16 B; moving sphere 36 B;
//   rect 24 B; instance chain entered 32 B; medium record 16 B; material +
//   texture per shade 16 + 16 B; Perlin turbulence 7 octaves x 8 gradient gathers
//   x (12 B gradient + 3 x 4 B permutation) = 1344 B; per work item the 4-B job
//   pixel read and the 16-B partial sum written.  (rt_resolve's own traffic — the
//   partial sums read back, the output index and the 12-B pixel — is not the
//   megakernel's.)
double algorithmic_bytes(const rt_stats &st, double items, int bvh_width) {
    const double node = bvh_width == 4 ? 112.0 : bvh_width == 8 ? 224.0 : bvh_width == RT_BVH_CW8 ? 96.0 : 64.0;
    return node * st.node_visits + 16.0 * st.sphere_tests + 36.0 * st.moving_sphere_tests + 24.0 * st.rect_tests +
           32.0 * st.instanced_tests + 16.0 * st.medium_tests + 32.0 * st.shades + 1344.0 * st.noise_evals +
           20.0 * items;
}

// Waves per LDS workgroup that gather the medium cell's paths (rt_megakernel.h stage 6);
// env RTNW_BALL_WAVES (0: none) for A/B runs.  Their ready batch (RTNW_BALL_BATCH) and the
// busy lanes below which they claim new samples (RTNW_BALL_CLAIM): 56 and 48 against 48 and
// 64, c4 48.87 -> 48.50 ms, the share of 8 25.20 -> 25.05 ms (profiles/r06/knobs3_ab.log).
// With the fused in-ball step below a ball wave serves about three times the segments per cycle
// in its trips, and 2 ball waves measure faster than 3 (c4 46.35 against 46.95 ms, 4: 48.1;
// profiles/r08/sweep.log).
#define RT_BALL_WAVES 2
#define RT_BALL_BATCH 56
#define RT_BALL_CLAIM 48
// The ball waves' fused in-ball step (rt_megakernel.h stage 3): the eligible lanes another trip of
// its loop needs; env RTNW_BALL_FAST (0: off) for A/B runs.  Scenes whose media do not qualify
// (scene_lower.cpp ball_fast_media) run without it whatever the setting.  A trip costs the same
// however few lanes it serves: 40 / 48 / 56 measure alike, 16 and 64 (hardly ever reached)
// slower than the step off (profiles/r08/sweep.log).
#ifndef RT_BALL_FAST
#define RT_BALL_FAST 48
#endif
// The shading stage's rejection sampler (rt_device.h coop_reject_mixed): candidates each
// requesting lane tries by itself before the cooperative rounds (RTNW_COOP_LOCAL, 0: none),
// in waves with at least RTNW_COOP_LOCAL_MIN requesters.  Any setting renders the same image;
// 2 and 33 against none: c4 48.49 -> 47.21 ms, c3 22.47 -> 21.84, c2 7.85 -> 7.57
// (profiles/r07/ab_c4.log, ab_c4_sweep.log for the other settings).
#define RT_COOP_LOCAL 2
#define RT_COOP_LOCAL_MIN 33
int ball_waves() {
    if (const char *e = std::getenv("RTNW_BALL_WAVES")) return std::max(0, std::min(RT_LDS_BLOCK / 64, std::atoi(e)));
    return RT_BALL_WAVES;
}

// Partial-sum slab budget per launch (bytes; env RTNW_SLAB_BUDGET overrides, for tests).
// A job whose slab would be larger runs as several launches over sample batches.
// 16 GiB of the 288 GiB HBM: config 5 on one GPU (1e9 samples, 12 GB) is one launch,
// one launch-end drain; 8 GiB made it two.
#define RT_SLAB_BUDGET (16ull << 30)
uint64_t slab_budget() {
    if (const char *e = std::getenv("RTNW_SLAB_BUDGET")) {
        const unsigned long long v = std::strtoull(e, nullptr, 10);
        if (v > 0) return v;
    }
    return RT_SLAB_BUDGET;
}

// Room for n pixels in both job lists, or neither list.
int reserve_job_lists(rt_scene *s, size_t n) {
    int rc = s->job_xy.reserve(n * sizeof(uint32_t));
    if (rc == RT_OK) rc = s->job_out.reserve(n * sizeof(uint32_t));
    if (rc != RT_OK) {
        s->job_xy.release();
        s->job_out.release();
    }
    return rc;
}

// The tile job's pixel lists (rtnw::tile_job_order), kept on the device until a job with
// another key comes.
int prepare_job(rt_scene *s, const int32_t *tiles, int ntiles, int nx, int ny, const rt_camera_desc *cam) {
    std::vector<int32_t> key(tiles, tiles + 4 * ntiles);
    // the deep-first order depends on the camera: its rays' frame joins the cache key
    const bool deep = deep_first(s);
    key.push_back(nx);
    key.push_back(ny);
    key.push_back(deep ? 1 : 0);
    // the empty-pixel bits depend on the camera too (and on whether it leaves the feature on)
    const bool empty = rtnw::empty_fast_scene_ok(*s, cam);
    key.push_back(empty ? 1 : 0);
    if (deep || empty) {
        const float *cf[4] = {cam->origin, cam->lower_left_corner, cam->horizontal, cam->vertical};
        for (const float *f : cf)
            for (int k = 0; k < 3; k++) { int32_t b; std::memcpy(&b, &f[k], 4); key.push_back(b); }
    }
    if (key == s->job_tiles && s->job_xy.p) return RT_OK;
    std::vector<uint32_t> xy, oi;
    uint32_t ndeep = 0;
    rtnw::DeepTest test;
    if (deep) test = [=](int x, int y) { return rtnw::deep_pixel(*s, cam, x, y, nx, ny); };
    if (int rc = rtnw::tile_job_order(tiles, ntiles, nx, ny, test, &xy, &oi, &ndeep)) return rc;
    // the old lists are freed, not reused: hipFree waits for the device, so a launch of the
    // previous job that still reads them (on a stream of the caller's) ends before the copies below
    s->job_xy.release();
    s->job_out.release();
    s->job_tiles.clear();
    if (int rc = reserve_job_lists(s, xy.size())) return rc;
    HIP_TRY(hipMemcpy(s->job_xy.p, xy.data(), xy.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->job_out.p, oi.data(), oi.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    s->npix = (uint32_t)xy.size();
    s->job_ndeep = ndeep;
    s->job_empty = false;
    s->job_nflagged = 0;
    if (empty) {
        // once per job and camera, outside any timed step (RTNW_TRACE prints its time)
        rtnw::PhaseTrace trace{"rt_render_tiles"};
        std::vector<uint32_t> bits;
        size_t nflagged = 0;
        const bool ok = rtnw::empty_pixel_bits(*s, cam, nx, ny, xy.data(), xy.size(), &bits, &nflagged);
        trace("empty pixels");
        if (ok && nflagged > 0) {   // (none flagged: the kernel runs as without the bits)
            if (int rc = s->empty_bits.reserve(bits.size() * sizeof(uint32_t))) return rc;
            HIP_TRY(hipMemcpy(s->empty_bits.p, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            s->job_empty = true;
            s->job_nflagged = (uint32_t)nflagged;
        }
    }
    s->job_tiles = key;
    return RT_OK;
}

// A job over any subset of a frame with explicit output slots (rt_render_adaptive's later
// passes): job pixel k is image pixel xy[k] (x | y << 16) and reads and writes its sums and
// moments at slot[k] of the caller's full-frame buffers, in place — no gather or scatter
// copies.  The pixels are claimed in the order given; the caller lists the deep ones first
// (ndeep of them: a frame's deep pixels are found once, not per pass).  xy and slot are
// pinned host memory that stays as it is until the job's launches have completed: they are
// copied on the job's stream, over the previous job's lists when those have the room (the
// caller has waited for the launches that read them).  Such a job never answers a later
// tile job's cache lookup: it leaves no key behind.
int prepare_job_slots(rt_scene *s, const JobSlots &js, int nx, int ny, hipStream_t stream) {
    if (js.n == 0 || js.ndeep > js.n || nx > 65535 || ny > 65535) return fail(RT_ERR_INVALID, "empty job or image too large");
    for (uint32_t i = 0; i < js.n; i++)
        if ((int)(js.xy[i] & 0xFFFFu) >= nx || (int)(js.xy[i] >> 16) >= ny) return fail(RT_ERR_INVALID, "job pixel outside the image");
    s->job_tiles.clear();
    s->job_empty = false;
    if (int rc = reserve_job_lists(s, js.n)) return rc;
    HIP_TRY(hipMemcpyAsync(s->job_xy.p, js.xy, (size_t)js.n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(s->job_out.p, js.slot, (size_t)js.n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    s->npix = js.n;
    s->job_ndeep = js.ndeep == js.n ? 0 : js.ndeep;   // all deep: one group
    return RT_OK;
}

// The counters of a RT_FLAG_COUNT or RT_FLAG_PROFILE render, read back into `stats`.
int read_counters(rt_scene *s, bool count, bool prof, double items, rt_stats *stats) {
    if (count) {
        unsigned long long c[RT_CNT_N];
        HIP_TRY(hipMemcpy(c, s->stats, sizeof c, hipMemcpyDeviceToHost));
        stats->samples = (double)c[RT_CNT_SAMPLES];
        stats->segments = (double)c[RT_CNT_SEGMENTS];
        stats->node_visits = (double)c[RT_CNT_NODES];
        stats->sphere_tests = (double)c[RT_CNT_SPHERES];
        stats->moving_sphere_tests = (double)c[RT_CNT_MSPHERES];
        stats->rect_tests = (double)c[RT_CNT_RECTS];
        stats->instanced_tests = (double)c[RT_CNT_INSTANCED];
        stats->medium_tests = (double)c[RT_CNT_MEDIA];
        stats->shades = (double)c[RT_CNT_SHADES];
        stats->noise_evals = (double)c[RT_CNT_NOISE];
        stats->algorithmic_bytes = algorithmic_bytes(*stats, items, s->bvh_width);
        unsigned long long w[5];
        HIP_TRY(hipMemcpy(w, (unsigned long long *)s->stats + RT_STAT_WAVE, sizeof w, hipMemcpyDeviceToHost));
        stats->wave_iterations = (double)w[0];
        stats->wave_node_trips = (double)w[1];
        stats->wave_prim_trips = (double)w[2];
        stats->wave_sphere_draw_trips = (double)w[3];
        stats->lane_sphere_draw_trips = (double)w[4];
        unsigned long long sh[3];
        HIP_TRY(hipMemcpy(sh, (unsigned long long *)s->stats + RT_STAT_SHADE, sizeof sh, hipMemcpyDeviceToHost));
        stats->wave_shade_passes = (double)sh[0];
        stats->wave_shade_kinds = (double)sh[1];
        stats->lane_scatters = (double)sh[2];
        // the ball waves (rt_megakernel.h stage 6): a variant without them leaves the slots 0
        unsigned long long b[RT_BALL_N];
        HIP_TRY(hipMemcpy(b, (unsigned long long *)s->stats + RT_STAT_BALL, sizeof b, hipMemcpyDeviceToHost));
        stats->ball_fused_scatters = (double)b[RT_BALL_FUSED];
        stats->ball_fused_declined = (double)b[RT_BALL_DECLINED];
        unsigned long long ef = 0;
        HIP_TRY(hipMemcpy(&ef, (unsigned long long *)s->stats + RT_STAT_EMPTY, sizeof ef, hipMemcpyDeviceToHost));
        stats->empty_fast_samples = (double)ef;
        if (std::getenv("RTNW_TRACE")) {   // diagnostics only
            std::fprintf(stderr,
                         "rtnw ball waves: iterations %llu, live lanes / iteration %.1f, traversal rounds / iteration %.2f, "
                         "cell-decided segments in ball waves %llu, pushes refused (pool full) %llu (of %.0f segments), pushed in %llu, "
                         "pushed out %llu, taken %llu; fused in-ball step: lanes served %llu, declined %llu\n",
                         b[RT_BALL_ITERS], b[RT_BALL_ITERS] ? (double)b[RT_BALL_LIVE] / b[RT_BALL_ITERS] : 0.0,
                         b[RT_BALL_ITERS] ? (double)b[RT_BALL_ROUNDS] / b[RT_BALL_ITERS] : 0.0, b[RT_BALL_CELL_BALL],
                         b[RT_BALL_DENIED], stats->segments, b[RT_BALL_PUSH_IN], b[RT_BALL_PUSH_OUT], b[RT_BALL_TAKEN],
                         b[RT_BALL_FUSED], b[RT_BALL_DECLINED]);
            unsigned long long r[RT_SAMPLER_N];
            HIP_TRY(hipMemcpy(r, (unsigned long long *)s->stats + RT_STAT_SAMPLER, sizeof r, hipMemcpyDeviceToHost));
            std::fprintf(stderr,
                         "rtnw shading-stage sampler: local trips / iteration %.3f, cooperative rounds / iteration %.3f; "
                         "ball waves: %.3f and %.3f\n",
                         w[0] ? (double)r[RT_SAMPLER_LOCAL] / w[0] : 0.0, w[0] ? (double)r[RT_SAMPLER_ROUNDS] / w[0] : 0.0,
                         b[RT_BALL_ITERS] ? (double)r[RT_SAMPLER_BALL_LOCAL] / b[RT_BALL_ITERS] : 0.0,
                         b[RT_BALL_ITERS] ? (double)r[RT_SAMPLER_BALL_ROUNDS] / b[RT_BALL_ITERS] : 0.0);
        }
    }
    if (prof) {
        unsigned long long c[RT_STATS_LEN];
        HIP_TRY(hipMemcpy(c, s->stats, sizeof c, hipMemcpyDeviceToHost));
        if (std::getenv("RTNW_TRACE")) {   // the ball waves' share of the stage cycles (diagnostics only)
            const unsigned long long *b = c + RT_STAT_BALL;
            std::fprintf(stderr,
                         "rtnw ball waves (profile): iterations %llu of %llu; cycles claim %llu of %llu, traverse %llu of "
                         "%llu, media %llu of %llu, shade %llu of %llu; fused in-ball trips %llu, their cycles %llu "
                         "(part of traverse)\n",
                         b[4], b[5], b[0], c[RT_STAT_PROF], b[1], c[RT_STAT_PROF + 1], b[2], c[RT_STAT_PROF + 2], b[3],
                         c[RT_STAT_PROF + 3], b[6], b[7]);
        }
        stats->cycles_claim = (double)c[RT_STAT_PROF + 0];
        stats->cycles_traverse = (double)c[RT_STAT_PROF + 1];
        stats->cycles_media = (double)c[RT_STAT_PROF + 2];
        stats->cycles_shade = (double)c[RT_STAT_PROF + 3];
        stats->cycles_scatter = (double)c[RT_STAT_SHADE + 3];
        // wave timeline of the last batch, s_memrealtime at 100 MHz (kernel: kProf)
        const unsigned long long *T = c + RT_STAT_TIME;
        const double t0 = (double)~T[0], us = 0.01;
        stats->wave_exhaust_first_us = ((double)~T[1] - t0) * us;
        stats->wave_exhaust_last_us = ((double)T[2] - t0) * us;
        stats->wave_end_first_us = ((double)~T[3] - t0) * us;
        stats->wave_end_last_us = ((double)T[4] - t0) * us;
        stats->wave_end_mean_us = T[6] ? (double)T[5] / (double)T[6] * us : 0.0;   // T[5]: sum of lifetimes
    }
    return RT_OK;
}

}  // namespace

// The scene part of a launch's arguments: the arrays, and what rt_scene_create found.
void fill_scene_args(const rt_scene *s, RtKernelArgs &a) {
    a.nodes = (const float4 *)s->nodes;
    a.prims = (const float4 *)s->prims;
    a.bprims = (const float4 *)s->bprims;
    a.media = (const int4 *)s->media;
    a.mats = (const float4 *)s->mats;
    a.texs = (const float4 *)s->texs;
    a.insts = (const float4 *)s->insts;
    a.ranvec = (const float4 *)s->ranvec;
    a.perm = (const int *)s->perm;
    a.texels = (const uint8_t *)s->texels;
    a.root = s->root;
    a.nnodes = (uint32_t)s->nnodes;
    a.bvh_width = s->bvh_width;
    a.has_bvh = s->has_bvh;
    a.nmedia = s->nmedia;
    a.lds_nodes = s->lds_nodes ? 1 : 0;
    a.scan = s->scan ? 1 : 0;
    a.groups = (const float4 *)s->groups;
    a.ngroups = s->ngroups;
    a.nprescan = s->nprescan;
    a.cell_first = s->cell_first;
    a.cell_n = s->cell_n;
    for (int k = 0; k < 3; k++) a.cell_c[k] = s->cell_c[k];
    a.cell_r2 = s->cell_r2;
    a.cell_rin2 = s->cell_rin2;
    a.nprims = (uint32_t)s->nprims;
    a.stack_depth = s->stack_depth;
    a.features = scene_features(s);
}

// The camera and the image part: what a primary ray is made from.
void fill_camera_args(const rt_camera_desc *cam, const rt_render_params *p, RtKernelArgs &a) {
    for (int k = 0; k < 3; k++) {
        a.org[k] = cam->origin[k];
        a.llc[k] = cam->lower_left_corner[k];
        a.hor[k] = cam->horizontal[k];
        a.ver[k] = cam->vertical[k];
        a.cu[k] = cam->u[k];
        a.cv[k] = cam->v[k];
    }
    a.lens = cam->lens_radius;
    a.ct0 = cam->time0;
    a.ct1 = cam->time1;
    a.nx = p->nx;
    a.ny = p->ny;
    a.rnx = 1.0f / (float)p->nx;   // nx, ny >= 1: normal reciprocals (div_rn, rt_device.h)
    a.rny = 1.0f / (float)p->ny;
    a.tmin = p->t_min;
    a.seed = p->seed;
}

// The shading stage's rejection sampler (RT_COOP_LOCAL above): any setting computes the same.
void fill_sampler_args(RtKernelArgs &a) {
    a.coop_local = env_int("RTNW_COOP_LOCAL", RT_COOP_LOCAL, 0, 3);
    a.coop_local_min = env_int("RTNW_COOP_LOCAL_MIN", RT_COOP_LOCAL_MIN, 1, 64);
}

// Whether a job lists the pixels whose primary rays enter a dense medium first
// (RTNW_DEEP_FIRST=0: never).
bool deep_first(const rt_scene *s) {
    bool v = !s->deep_balls.empty();
    if (const char *e = std::getenv("RTNW_DEEP_FIRST")) v = v && std::atoi(e) != 0;
    return v;
}

// The limits of rt_render_params (rt_hip.h), held by every render entry point with its other
// arguments, before any HIP call.
int render_params_check(const rt_render_params *p) {
    if (p->nx <= 0 || p->ny <= 0 || p->spp <= 0 || p->max_depth < 0) return fail(RT_ERR_INVALID, "bad render parameters");
    if (p->nx > 65535 || p->ny > 65535) return fail(RT_ERR_INVALID, "nx and ny must be in 1..65535");
    if (!rtnw::sample_range_ok(p->sample_offset, p->spp))
        return fail(RT_ERR_INVALID, "sample_offset + spp must not pass 0xFFFFFFFF (32-bit sample indices)");
    return RT_OK;
}

// The body of rt_render_tiles and rt_render_tiles_moments: the job is the tile list, or `js`
// when non-null; with mom_dev the resolve is rt_moments.hip's, which also keeps the moments.
int render_job(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p, const int32_t *tiles, int ntiles,
               const JobSlots *js, float *out_dev, float *mom_dev, void *stream_v, rt_stats *stats) {
    if (int rc = render_params_check(p)) return rc;
    if (s->has_moving && (cam->time0 < s->time0 || cam->time1 > s->time1))
        return fail(RT_ERR_INVALID, "camera shutter outside the scene's time span (moving-sphere bounds)");
    // RT_FLAG_RIGHT_FOLD (rt_hip.h): plain renders of width-2 scenes only, and a stack of
    // max_depth attenuations (16 B each) for every lane of the launch, within the slab
    // budget's default (RTNW_SLAB_BUDGET shapes the sample batches, not this bound)
    const bool fold = (p->flags & RT_FLAG_RIGHT_FOLD) != 0;
    const uint64_t fold_lanes = (uint64_t)s->grid[0] * block_threads(s);
    const uint64_t fold_bytes = fold ? fold_lanes * (uint64_t)std::max(1, p->max_depth) * sizeof(float4) : 0;
    if (fold) {
        if (p->flags & (RT_FLAG_COUNT | RT_FLAG_PROFILE))
            return fail(RT_ERR_INVALID, "RT_FLAG_RIGHT_FOLD cannot be combined with RT_FLAG_COUNT or RT_FLAG_PROFILE");
        if (s->bvh_width != 2)
            return fail(RT_ERR_UNSUPPORTED, "RT_FLAG_RIGHT_FOLD needs a scene with a 2-wide BVH (RTNW_BVH_WIDTH=2)");
        if (!rt_megakernel_has_fold())
            return fail(RT_ERR_UNSUPPORTED, "RT_FLAG_RIGHT_FOLD: this library was linked without the fold variants (rt_kernel_fold.o)");
        if (fold_bytes > RT_SLAB_BUDGET)
            return fail(RT_ERR_INVALID, "RT_FLAG_RIGHT_FOLD: max_depth " + std::to_string(p->max_depth) + " needs a " +
                                            std::to_string(fold_bytes) + "-byte attenuation stack, over the " +
                                            std::to_string(RT_SLAB_BUDGET) + "-byte budget");
    }
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t)stream_v;
    if (int rc = js ? prepare_job_slots(s, *js, p->nx, p->ny, stream) : prepare_job(s, tiles, ntiles, p->nx, p->ny, cam))
        return rc;

    // the job's sample batches (rtnw::plan_batches: one partial sum, rgb, per work item)
    const int chunk = p->chunk > 0 ? p->chunk : 1;
    const uint64_t item_bytes = 4 * (uint64_t)rt_slab_floats();
    rtnw::BatchPlan plan;
    if (int rc = rtnw::plan_batches(s->npix, p->spp, chunk, slab_budget(), item_bytes, &plan)) return rc;
    const uint64_t nbatches = plan.nbatches, nchunks_total = plan.nchunks_total;
    if (int rc = s->slab.reserve((size_t)s->npix * plan.per * item_bytes)) return rc;
    if (int rc = s->acc.reserve(nbatches > 1 ? (size_t)s->npix * 16 : 0)) return rc;
    if (int rc = s->fold.reserve(fold_bytes)) return rc;
    const bool count = (p->flags & RT_FLAG_COUNT) != 0;
    const bool prof = !count && (p->flags & RT_FLAG_PROFILE) != 0;
    const bool sum_in = (p->flags & RT_FLAG_SUM_IN) != 0, sum_out = (p->flags & RT_FLAG_SUM_OUT) != 0;
    const int mode = count ? 1 : (prof ? 2 : 0);
    if (count || prof) HIP_TRY(hipMemsetAsync(s->stats, 0, RT_STATS_LEN * sizeof(unsigned long long), stream));

    RtKernelArgs a{};
    fill_scene_args(s, a);
    fill_camera_args(cam, p, a);
    a.need_dlen = s->nmedia > 0 || s->has_specular || p->background == RT_BG_SKY;
    // (a scene without a medium cell has no paths for ball waves: none are made)
    a.ball_waves = s->cell_n > 0 ? ball_waves() : 0;
    a.ball_fast = s->ball_fast ? env_int("RTNW_BALL_FAST", RT_BALL_FAST, 0, 64) : 0;
    for (int i = 0; i < 2; i++)
        for (int k = 0; k < 3; k++) a.ball_alb[i][k] = s->ball_alb[i][k];
    a.ball_batch = env_int("RTNW_BALL_BATCH", RT_BALL_BATCH, 1, 64);
    a.ball_claim = env_int("RTNW_BALL_CLAIM", RT_BALL_CLAIM, 1, 64);
    a.ball_park = env_int("RTNW_BALL_PARK", 1, 0, 1);
    a.ball_drain = env_int("RTNW_BALL_DRAIN", 1, 0, 1);
    fill_sampler_args(a);
    a.ns = p->spp;
    a.max_depth = p->max_depth;
    a.background = p->background;
    a.chunk = chunk;
    a.job_xy = (const uint32_t *)s->job_xy.p;
    a.npix = s->npix;
    a.slab = (float *)s->slab.p;
    a.counter = (uint32_t *)s->counter.p;
    a.stats = (unsigned long long *)s->stats;
    // RTNW_WAVE_LOG=<file> with RT_FLAG_PROFILE: every wave's timeline appended to the
    // file as 5 uint64 (start, pool dry, end in s_memrealtime ticks, xcc << 32 | HW_ID,
    // items claimed) per wave and batch (tools/tail_probe.py --wave-log; diagnostics)
    const char *wave_log_path = prof ? std::getenv("RTNW_WAVE_LOG") : nullptr;
    DevBuf wave_log;   // freed by every return below, error paths included
    const size_t wave_log_n = (size_t)s->grid[2] * (block_threads(s) / 64) * RT_WAVE_LOG_WORDS;
    if (wave_log_path) {
        if (int rc = wave_log.reserve(wave_log_n * sizeof(unsigned long long))) return rc;
        HIP_TRY(hipMemsetAsync(wave_log.p, 0, wave_log_n * sizeof(unsigned long long), stream));
    }
    a.wave_log = (unsigned long long *)wave_log.p;
    a.fold = fold ? (float4 *)s->fold.p : nullptr;
    a.fold_stride = (uint32_t)fold_lanes;
    // refill finishes the samples of the job's empty pixels itself (rt_megakernel.h): a tile job of a
    // scene and camera that allow it (prepare_job, empty_pixels.cpp), one sample per work item (the
    // item is then the sample), no hit before the origin, not the right fold
    const bool empty_fast = s->job_empty && rtnw::empty_fast_render_ok(p->t_min, chunk, p->flags, !js);
    a.empty_bits = empty_fast ? (const uint32_t *)s->empty_bits.p : nullptr;

    // vec3::operator/= (vec3.h:134-141): col *= float(1.0 / ns)
    const uint32_t ns_total = sum_in ? p->sample_offset + (uint32_t)p->spp : (uint32_t)p->spp;
    const float k = (float)(1.0 / (double)(float)ns_total);
    const uint64_t waves = (uint64_t)s->grid[mode] * (block_threads(s) / 64);
    double kernel_ms = 0, resolve_ms = 0;
    // RTNW_CLAIM (x 64 items) and RTNW_TAIL_CLAIMS override the claim sizes (tests, A/B runs); -1: none
    const char *ec = std::getenv("RTNW_CLAIM"), *et = std::getenv("RTNW_TAIL_CLAIMS");
    const int claim_x64 = ec ? std::max(1, std::atoi(ec)) : -1, tail_claims = et ? std::max(0, std::atoi(et)) : -1;
    for (uint64_t b = 0; b < nbatches; ++b) {
        const rtnw::BatchLaunch l = rtnw::plan_batch(plan, b, s->npix, p->spp, chunk, p->sample_offset, waves, s->job_ndeep,
                                                     claim_x64, tail_claims);
        a.ns = l.ns;
        a.sample_offset = l.sample_offset;
        a.nchunks = l.nchunks;
        a.nitems = l.nitems;
        a.ndeep = s->job_ndeep;
        a.ndeep_items = l.ndeep_items;
        a.claim = l.claim;
        a.claim_tail = l.claim_tail;
        a.nbig = l.nbig;
        const int rmode = (b == 0 ? RT_RESOLVE_FIRST : 0) | (b + 1 == nbatches ? RT_RESOLVE_LAST : 0) |
                          (sum_in ? RT_RESOLVE_SUM_IN : 0) | (sum_out ? RT_RESOLVE_RAW : 0);
        HIP_TRY(hipMemsetAsync(s->counter.p, 0, 64, stream));
        // the wave timeline describes the last batch: its slots start from zero each launch
        if (prof)
            HIP_TRY(hipMemsetAsync((unsigned long long *)s->stats + RT_STAT_TIME, 0, 7 * sizeof(unsigned long long), stream));
        HIP_TRY(hipEventRecord(s->ev[0], stream));
        HIP_TRY(rt_launch_megakernel(&a, s->grid[mode], fold ? RT_LAUNCH_FOLD : mode, stream));
        HIP_TRY(hipEventRecord(s->ev[1], stream));
        if (mom_dev)
            HIP_TRY(rt_moments_launch.resolve((const float *)s->slab.p, rt_slab_floats(), s->npix, a.nchunks, k,
                                             (float4 *)s->acc.p, rmode, (const uint32_t *)s->job_out.p, out_dev, mom_dev,
                                             stream));
        else
            HIP_TRY(rt_launch_resolve((const float *)s->slab.p, s->npix, a.nchunks, k, (float4 *)s->acc.p, rmode,
                                      (const uint32_t *)s->job_out.p, out_dev, stream));
        HIP_TRY(hipEventRecord(s->ev[2], stream));
        if (wave_log.p) {
            std::vector<unsigned long long> h(wave_log_n);   // the render stream may be non-blocking
            HIP_TRY(hipMemcpyAsync(h.data(), wave_log.p, h.size() * sizeof h[0], hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (FILE *f = std::fopen(wave_log_path, "ab")) {
                std::fwrite(h.data(), sizeof h[0], h.size(), f);
                std::fclose(f);
            }
        }
        if (stats) {   // one batch at a time: the events are reused
            HIP_TRY(hipEventSynchronize(s->ev[2]));
            float ms0 = 0, ms1 = 0;
            HIP_TRY(hipEventElapsedTime(&ms0, s->ev[0], s->ev[1]));
            HIP_TRY(hipEventElapsedTime(&ms1, s->ev[1], s->ev[2]));
            kernel_ms += ms0;
            resolve_ms += ms1;
        }
    }

    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->samples = (double)s->npix * (double)p->spp;
        stats->chunk = (double)chunk;
        stats->batches = (double)nbatches;
        stats->kernel_ms = kernel_ms;
        stats->resolve_ms = resolve_ms;
        if (int rc = read_counters(s, count, prof, (double)s->npix * (double)nchunks_total, stats)) return rc;
        stats->grid = (double)s->grid[mode];
        stats->lds_level = s->lds_nodes ? 1.0 : 0.0;
        stats->scan_groups = s->scan ? (double)s->ngroups : 0.0;
        stats->prescan = (double)s->nprescan;
        stats->stack_depth = (double)(s->lds_nodes ? s->stack_depth : s->bvh_width >= 8 ? RT_STACK_DEPTH_W8 : RT_STACK_DEPTH);
        stats->empty_pixels = a.empty_bits ? (double)s->job_nflagged : 0.0;
    }
    return RT_OK;
}

extern "C" {

int rt_render_tiles(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p, const int32_t *tiles, int ntiles,
                    float *out_dev, void *stream_v, rt_stats *stats) {
    if (!s || !cam || !p || ntiles < 0) return fail(RT_ERR_INVALID, "rt_render_tiles: bad argument");
    if (int rc = render_params_check(p)) return rc;   // a rank with no tiles answers as the others do
    if (ntiles == 0) {   // a rank with no tiles (more ranks than tiles) has nothing to do
        if (stats) std::memset(stats, 0, sizeof *stats);
        return RT_OK;
    }
    if (!tiles || !out_dev) return fail(RT_ERR_INVALID, "rt_render_tiles: null tiles or output");
    return render_job(s, cam, p, tiles, ntiles, nullptr, out_dev, nullptr, stream_v, stats);
}

int rt_render_tiles_moments(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p, const int32_t *tiles,
                            int ntiles, float *out_dev, float *moments_dev, void *stream_v, rt_stats *stats) {
    if (!cam || !p || ntiles < 0) return fail(RT_ERR_INVALID, "rt_render_tiles_moments: bad argument");
    if (p->flags & (RT_FLAG_COUNT | RT_FLAG_PROFILE))
        return fail(RT_ERR_INVALID, "rt_render_tiles_moments: RT_FLAG_COUNT and RT_FLAG_PROFILE are not supported");
    if (!s) return fail(RT_ERR_INVALID, "rt_render_tiles_moments: null scene");
    if (int rc = render_params_check(p)) return rc;
    if (!rt_moments_launch.resolve)
        return fail(RT_ERR_UNSUPPORTED, "rt_render_tiles_moments: this library was linked without the moments unit (rt_moments.o)");
    if (ntiles == 0) {
        if (stats) std::memset(stats, 0, sizeof *stats);
        return RT_OK;
    }
    if (!tiles || !out_dev || !moments_dev) return fail(RT_ERR_INVALID, "rt_render_tiles_moments: null tiles, output or moments");
    return render_job(s, cam, p, tiles, ntiles, nullptr, out_dev, moments_dev, stream_v, stats);
}

int rt_render_tile(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p, int x0, int y0, int w, int h,
                   float *out_rgb, rt_stats *stats) {
    if (!s || !out_rgb || !cam || !p) return fail(RT_ERR_INVALID, "rt_render_tile: bad argument");
    if (int rc = render_params_check(p)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t bytes = (size_t)w * h * 3 * sizeof(float);
    if (w <= 0 || h <= 0) return fail(RT_ERR_INVALID, "empty tile");
    if (int rc = s->host_out.reserve(bytes)) return rc;
    if (int rc = ensure_own_stream(s)) return rc;
    const int32_t tile[4] = {x0, y0, w, h};
    if (p && (p->flags & RT_FLAG_SUM_IN))   // the running sums come from the caller's buffer
        HIP_TRY(hipMemcpyAsync(s->host_out.p, out_rgb, bytes, hipMemcpyHostToDevice, s->own_stream));
    rt_stats local;
    if (int rc = rt_render_tiles(s, cam, p, tile, 1, (float *)s->host_out.p, s->own_stream, stats ? stats : &local)) return rc;
    HIP_TRY(hipMemcpyAsync(out_rgb, s->host_out.p, bytes, hipMemcpyDeviceToHost, s->own_stream));
    HIP_TRY(hipStreamSynchronize(s->own_stream));
    return RT_OK;
}

}  // extern "C"
