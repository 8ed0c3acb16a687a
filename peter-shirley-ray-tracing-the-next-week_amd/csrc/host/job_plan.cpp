// job_plan.cpp — the arithmetic of a render job: pixel order, sample batches, claim sizes.
// A sample's value depends only on its (pixel, sample) key, so none of this shows in an
// image unless a pixel is lost or doubled: its properties are checked on the host
// (tests/native/host_sanitize.cpp).
#include "job_plan.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace rtnw {

namespace {
int fail(int code, const std::string &msg) { return rt_internal_fail(code, msg); }
}  // namespace

bool deep_pixel(const SceneInfo &s, const rt_camera_desc *cam, int x, int y, int nx, int ny) {
    // the pixel centre's primary ray (main.cpp:305-306, camera.h:52-55 without jitter or lens)
    const float u = (x + 0.5f) / nx, v = (ny - 1 - y + 0.5f) / ny;
    float o[3], d[3];
    for (int k = 0; k < 3; k++) {
        o[k] = cam->origin[k];
        d[k] = cam->lower_left_corner[k] + u * cam->horizontal[k] + v * cam->vertical[k] - o[k];
    }
    for (size_t b = 0; b + 3 < s.deep_balls.size(); b += 4) {
        const float *c = &s.deep_balls[b];
        const double oc[3] = {o[0] - (double)c[0], o[1] - (double)c[1], o[2] - (double)c[2]};
        const double a = (double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2];
        const double bb = oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2];
        const double cc = oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2] - (double)c[3] * c[3];
        if (bb * bb - a * cc > 0 && (bb < 0 || cc < 0)) return true;
    }
    return false;
}

// Job pixel order: tiles in the order given; inside a tile, bands of 8 rows listed
// column by column (8 pixels per column), so that ANY 64 consecutive items — a wave
// claim, wherever it starts — are 8 neighbouring columns of one band (coherent
// primary rays), also when the tile width is not a multiple of 8 (500 = 62.5 x 8).
int tile_job_order(const int32_t *tiles, int ntiles, int nx, int ny, const DeepTest &deep, std::vector<uint32_t> *xy_out,
                   std::vector<uint32_t> *oi_out, uint32_t *ndeep_out) {
    std::vector<uint32_t> xy, oi;
    uint32_t base = 0;
    for (int t = 0; t < ntiles; t++) {
        const int x0 = tiles[4 * t], y0 = tiles[4 * t + 1], w = tiles[4 * t + 2], h = tiles[4 * t + 3];
        // (the image's size first: nx - x0 cannot overflow where x0 + w could)
        if (nx < 1 || ny < 1 || nx > 65535 || ny > 65535 || w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || w > nx - x0 || h > ny - y0)
            return fail(RT_ERR_INVALID, "tile outside the image");
        for (int by = 0; by < h; by += 8)
            for (int xx = 0; xx < w; xx++)
                for (int yy = by; yy < std::min(by + 8, h); yy++) {
                    xy.push_back((uint32_t)(x0 + xx) | ((uint32_t)(y0 + yy) << 16));
                    oi.push_back(base + ((uint32_t)yy * (uint32_t)w + (uint32_t)xx));
                }
        base += (uint32_t)w * (uint32_t)h;
    }
    // deep pixels first, each group in the band order above (a claim of 64 consecutive
    // items stays 64 neighbouring pixels of one group)
    uint32_t ndeep = 0;
    if (deep) {
        std::vector<uint32_t> dxy, doi, rxy, roi;
        for (size_t i = 0; i < xy.size(); i++) {
            const bool in = deep((int)(xy[i] & 0xFFFFu), (int)(xy[i] >> 16));
            (in ? dxy : rxy).push_back(xy[i]);
            (in ? doi : roi).push_back(oi[i]);
        }
        ndeep = (uint32_t)dxy.size();
        if (ndeep == xy.size()) ndeep = 0;   // all deep: one group
        dxy.insert(dxy.end(), rxy.begin(), rxy.end());
        doi.insert(doi.end(), roi.begin(), roi.end());
        xy.swap(dxy);
        oi.swap(doi);
    }
    xy_out->swap(xy);
    oi_out->swap(oi);
    *ndeep_out = ndeep;
    return RT_OK;
}

void fill_deep_map(const SceneInfo &s, const rt_camera_desc *cam, int x0, int y0, int w, int h, int nx, int ny,
                   std::vector<uint8_t> *deep) {
    deep->resize((size_t)w * h);
    for (int yy = 0; yy < h; yy++)
        for (int xx = 0; xx < w; xx++) (*deep)[(size_t)yy * w + xx] = deep_pixel(s, cam, x0 + xx, y0 + yy, nx, ny);
}

// The active pixels, the deep ones first; each group block by block (8 x 8 blocks of the frame
// in raster order), a block column by column, so that a wave's 64 items stay neighbours.  One
// sweep without a branch on the flags (they are as good as random): every pixel is written to
// the end of both lists, and a list grows only if the pixel is its own.
int active_job_order(const std::string &who, const uint8_t *flags, int x0, int y0, int w, int h, uint32_t nactive,
                     ActiveJobState *st, uint32_t *xy, uint32_t *slot, uint32_t *ndeep_out) {
    const uint32_t npix = (uint32_t)w * (uint32_t)h;
    const std::vector<uint8_t> &deep = st->deep;
    std::vector<uint32_t> &rxy = st->rxy, &rslot = st->rslot;
    const bool deep_front = !deep.empty();
    uint32_t n = 0, nr = 0;
    if (deep_front && rxy.empty()) {
        rxy.resize((size_t)npix + 1);
        rslot.resize((size_t)npix + 1);
    }
    for (int by = 0; by < h; by += 8)
        for (int bx = 0; bx < w; bx += 8)
            for (int xx = bx; xx < std::min(bx + 8, w); xx++)
                for (int yy = by; yy < std::min(by + 8, h); yy++) {
                    const uint32_t o = (uint32_t)yy * (uint32_t)w + (uint32_t)xx;
                    const uint32_t v = (uint32_t)(x0 + xx) | ((uint32_t)(y0 + yy) << 16);
                    const uint32_t on = flags[o] != 0;
                    if (deep_front) {
                        const uint32_t d = deep[o] != 0;
                        rxy[nr] = v;
                        rslot[nr] = o;
                        nr += on & (d ^ 1u);
                        xy[n] = v;
                        slot[n] = o;
                        n += on & d;
                    } else {
                        xy[n] = v;
                        slot[n] = o;
                        n += on;
                    }
                }
    *ndeep_out = deep_front ? n : 0;
    if ((uint64_t)n + nr > npix) return fail(RT_ERR_HIP, who + ": pixel list overflow");
    if (nr) {
        std::memcpy(xy + n, rxy.data(), (size_t)nr * sizeof(uint32_t));
        std::memcpy(slot + n, rslot.data(), (size_t)nr * sizeof(uint32_t));
        n += nr;
    }
    if (n != nactive) return fail(RT_ERR_HIP, who + ": the active flags and their count disagree");
    return RT_OK;
}

// Work item = `chunk` samples of one pixel, one by default: short items keep each
// wave's lanes on neighbouring pixels (a wave deals its claims to lanes as they free
// up; long items let its pixels drift apart): 16 -> 1 sample per item is 92.2 ->
// 81.8 ms on c4.  The partial-sum slab holds one rgb (item_bytes) per item
// of a launch; a job whose slab would pass the budget runs as several launches
// over sample batches (whole chunks), and the resolve adds every batch to a
// per-pixel running sum in sample order — so the sum is the same sequence of
// float adds whatever the batch size, i.e. the image does not depend on the job's
// size (one GPU or a rank's share of eight).  A launch has at most 2^32 - 65 items: the
// kernel's 32-bit item index plus a claim of 64 does not wrap.
int plan_batches(uint64_t npix, int spp, int chunk, uint64_t budget_bytes, uint64_t item_bytes, BatchPlan *out) {
    const uint64_t nchunks_total = ((uint64_t)spp + chunk - 1) / chunk;
    const uint64_t max_items = 0xFFFFFFFFull - 64;
    if (npix > max_items) return fail(RT_ERR_INVALID, "job too large (pixels >= 2^32)");
    uint64_t per = std::max<uint64_t>(1, budget_bytes / (npix * item_bytes));
    per = std::min<uint64_t>(per, max_items / npix);
    per = std::min<uint64_t>(per, nchunks_total);
    const uint64_t nbatches = (nchunks_total + per - 1) / per;
    per = (nchunks_total + nbatches - 1) / nbatches;   // batches of (nearly) equal size, as many
    *out = BatchPlan{per, nbatches, nchunks_total};
    return RT_OK;
}

// Small claims per wave at the end of a launch.
#define RT_TAIL_CLAIMS 32

BatchLaunch plan_batch(const BatchPlan &pl, uint64_t b, uint64_t npix, int spp, int chunk, uint32_t sample_offset,
                       uint64_t waves, uint32_t job_ndeep, int claim_x64, int tail_claims) {
    BatchLaunch l{};
    const uint64_t c0 = b * pl.per, c1 = std::min(c0 + pl.per, pl.nchunks_total);
    const uint64_t s0 = c0 * (uint64_t)chunk, s1 = std::min<uint64_t>(c1 * (uint64_t)chunk, (uint64_t)spp);
    l.ns = (int)(s1 - s0);                                 // samples of this batch
    l.sample_offset = sample_offset + (uint32_t)s0;        // their first sample index
    l.nchunks = (int)(c1 - c0);
    const uint64_t nitems = npix * (c1 - c0);
    l.nitems = (uint32_t)nitems;
    l.ndeep_items = (uint32_t)((uint64_t)job_ndeep * (c1 - c0));
    // Claim size: up to 512 items per atomic (64 -> 512 is 81.6 -> 76.9 ms on c4:
    // fewer round trips to the one contended counter), at least 8
    // claims per wave so that small jobs still spread over every wave.
    // The last RT_TAIL_CLAIMS claims per wave are of 64 items: with 512-item claims
    // to the end, the waves ran dry over 2.4 ms (the first found the pool empty at
    // 54.1 ms of a 57.1-ms launch, the last at 56.5; with 64-item claims over 0.5 ms,
    // but every claim is a round trip to the one device-scope counter:
    // tools/tail_probe.py).
    uint64_t c = std::min<uint64_t>(std::max<uint64_t>(nitems / (waves * 8) / 64 * 64, 64), 512);
    uint64_t tail = 64 * RT_TAIL_CLAIMS * waves;
    if (claim_x64 >= 0) c = (uint64_t)std::max(1, claim_x64) * 64;   // x 64 items
    if (tail_claims >= 0) tail = 64 * (uint64_t)tail_claims * waves;
    l.claim = (uint32_t)c;
    l.claim_tail = 64;
    l.nbig = (uint32_t)(nitems > tail ? (nitems - tail) / c : 0);
    return l;
}

int plan_feature_batches(uint64_t npix, int spp, uint64_t pixel_bytes, uint64_t slab_bytes, uint64_t *per_out) {
    uint64_t per = std::max<uint64_t>(1, slab_bytes / (npix * pixel_bytes));
    per = std::min<uint64_t>(per, std::max<uint64_t>(1, 0x7FFFFFFFull / npix));
    per = std::min<uint64_t>(per, (uint64_t)spp);
    if (npix * per >= 0x80000000ull) return fail(RT_ERR_INVALID, "rt_render_features: rectangle too large");
    *per_out = per;
    return RT_OK;
}

uint64_t plan_trace_batch(uint64_t n, const char *knob) {
    uint64_t per = RT_TRACE_BATCH;
    if (knob) {
        const long long v = std::atoll(knob);
        if (v > 0) per = std::min<uint64_t>((uint64_t)v, RT_TRACE_BATCH_MAX);
    }
    return std::max<uint64_t>(1, std::min(per, n));
}

uint64_t lens_batch_limit(const char *knob) {
    uint64_t limit = RT_LENS_BATCH;
    if (knob) {
        const long long v = std::atoll(knob);
        if (v > 0) limit = std::min<uint64_t>((uint64_t)v, RT_LENS_BATCH_MAX);
    }
    return limit;
}

LensPlan plan_lens(uint64_t npix, uint64_t spp, uint64_t limit) {
    LensPlan pl{};
    limit = std::max<uint64_t>(1, limit);
    pl.pix_per = std::max<uint64_t>(1, std::min(limit, npix));
    pl.smp_per = std::max<uint64_t>(1, std::min(limit / pl.pix_per, spp));   // whole planes of the block
    pl.nblocks = (npix + pl.pix_per - 1) / pl.pix_per;
    pl.nruns = (spp + pl.smp_per - 1) / pl.smp_per;
    pl.nbatches = pl.nblocks * pl.nruns;
    pl.rays_per = pl.pix_per * pl.smp_per;
    return pl;
}

LensBatch lens_batch(const LensPlan &pl, uint64_t b, uint64_t npix, uint64_t spp) {
    const uint64_t block = b / pl.nruns, run = b - block * pl.nruns;
    LensBatch l;
    l.p0 = block * pl.pix_per;
    l.np = std::min(pl.pix_per, npix - l.p0);
    l.s0 = run * pl.smp_per;
    l.ns = std::min(pl.smp_per, spp - l.s0);
    return l;
}

}  // namespace rtnw
