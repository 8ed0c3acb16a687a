// job_plan.h — the arithmetic of a render job (job_plan.cpp): the order of its pixels, its
// sample batches and each launch's claim sizes.  Host arithmetic only, no HIP, so that it
// runs, and is tested, without a GPU (tests/native/host_sanitize.cpp).
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "scene_lower.h"

#pragma GCC visibility push(hidden)
namespace rtnw {

// Whether the primary ray through the centre of pixel (x, y) enters one of the scene's dense
// media first (SceneInfo::deep_balls).
bool deep_pixel(const SceneInfo &s, const rt_camera_desc *cam, int x, int y, int nx, int ny);

// The pixel lists of a tile job: pixel k of the job is image pixel xy[k] (x | y << 16) and
// goes to oi[k] of the packed output.  `deep` (x, y) -> bool lists the deep pixels first,
// ndeep of them (0 when all are deep: one group); empty: no such split.
using DeepTest = std::function<bool(int, int)>;
int tile_job_order(const int32_t *tiles, int ntiles, int nx, int ny, const DeepTest &deep, std::vector<uint32_t> *xy,
                   std::vector<uint32_t> *oi, uint32_t *ndeep);

// The pixel lists of an adaptive pass over the frame (x0, y0, w, h): the pixels whose flag is
// set, into xy and slot (room for w * h + 1 entries each; slot = yy * w + xx).  With a deep map
// in the frame's state the deep ones come first, *ndeep of them.  The state also keeps the other
// group's scratch lists between the frame's passes.
struct ActiveJobState {
    std::vector<uint8_t> deep;          // one byte per slot (fill_deep_map); empty: no split
    std::vector<uint32_t> rxy, rslot;
};
void fill_deep_map(const SceneInfo &s, const rt_camera_desc *cam, int x0, int y0, int w, int h, int nx, int ny,
                   std::vector<uint8_t> *deep);
int active_job_order(const std::string &who, const uint8_t *flags, int x0, int y0, int w, int h, uint32_t nactive,
                     ActiveJobState *st, uint32_t *xy, uint32_t *slot, uint32_t *ndeep);

// The legal sample ranges (rt_hip.h, rt_render_params): sample indices are 32-bit, and the last
// one, sample_offset + spp - 1, must be below 0xFFFFFFFF, so that the count sample_offset + spp
// (the mean's divisor under RT_FLAG_SUM_IN) is a uint32_t too.
inline bool sample_range_ok(uint32_t sample_offset, int spp) {
    return spp > 0 && (uint64_t)sample_offset + (uint64_t)spp <= 0xFFFFFFFFull;
}

// Sample batches of a render job: `per` chunks of every pixel per launch, nbatches launches.
struct BatchPlan {
    uint64_t per, nbatches, nchunks_total;
};
int plan_batches(uint64_t npix, int spp, int chunk, uint64_t budget_bytes, uint64_t item_bytes, BatchPlan *out);

// Launch b of a plan: its samples, its items and how the waves claim them (RtKernelArgs).
// claim_x64 and tail_claims are the overrides RTNW_CLAIM and RTNW_TAIL_CLAIMS, negative: none.
struct BatchLaunch {
    int ns;
    uint32_t sample_offset;
    int nchunks;
    uint32_t nitems, ndeep_items, claim, claim_tail, nbig;
};
BatchLaunch plan_batch(const BatchPlan &pl, uint64_t b, uint64_t npix, int spp, int chunk, uint32_t sample_offset,
                       uint64_t waves, uint32_t job_ndeep, int claim_x64, int tail_claims);

// The feature pass's own rule: batches of *per whole samples of every pixel within slab_bytes.
int plan_feature_batches(uint64_t npix, int spp, uint64_t pixel_bytes, uint64_t slab_bytes, uint64_t *per);

// Ray queries (capi_trace.cpp): the legal ray counts (one launch takes fewer than 2^31 lanes, and
// a batch is at most the whole call), and the rays per batch of a host-side call: `knob` is
// RTNW_TRACE_BATCH's text (NULL or not a positive number: RT_TRACE_BATCH rays), clipped to
// 1..RT_TRACE_BATCH_MAX and to n.  n >= 1.
#define RT_TRACE_BATCH (1ull << 20)       // 48 MiB of rays and as much of hits
#define RT_TRACE_BATCH_MAX (1ull << 24)
inline bool ray_count_ok(int64_t n) { return n >= 0 && n <= 0x7FFFFFFFll; }
uint64_t plan_trace_batch(uint64_t n, const char *knob);

// Lens renders (capi_lens.cpp): the batches of a w x h rectangle's npix pixels times spp samples.
// A batch is a run of whole sample planes of a pixel block, pixels [p0, p0 + np) (row-major in
// the rectangle) times samples [s0, s0 + ns) (counted from the call's first), of at most `limit`
// rays, limit >= 1; lens_batch_limit reads it from RTNW_LENS_BATCH's text (NULL or not a positive
// number: RT_LENS_BATCH; clipped to 1..RT_LENS_BATCH_MAX, so always below 2^31).  Batch
// b < nbatches lists the pixel blocks in order and, inside a block, its sample runs in order: a
// pixel's samples arrive in sample order.
#define RT_LENS_BATCH (1ull << 21)        // 128 MiB of records and radiance, 320 MiB with the guides' rays and hits
#define RT_LENS_BATCH_MAX (1ull << 24)
struct LensPlan {
    uint64_t pix_per, smp_per;    // pixels per block, samples per run
    uint64_t nblocks, nruns;      // blocks of the rectangle, runs of the sample range
    uint64_t nbatches;            // nblocks * nruns
    uint64_t rays_per;            // pix_per * smp_per: the largest batch
};
struct LensBatch {
    uint64_t p0, np, s0, ns;
};
uint64_t lens_batch_limit(const char *knob);
LensPlan plan_lens(uint64_t npix, uint64_t spp, uint64_t limit);
LensBatch lens_batch(const LensPlan &pl, uint64_t b, uint64_t npix, uint64_t spp);

// One buffer carved into regions declared one after another (capi_internal.h Staging): add(n)
// is the next region, n elements from where the one before ended; total is what all of them take.
struct Region {
    size_t at, n;
};
struct Regions {
    size_t total = 0;
    Region add(size_t n) { total += n; return Region{total - n, n}; }
};

}  // namespace rtnw
#pragma GCC visibility pop
