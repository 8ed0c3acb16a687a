// capi_internal.h — what the units of the C ABI (capi_*.cpp) share: the scene object, the
// error helpers, the grow-on-demand buffers, the launch-argument fillers and the side units' plumbing.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "rt_hip.h"
#include "../rt_layout.h"
#include "../hip/rt_kernel.h"
#include "scene_lower.h"
#include "job_plan.h"
#include "empty_pixels.h"

inline int fail(int code, const std::string &msg) { return rt_internal_fail(code, msg); }
inline int hip_fail(hipError_t e, const char *what) {
    return fail(RT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t e_ = (expr);                         \
        if (e_ != hipSuccess) return hip_fail(e_, #expr); \
    } while (0)
#define RT_TRY(expr)                      \
    do {                                  \
        if (int rc_ = (expr)) return rc_; \
    } while (0)

inline int env_int(const char *name, int dflt, int lo, int hi) {
    if (const char *e = std::getenv(name)) return std::max(lo, std::min(hi, std::atoi(e)));
    return dflt;
}

// A device buffer grown on demand (the old allocation is freed first; it never shrinks), its
// sibling in pinned host memory, and a set of events.  Each owns what it holds: whoever holds
// one (a scene, a call's frame) frees it by going away, error paths included.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int reserve(size_t n) {
        if (n <= bytes) return RT_OK;
        release();
        HIP_TRY(hipMalloc(&p, n));
        bytes = n;
        return RT_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};
struct PinBuf {
    void *p = nullptr;
    size_t bytes = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { release(); }
    int reserve(size_t n) {
        if (n <= bytes) return RT_OK;
        release();
        HIP_TRY(hipHostMalloc(&p, n, hipHostMallocDefault));
        bytes = n;
        return RT_OK;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};
template <int N>
struct Events {   // created by the holder (hipEventCreate(&ev[k])), destroyed here
    hipEvent_t e[N] = {};
    Events() = default;
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    ~Events() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    hipEvent_t &operator[](int k) { return e[k]; }
};

// Destroyed by `delete` with its device current (rt_scene_destroy): every member frees itself.
struct rt_scene : rtnw::SceneInfo {
    int device = 0;
    int cus = 0;
    int grid[3] = {0, 0, 0};      // persistent megakernel grid per variant (plain, count, profile)
    bool lds_nodes = false;       // the BVH2 fits the LDS variant (one RT_LDS_BLOCK workgroup per CU)
    int stack_depth = 0;          // its traversal stack entries per lane
    hipStream_t own_stream = nullptr;
    // scene in HBM: one allocation (arena) holding the arrays below (rtnw::LoweredScene's image)
    DevBuf arena;
    void *nodes = nullptr, *prims = nullptr, *bprims = nullptr, *media = nullptr, *mats = nullptr, *texs = nullptr,
         *insts = nullptr, *ranvec = nullptr, *perm = nullptr, *texels = nullptr, *groups = nullptr;
    // job cache
    std::vector<int32_t> job_tiles;
    uint32_t job_ndeep = 0;                 // the job's first job_ndeep pixels are the deep ones (prepare_job)
    uint32_t npix = 0;
    DevBuf job_xy, job_out;       // the job's pixel lists (both have room for the same number of pixels)
    // the tile job's provably empty pixels, one bit per job pixel (empty_pixels.cpp), made with the
    // lists and cached with them; job_empty: the bits describe the current job (a tile job of a
    // scene and camera with the feature on), job_nflagged of them set
    DevBuf empty_bits;
    bool job_empty = false;
    uint32_t job_nflagged = 0;
    DevBuf slab;
    DevBuf acc;                   // per-pixel running sums between sample batches
    DevBuf frame;                 // rt_render_adaptive: the frame's sums, moments, counts and flags ...
    PinBuf pin;                   // ... and pinned host memory for the passes' pixel lists, flags and counters
    DevBuf fold;                  // RT_FLAG_RIGHT_FOLD: the lanes' attenuation stacks (rt_kernel.h RtKernelArgs.fold)
    DevBuf counter;               // the work counter (64 B), then the statistics counters ...
    void *stats = nullptr;        // ... which start here
    DevBuf host_out;
    DevBuf trace_ws;              // rt_trace_rays, rt_occluded: one batch of rays, then its results
    DevBuf lens_ws;               // rt_render_lens: one batch of records, their radiance and, for guides, its rays and hits
    Events<3> ev;
    rt_scene() = default;
    ~rt_scene() {
        if (own_stream) (void)hipStreamDestroy(own_stream);
    }
};
// threads per workgroup of the scene's render launches (rt_megakernel.h rt_mega_block)
inline int block_threads(const rt_scene *s) { return s->lds_nodes ? RT_LDS_BLOCK : RT_BLOCK; }

// internal to the library: not among its dynamic symbols
#pragma GCC visibility push(hidden)

// capi_scene.cpp
int scene_features(const rt_scene *s);
int ensure_own_stream(rt_scene *s);   // created on first use (rt_scene_create)

// capi_render.cpp
void fill_scene_args(const rt_scene *s, RtKernelArgs &a);
void fill_camera_args(const rt_camera_desc *cam, const rt_render_params *p, RtKernelArgs &a);
void fill_sampler_args(RtKernelArgs &a);   // the shading stage's rejection sampler knobs (RTNW_COOP_LOCAL*)
bool deep_first(const rt_scene *s);
// rt_render_params' limits (rt_hip.h): RT_OK, or RT_ERR_INVALID with the message set
int render_params_check(const rt_render_params *p);
struct JobSlots {
    const uint32_t *xy, *slot;
    uint32_t n, ndeep;
};
int render_job(rt_scene *s, const rt_camera_desc *cam, const rt_render_params *p, const int32_t *tiles, int ntiles,
               const JobSlots *js, float *out_dev, float *mom_dev, void *stream_v, rt_stats *stats);

// capi_radiance.cpp, capi_trace.cpp: one launch over n < 2^31 records in device memory, as the
// queries' _dev forms enqueue it (the lens renders launch both: capi_lens.cpp)
int radiance_launch(rt_scene *s, const rt_render_params *p, const void *rays_dev, uint32_t n, void *out_dev, hipStream_t stream);
int trace_launch(const rt_scene *s, const void *rays_dev, uint32_t n, bool any, void *out_dev, hipStream_t stream);

// The host form of a side unit (rt_denoise, rt_firefly, rt_temporal): one device buffer that
// lives for the call, carved into regions of floats in the order they are declared (an int32
// count takes a float's room), filled and read back by synchronous copies on the null stream,
// and two events around the launches, which alone elapsed() reports.
struct Staging {
    DevBuf buf;
    Events<2> ev;
    rtnw::Regions plan;
    rtnw::Region floats(size_t n) { return plan.add(n); }
    int reserve() { return buf.reserve(plan.total * sizeof(float)); }   // once, after the last region
    float *ptr(rtnw::Region r) const { return (float *)buf.p + r.at; }
    float *ptr_if(const void *wanted, rtnw::Region r) const { return wanted ? ptr(r) : nullptr; }
    int upload(rtnw::Region r, const void *src) {   // a null input is not there: skipped
        if (src) HIP_TRY(hipMemcpy(ptr(r), src, r.n * sizeof(float), hipMemcpyHostToDevice));
        return RT_OK;
    }
    int download(void *dst, rtnw::Region r) {   // a null output is not wanted: skipped
        if (dst) HIP_TRY(hipMemcpy(dst, ptr(r), r.n * sizeof(float), hipMemcpyDeviceToHost));
        return RT_OK;
    }
    int begin() {
        HIP_TRY(hipEventCreate(&ev[0]));
        HIP_TRY(hipEventCreate(&ev[1]));
        HIP_TRY(hipEventRecord(ev[0], nullptr));
        return RT_OK;
    }
    int end() { HIP_TRY(hipEventRecord(ev[1], nullptr)); return RT_OK; }
    int elapsed(double *ms) {   // after a download: the events have completed
        float t = 0.f;
        if (ms) HIP_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
        if (ms) *ms = (double)t;
        return RT_OK;
    }
};

// The argument checks the side units share, each at its place in its function's order; `f` is
// the entry point's name.  RT_OK, or the error with the message set.
inline int image_size_check(const std::string &f, int nx, int ny) {
    if (nx < 1 || ny < 1 || (uint64_t)nx * (uint64_t)ny > 0x7FFFFFFFull)
        return fail(RT_ERR_INVALID, f + ": nx and ny must be at least 1 (and nx * ny below 2^31)");
    return RT_OK;
}
inline int ray_count_check(const std::string &f, int64_t n, bool *empty) {   // *empty: n == 0, nothing to do
    *empty = n == 0;
    if (!rtnw::ray_count_ok(n)) return fail(RT_ERR_INVALID, f + ": n must be in 0..2^31 - 1");
    return RT_OK;
}
inline int scene_check(const std::string &f, const rt_scene *s) {
    if (!s) return fail(RT_ERR_INVALID, f + ": null scene");
    if (s->bvh_width != 2) return fail(RT_ERR_UNSUPPORTED, f + " needs a scene with a 2-wide BVH (RTNW_BVH_WIDTH=2)");
    return RT_OK;
}
inline int unit_missing(const std::string &f, const char *unit, const char *object) {
    return fail(RT_ERR_UNSUPPORTED, f + ": this library was linked without the " + unit + " unit (" + object + ")");
}

// The host form of a ray query: n records of in_bytes each through the scene's workspace
// (a batch of records in, then its records out of out_bytes each), each batch copied in, launched
// by launch(in_dev, m, out_dev, stream) and copied out on the scene's stream; *ms, when asked
// for, is the launches' summed event time.  `knob` is the batch size's environment variable
// (rtnw::plan_trace_batch).  A record out depends on its record in alone, so not on the batches.
template <class Launch>
int ray_batches(rt_scene *s, const void *in, size_t in_bytes, void *out, size_t out_bytes, int64_t n, const char *knob,
                double *ms, Launch launch) {
    HIP_TRY(hipSetDevice(s->device));
    RT_TRY(ensure_own_stream(s));
    const uint64_t per = rtnw::plan_trace_batch((uint64_t)n, std::getenv(knob));
    RT_TRY(s->trace_ws.reserve((size_t)per * (in_bytes + out_bytes)));
    char *in_dev = (char *)s->trace_ws.p, *out_dev = in_dev + (size_t)per * in_bytes;
    Events<2> ev;
    HIP_TRY(hipEventCreate(&ev[0]));
    HIP_TRY(hipEventCreate(&ev[1]));
    double total = 0.0;
    for (uint64_t k0 = 0; k0 < (uint64_t)n; k0 += per) {
        const uint64_t m = std::min<uint64_t>(per, (uint64_t)n - k0);
        HIP_TRY(hipMemcpyAsync(in_dev, (const char *)in + (size_t)k0 * in_bytes, (size_t)m * in_bytes, hipMemcpyHostToDevice,
                               s->own_stream));
        HIP_TRY(hipEventRecord(ev[0], s->own_stream));
        RT_TRY(launch(in_dev, (uint32_t)m, out_dev, s->own_stream));
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

#pragma GCC visibility pop
