// rt_features.hip — first-hit feature buffers: per pixel the mean albedo, normal, depth and
// coverage of its camera samples' first surface hits, the guides of the denoiser
// (rt_denoise.hip).
//
//   rt_features           one lane per (pixel, sample): the camera ray the megakernel builds
//                         for that sample (the same key, jitter draws, lens-disk loop and time
//                         draw: rt_megakernel.h camera_begin / camera_finish; stated per lane
//                         in rt_camera.h, which rt_lens.hip shares), its closest
//                         surface hit under hitable_list's (t, key) rule, and the hit's
//                         material colour, world normal and distance into a slab.
//   rt_features_resolve   adds a pixel's samples in sample order (float32) and scales the
//                         sums by float(1.0 / n), as rt_resolve does with the radiance.
//
// Constant media are ignored: the features see through them to the surface behind (the
// subsurface ball's glass shell is final()'s first hit).  Compiled with -ffp-contract=off
// like the megakernel.
#include "rt_features.h"
#include "rt_device.h"
#include "rt_camera.h"
#include "rt_colour.h"

namespace {

__global__ __launch_bounds__(RT_BLOCK) void rt_features(const RtKernelArgs A, int x0, int y0, int w,
                                                        float4 *__restrict__ slab) {
    __shared__ uint32_t lds_stack[RT_BLOCK / 64][RT_STACK_DEPTH][64];   // [wave][depth][lane], as the megakernel's
    rtl_lds_init(threadIdx.x);   // rt_libm.h's sine constants (the checker and noise textures)
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t *stk = &lds_stack[wave][0][lane];
    const uint32_t gid = blockIdx.x * RT_BLOCK + threadIdx.x;
    const uint32_t total = A.npix * (uint32_t)A.ns;
    const bool valid = gid < total;   // the lanes past the end stay in the wave, idle
    const uint32_t it = valid ? gid : 0u;
    const uint32_t k = it / A.npix, p = it - k * A.npix;
    const int x = x0 + (int)(p % (uint32_t)w), j = A.ny - 1 - (y0 + (int)(p / (uint32_t)w));
    const Ray r = camera_ray(A, x, j, A.sample_offset + k, seed_key(A.seed));

    // closest surface hit (hitable_list.h:20-32)
    float best_t = RT_FLT_MAX;
    int best_key = 0x7FFFFFFF;
    uint32_t best_prim = RT_NO_PRIM;
    lane_closest_hit<false>(A, r, A.tmin, valid, stk, best_t, best_key, best_prim);

    const bool have = valid && best_prim != RT_NO_PRIM;
    V3 alb = mk(1.0f, 1.0f, 1.0f), nrm = mk(0, 0, 0);
    float depth = 0.f, cov = 0.f;
    if (have) {
        nrm = hit_guides(A, r, best_prim, best_t, alb, depth).n;
        cov = 1.0f;
    }
    if (valid) {
        slab[(size_t)gid * 2 + 0] = make_float4(alb.x, alb.y, alb.z, cov);
        slab[(size_t)gid * 2 + 1] = make_float4(nrm.x, nrm.y, nrm.z, depth);
    }
}

__global__ __launch_bounds__(256) void rt_features_resolve(const float4 *__restrict__ slab, uint32_t npix, int ns, float k,
                                                           int first, int last, float4 *__restrict__ guides) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), g = a;
    if (!first) { a = guides[(size_t)p * 2]; g = guides[(size_t)p * 2 + 1]; }
#pragma unroll 4
    for (int c = 0; c < ns; ++c) {   // the loads run ahead; the adds stay in sample order
        const float4 u = slab[((size_t)c * npix + p) * 2], v = slab[((size_t)c * npix + p) * 2 + 1];
        a.x = a.x + u.x; a.y = a.y + u.y; a.z = a.z + u.z; a.w = a.w + u.w;
        g.x = g.x + v.x; g.y = g.y + v.y; g.z = g.z + v.z; g.w = g.w + v.w;
    }
    if (last) {
        a.x = a.x * k; a.y = a.y * k; a.z = a.z * k; a.w = a.w * k;
        g.x = g.x * k; g.y = g.y * k; g.z = g.z * k; g.w = g.w * k;
    }
    guides[(size_t)p * 2] = a;
    guides[(size_t)p * 2 + 1] = g;
}

}  // namespace

extern "C" hipError_t rt_launch_features(const RtKernelArgs *a, int x0, int y0, int w, float *slab, hipStream_t stream) {
    const uint64_t total = (uint64_t)a->npix * (uint64_t)a->ns;
    if (total == 0) return hipSuccess;
    if (total >= 0x80000000ull || w <= 0 || a->bvh_width != 2) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((total + RT_BLOCK - 1) / RT_BLOCK);
    hipLaunchKernelGGL(rt_features, dim3(blocks), dim3(RT_BLOCK), 0, stream, *a, x0, y0, w, (float4 *)slab);
    return hipGetLastError();
}

extern "C" hipError_t rt_launch_features_resolve(const float *slab, uint32_t npix, int ns, float k, int first, int last,
                                                 float *guides, hipStream_t stream) {
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_features_resolve, dim3((npix + 255) / 256), dim3(256), 0, stream, (const float4 *)slab, npix, ns, k,
                       first, last, (float4 *)guides);
    return hipGetLastError();
}

// the unit announces its launchers to the host when it is linked in
static const bool features_unit_linked =
    (rt_features_launch = RtFeaturesLaunch{rt_launch_features, rt_launch_features_resolve}, true);
