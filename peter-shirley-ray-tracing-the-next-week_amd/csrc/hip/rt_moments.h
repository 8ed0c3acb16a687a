// rt_moments.h — launch interface of rt_moments.hip: the resolve that also keeps each
// pixel's moments, and the adaptive driver's select / test / guard / finish kernels (capi_adaptive.cpp
// rt_render_tiles_moments, rt_render_adaptive, rt_render_adaptive_guarded).  Internal to
// librt_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// rt_launch_resolve (rt_kernel.h) plus the moments of the work items' channel sums
// y = (r + g) + b: mom[2 * o] += y, mom[2 * o + 1] += y * y per slab item, in item order
// (o = out_index[p]).  Between sample batches the moments stay in `mom` itself; they start
// from zero with RT_RESOLVE_FIRST, from mom's contents with RT_RESOLVE_SUM_IN as well.
// slab_floats: rt_slab_floats().
extern "C" hipError_t rt_launch_resolve_moments(const float *slab, int slab_floats, uint32_t npix, int nchunks, float k,
                                                float4 *acc, int mode, const uint32_t *out_index, float *out, float *mom,
                                                hipStream_t stream);

// One convergence decision per pixel of the frame (npix pixels, slot order).  A pixel with
// active[i] != 0 has just received `added` samples: spp[i] += added, and with tol > 0 it
// leaves the active set (active[i] = 0) when, in FP64 with n = spp[i],
//   n * m2 - m1 * m1  <=  ((tol * tol) * (n - 1)) * ((m1 + floor * n) * (m1 + floor * n))
// (rt_hip.h rt_adaptive_params; a NaN compares false).  counters[0] += pixels still
// active, counters[1] += pixels that converged in this call.
extern "C" hipError_t rt_launch_adaptive_select(uint32_t npix, int added, float tol, float floor, const float *mom,
                                                int32_t *spp, uint8_t *active, uint32_t *counters, hipStream_t stream);

// rt_launch_adaptive_select's decision without the retirement (rt_render_adaptive_guarded):
// spp[i] += added for the active pixels, as there, and for every pixel of the frame
// fail[i] = active[i] != 0 and not converged.  `active` and the counters are not written.
extern "C" hipError_t rt_launch_adaptive_test(uint32_t npix, int added, float tol, float floor, const float *mom,
                                              int32_t *spp, const uint8_t *active, uint8_t *fail, hipStream_t stream);

// The neighbourhood guard over a w x h frame in slot order (y * w + x), r in 0..8: an active
// pixel (x, y) leaves the active set (active = 0) iff no pixel (qx, qy) of the frame with
// |qx - x| <= r and |qy - y| <= r has fail != 0.  counters[0] += pixels still active,
// counters[1] += pixels retired in this call.  fail must be 0 wherever active is 0.
extern "C" hipError_t rt_launch_adaptive_guard(int w, int h, int r, const uint8_t *fail, uint8_t *active,
                                               uint32_t *counters, hipStream_t stream);

// sums[3 * i + c] *= float(1.0 / double(float(spp[i]))): each pixel's mean over its own
// sample count (vec3.h:134-141, as rt_resolve's last batch does with the job's one count).
extern "C" hipError_t rt_launch_adaptive_finish(uint32_t npix, const int32_t *spp, float *sums, hipStream_t stream);

// The host reaches the launchers through this table, which rt_moments.hip's static
// initialiser fills when the unit is linked in (like rt_kernel.h's rt_fold_launch): the host
// objects still link against rt_kernel.o alone, and the moments / adaptive entry points of
// such a library return RT_ERR_UNSUPPORTED.
struct RtMomentsLaunch {
    decltype(&rt_launch_resolve_moments) resolve;
    decltype(&rt_launch_adaptive_select) select;
    decltype(&rt_launch_adaptive_finish) finish;
    decltype(&rt_launch_adaptive_test) test;
    decltype(&rt_launch_adaptive_guard) guard;
};
extern "C" RtMomentsLaunch rt_moments_launch;   // defined (empty) in capi_adaptive.cpp
