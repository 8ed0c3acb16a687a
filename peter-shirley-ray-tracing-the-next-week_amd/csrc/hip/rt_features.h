// rt_features.h — launch interface of rt_features.hip: the first-hit feature pass
// (albedo, normal, depth, coverage per pixel; capi_post.cpp rt_render_features,
// rt_render_features_dev).  Internal to librt_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernel.h"

// Floats per pixel of the packed guide layout, two float4:
//   (albedo.r, albedo.g, albedo.b, coverage), (normal.x, normal.y, normal.z, depth)
#define RT_GUIDE_FLOATS 8

// One lane per (pixel, sample) of the w-wide rectangle at (x0, y0): sample a.sample_offset + k
// of job pixel p (row-major in the rectangle), k < a.ns, p < a.npix, writes its eight values
// to slab[(k * a.npix + p) * RT_GUIDE_FLOATS].  Uses the scene arrays, the camera, nx, ny, rnx,
// rny, tmin, seed, sample_offset, ns, npix, has_bvh, scan, nprims, nprescan and root of `a`;
// the scene's BVH must be 2-wide.  a.npix * a.ns < 2^31.
extern "C" hipError_t rt_launch_features(const RtKernelArgs *a, int x0, int y0, int w, float *slab, hipStream_t stream);

// Adds the slab's ns samples to each pixel's eight running sums in sample order (float32):
// from zero when `first`, else from guides' contents; when `last` the sums are written times
// k, else as they are.  guides: npix * RT_GUIDE_FLOATS floats.
extern "C" hipError_t rt_launch_features_resolve(const float *slab, uint32_t npix, int ns, float k, int first, int last,
                                                 float *guides, hipStream_t stream);

// capi_post.cpp reaches the launchers through this table, which rt_features.hip's static
// initialiser fills when the unit is linked in (like rt_moments.h's RtMomentsLaunch): a
// library linked without it returns RT_ERR_UNSUPPORTED from the feature entry points.
struct RtFeaturesLaunch {
    decltype(&rt_launch_features) sample;
    decltype(&rt_launch_features_resolve) resolve;
};
extern "C" RtFeaturesLaunch rt_features_launch;   // defined (empty) in capi_post.cpp
