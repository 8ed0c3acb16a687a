// rt_trace.h — launch interface of rt_trace.hip: ray queries on caller-supplied rays
// (closest hit and occlusion; capi_trace.cpp rt_trace_rays, rt_occluded and their _dev forms;
// DESIGN.md §7f).  Internal to librt_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernel.h"

// The records of rt_hip.h (rt_ray, rt_hit) as the kernel moves them: three 16-B words each.
#define RT_RAY_BYTES 48
#define RT_HIT_BYTES 48

// One lane per ray k < n: rays[k] (rt_ray) against the scene arrays of `a` (nodes, prims,
// insts, mats, texs, texels, ranvec, perm, root, has_bvh, scan, nprims, nprescan; the BVH must
// be 2-wide).  any = 0: the closest hit under hitable_list's (t, list order) rule into hits[k]
// (rt_hit); any = 1: 0 / 1 / 255 into occ[k], the lane leaving at its first accepted hit.
// moving: the scene has moving spheres, whose boxes cover [time0, time1] only: a ray whose time
// lies outside is invalid.  n < 2^31.
extern "C" hipError_t rt_launch_trace(const RtKernelArgs *a, const void *rays, uint32_t n, int moving, float time0, float time1,
                                      int any, void *hits, uint8_t *occ, hipStream_t stream);

// capi_trace.cpp reaches the launcher through this table, which rt_trace.hip's static
// initialiser fills when the unit is linked in (like rt_features.h's RtFeaturesLaunch): a
// library linked without it returns RT_ERR_UNSUPPORTED from the ray-query entry points.
struct RtTraceLaunch {
    decltype(&rt_launch_trace) trace;
};
extern "C" RtTraceLaunch rt_trace_launch;   // defined (empty) in capi_trace.cpp
