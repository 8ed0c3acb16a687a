// rt_lens.h — launch interface of rt_lens.hip: the device-side ray generator of the lens
// renders (perspective, orthographic, fisheye, equirectangular) and their in-order resolve
// (capi_lens.cpp rt_lens_rays, rt_render_lens and their _dev forms).
// Internal to librt_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernel.h"

// What the generator reads beside RtKernelArgs' camera and image part (fill_camera_args):
// the model, the camera's w, and the fisheye's angle per unit radius, fov_deg * float(pi / 360)
// as one float32 product.
struct RtLensArgs {
    int model;        // RT_LENS_*
    float cw[3];
    float fov_k;
};

// One lane per (pixel, sample) of a batch: pixels [p0, p0 + np) of the w-wide rectangle at
// (x0, y0), counted row-major from its top-left corner, times samples [a->sample_offset,
// a->sample_offset + ns).  Record (s, p) goes to rays[s * stride + p] (rt_path_ray; stride >= np
// records between sample planes) and, when trace_rays is non-null, to trace_rays[s * stride + p]
// (rt_ray: t_min = a->tmin, t_max = +inf).  Read from a: org, llc, hor, ver, cu, cv, lens, ct0,
// ct1, nx, ny, rnx, rny, tmin, seed, sample_offset.  np * ns < 2^31.
extern "C" hipError_t rt_launch_lens_generate(const RtKernelArgs *a, const RtLensArgs *l, int x0, int y0, int w, uint32_t p0,
                                              uint32_t np, int ns, uint64_t stride, void *rays, void *trace_rays,
                                              hipStream_t stream);

// One lane per pixel p < np: adds the batch's ns sample planes (radiance[s * np + p], rt_radiance;
// hits[s * np + p], rt_hit, when guides is non-null) in sample order, float32, to the pixel's
// sums: rgb[3 p ..], moments[2 p ..] (sum y, sum y * y, y = (r + g) + b; may be null) and
// guides[8 p ..] (albedo.rgb, coverage, normal.xyz, depth; may be null).  first: the sums start
// from 0, else from what the outputs hold; last: rgb and guides are multiplied by k.
extern "C" hipError_t rt_launch_lens_resolve(const void *radiance, const void *hits, uint32_t np, int ns, float k, int first,
                                             int last, float *rgb, float *moments, float *guides, hipStream_t stream);

// capi_lens.cpp reaches the launchers through this table, which rt_lens.hip's static
// initialiser fills when the unit is linked in (like rt_trace.h's RtTraceLaunch): a library
// linked without it returns RT_ERR_UNSUPPORTED from the lens entry points.
struct RtLensLaunch {
    decltype(&rt_launch_lens_generate) generate;
    decltype(&rt_launch_lens_resolve) resolve;
};
extern "C" RtLensLaunch rt_lens_launch;   // defined (empty) in capi_lens.cpp
