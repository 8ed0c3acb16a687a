// rt_firefly.h — launch interface of rt_firefly.hip: the guide-aware firefly clamp that runs
// ahead of the denoiser (capi_post.cpp rt_firefly, rt_firefly_dev).  Internal
// to librt_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_hip.h"

// One Jacobi pass over the nx x ny image: a pixel whose demodulated luminance exceeds
// k * (mean over its similar neighbours within fp->radius) + floor is scaled down to that bound.
// color: 3 floats per pixel; guides: the packed layout of rt_features.h; moments: 2 per pixel
// or null; out: 3 per pixel, not color; out_moments (2 per pixel, may be moments) and ratio
// (1 per pixel) may be null.  fp has passed capi_post.cpp's checks (radius 1..3).
extern "C" hipError_t rt_launch_firefly(int nx, int ny, const float *color, const float *guides, const float *moments,
                                        const rt_firefly_params *fp, float *out, float *out_moments, float *ratio,
                                        hipStream_t stream);

// capi_post.cpp reaches the launcher through this table, filled by rt_firefly.hip's static
// initialiser when the unit is linked in (like rt_denoise.h's RtDenoiseLaunch).
struct RtFireflyLaunch {
    decltype(&rt_launch_firefly) clamp;
};
extern "C" RtFireflyLaunch rt_firefly_launch;   // defined (empty) in capi_post.cpp
