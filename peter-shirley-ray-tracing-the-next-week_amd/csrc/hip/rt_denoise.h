// rt_denoise.h — launch interface of rt_denoise.hip: the variance-guided edge-avoiding
// à-trous filter (capi_post.cpp rt_denoise, rt_denoise_dev).  Internal to
// librt_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Packs the filter's two planes, one float4 per pixel each: G = (normal.xyz, depth) and
// E = (colour / a', variance of the demodulated luminance's mean), a' = max(albedo, 0.01)
// per channel when `demodulate`, else 1.  color: 3 floats per pixel; guides: the packed
// layout of rt_features.h; moments: 2 per pixel or null (then E.w = 0 and no tap looks at
// it); spp: each pixel's sample count, or null for uniform_spp.
extern "C" hipError_t rt_launch_denoise_prepare(uint32_t npix, const float *color, const float *guides,
                                                const float *moments, const int32_t *spp, int uniform_spp,
                                                int demodulate, float4 *G, float4 *E, hipStream_t stream);

// One à-trous iteration with taps `step` pixels apart over the nx x ny planes: E_in -> E_out,
// or, when out_rgb is non-null (the last iteration), the filtered colour times a' (from
// guides, as above) to out_rgb, 3 floats per pixel.  use_var: the luminance weight is on
// (moments were present); variance_filter: with use_var, its denominator takes the 3 x 3
// Gaussian (1 2 1 / 4, direct neighbours, the centre for those outside the image) of E_in's
// variance in place of the centre's own.
extern "C" hipError_t rt_launch_denoise_atrous(int nx, int ny, int step, float sigma_color, float sigma_depth,
                                               int use_var, int variance_filter, const float4 *G, const float4 *E_in,
                                               float4 *E_out, const float *guides, int demodulate, float *out_rgb,
                                               hipStream_t stream);

// capi_post.cpp reaches the launchers through this table, filled by rt_denoise.hip's static
// initialiser when the unit is linked in (like rt_moments.h's RtMomentsLaunch).
struct RtDenoiseLaunch {
    decltype(&rt_launch_denoise_prepare) prepare;
    decltype(&rt_launch_denoise_atrous) atrous;
};
extern "C" RtDenoiseLaunch rt_denoise_launch;   // defined (empty) in capi_post.cpp
