// rt_temporal.h — launch interface of rt_temporal.hip: the reprojected frame history that runs
// ahead of the denoiser (capi_temporal.cpp rt_temporal, rt_temporal_dev).
// Internal to librt_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_hip.h"

// How a pixel finds its history: none (a first frame: the frame is copied), its own pixel (the
// two cameras are bytewise equal), or the four taps around its reprojected surface point.
enum { RT_TEMPORAL_FIRST = 0, RT_TEMPORAL_STATIC = 1, RT_TEMPORAL_REPROJECT = 2 };

// One Jacobi pass over the nx x ny image.  The frames hold device pointers and have passed
// capi_temporal.cpp's checks: cur (color, guides; moments or null), hist (color, guides, len;
// moments as cur's; unread in mode RT_TEMPORAL_FIRST and may then be all null), out (color, len;
// moments or null, only with cur's).  out's arrays are written; none of them is one of hist's,
// and out->color is not cur->color.
extern "C" hipError_t rt_launch_temporal(int nx, int ny, int mode, const rt_temporal_frame *cur,
                                         const rt_camera_desc *cam, const rt_temporal_frame *hist,
                                         const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                                         const rt_temporal_frame *out, hipStream_t stream);

// The half-width of the clamp's window is at most this (rt_temporal_clamp_params.radius): the
// clamped kernel's LDS tile is sized by it.
#define RT_TEMPORAL_CLAMP_MAX_RADIUS 3

// rt_launch_temporal with the history colour clipped to the colour box of the current frame's
// neighbourhood (rt_temporal_clamped).  Only mode RT_TEMPORAL_REPROJECT with
// cp->radius >= 1 runs the clamped kernel (rt_temporal_clamps); every other case runs
// rt_launch_temporal's and leaves `clipped` alone: the caller zeroes it then, outside what it
// times.  `clipped` (device, nx * ny, or null; none of the frames' arrays) receives the mask of the
// channels the clamp moved.  cp has passed capi_temporal.cpp's checks.
inline bool rt_temporal_clamps(int mode, const rt_temporal_clamp_params *cp) {
    return mode == RT_TEMPORAL_REPROJECT && cp->radius >= 1;
}
extern "C" hipError_t rt_launch_temporal_clamped(int nx, int ny, int mode, const rt_temporal_frame *cur,
                                                 const rt_camera_desc *cam, const rt_temporal_frame *hist,
                                                 const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                                                 const rt_temporal_clamp_params *cp, const rt_temporal_frame *out,
                                                 int32_t *clipped, hipStream_t stream);

// rt_launch_temporal_clamped with a history for background and edge pixels (rt_temporal_cover;
// DESIGN.md §7k).  Mode RT_TEMPORAL_REPROJECT runs the cover kernel at any radius in 0..3, which
// writes `clipped` and `source` (device, nx * ny each, or null; buffers of their own) itself;
// every other mode runs rt_launch_temporal's and leaves both alone: the caller fills them then,
// outside what it times (zeros, and under equal cameras rt_launch_temporal_same for `source`).
// cp and vp have passed capi_temporal.cpp's checks.
extern "C" hipError_t rt_launch_temporal_cover(int nx, int ny, int mode, const rt_temporal_frame *cur,
                                               const rt_camera_desc *cam, const rt_temporal_frame *hist,
                                               const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                                               const rt_temporal_clamp_params *cp, const rt_temporal_cover_params *vp,
                                               const rt_temporal_frame *out, int32_t *clipped, int32_t *source,
                                               hipStream_t stream);
// source[p] = RT_TEMPORAL_SRC_SAME where mode RT_TEMPORAL_STATIC uses the history of pixel p
// (min(hist_len[p], max_history) > 0), else 0.
extern "C" hipError_t rt_launch_temporal_same(int nx, int ny, const int32_t *hist_len, int max_history, int32_t *source,
                                              hipStream_t stream);

// capi_temporal.cpp reaches the launchers through this table, filled by rt_temporal.hip's static
// initialiser when the unit is linked in (like rt_firefly.h's RtFireflyLaunch).
struct RtTemporalLaunch {
    decltype(&rt_launch_temporal) accumulate;
    decltype(&rt_launch_temporal_clamped) accumulate_clamped;
    decltype(&rt_launch_temporal_cover) accumulate_cover;
    decltype(&rt_launch_temporal_same) mark_same;
};
extern "C" RtTemporalLaunch rt_temporal_launch;   // defined (empty) in capi_temporal.cpp
