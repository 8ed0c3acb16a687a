// empty_pixels.h — which pixels of a render job are provably empty (empty_pixels.cpp): no
// primary ray of the pixel can reach a surface primitive.  Host arithmetic only, no HIP, so
// that it runs, and is tested, without a GPU (tests/test_empty_pixels.py,
// tests/native/empty_sanitize.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "scene_lower.h"

#pragma GCC visibility push(hidden)
namespace rtnw {

// Whether the samples of a scene's empty pixels, seen through `cam`, may be finished at the
// work claim (rt_megakernel.h refill) as far as the scene and the camera decide it: a pinhole
// (lens_radius == 0: the ray's origin and direction do not depend on the lens-disk draw), no
// -0.0f origin component (org + (+-0) keeps its sign only then), every medium bounded by one
// plain sphere (the only boundary code refill carries; such a boundary does not move, so the
// ray's time, drawn after the disk, is not needed either), a scene that runs the kernel's
// width-2 media variant (no instance chain, (u, v) material, checker or pre-scan: the only
// variant with refill's code) and a camera whose three edge vectors span space.
// RTNW_EMPTY_FAST=0 turns it off.  The render's own conditions (t_min >= 0,
// chunk == 1, no right fold, a tile job) are render_job's (capi_render.cpp).
bool empty_fast_scene_ok(const SceneInfo &s, const rt_camera_desc *cam);

// ... and as far as the render decides it: no hit before the origin (t_min >= 0), one sample per
// work item (the item is then the sample), not the right fold, a tile job (not a job with
// explicit output slots).
bool empty_fast_render_ok(float t_min, int chunk, int flags, bool tile_job);

// One bit per job pixel (bit k & 31 of word k >> 5, job pixel k = image pixel xy[k], x | y << 16):
// set when no primary ray of the pixel can hit a surface primitive.  *nflagged: the bits set.
// Returns false, with no bit set, when it cannot tell (a degenerate camera, a job whose pixels
// lie too far apart for the map).
bool empty_pixel_bits(const SceneInfo &s, const rt_camera_desc *cam, int nx, int ny, const uint32_t *xy, size_t n,
                      std::vector<uint32_t> *bits, size_t *nflagged);

}  // namespace rtnw
#pragma GCC visibility pop

// Diagnostics, exported from the library but not part of rt_hip.h (empty_pixels.cpp; the prototype
// tests/test_empty_pixels.py binds): lowers `d` and classifies the w x h rectangle at (x0, y0)
// of an nx x ny frame seen through `cam`; flags[yy * w + xx] = 1 for an empty pixel.  *on (may
// be null): whether a tile render with t_min, chunk and flags would use the bits
// (empty_fast_scene_ok and empty_fast_render_ok).  Returns the number flagged (the classifier
// answers whether or not the feature is on; 0 where it cannot tell), or a negative error code.
// No HIP call.
extern "C" long rt_scene_desc_empty_pixels(const rt_scene_desc *d, const rt_camera_desc *cam, int nx, int ny, int x0, int y0,
                                           int w, int h, float t_min, int chunk, int flags, uint8_t *flags_out, int *on);
