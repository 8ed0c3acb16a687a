// tests/native/empty_sanitize.cpp — drives the empty-pixel classifier (csrc/host/empty_pixels.cpp)
// over every built-in scene in a build whose objects carry AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_empty_sanitize.py).  Host code only: no HIP, no device
// code object.  Checked besides: the bit count, that a job's pixel order does not change a
// pixel's bit, that a tile at the far corner of a 65535 x 65535 frame is classified through a
// map of its own size, and that a job whose pixels lie too far apart for a map is declined.
// Exit 0 and a last line "OK" = every call returned as expected and no sanitizer fired.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "rt_hip.h"
#include "rtnw.h"
#include "scene_lower.h"
#include "empty_pixels.h"

// (the library's own is capi_util.cpp's, which needs the HIP runtime)
int rt_internal_fail(int code, const std::string &msg) {
    std::printf("error %d: %s\n", code, msg.c_str());
    return code;
}

namespace {

int failures = 0;
#define EXPECT(c)                                                  \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            failures++;                                            \
        }                                                          \
    } while (0)

size_t popcount(const std::vector<uint32_t> &bits) {
    size_t n = 0;
    for (uint32_t w : bits) n += (size_t)__builtin_popcount(w);
    return n;
}

std::vector<uint32_t> raster(int x0, int y0, int w, int h) {
    std::vector<uint32_t> xy;
    for (int yy = 0; yy < h; yy++)
        for (int xx = 0; xx < w; xx++) xy.push_back((uint32_t)(x0 + xx) | ((uint32_t)(y0 + yy) << 16));
    return xy;
}

void scene(const char *name) {
    float t0 = 0, t1 = 1;
    rtnw::hitable *world = rtnw::build_named_scene(name, &t0, &t1);
    EXPECT(world != nullptr);
    if (!world) return;
    std::unique_ptr<rtnw::flat_scene> fs = rtnw::flatten_world(world, t0, t1);
    rtnw::LoweredScene low;
    EXPECT(rtnw::validate_desc(&fs->desc) == RT_OK);
    EXPECT(rtnw::lower_scene(&fs->desc, &low) == RT_OK);
    EXPECT(low.surf_boxes.size() == (size_t)fs->desc.nprims * 6 && low.surf_spheres.size() == (size_t)fs->desc.nprims * 5);
    const struct { rtnw::vec3 from, at; float vfov; } views[] = {
        {rtnw::vec3(478, 278, -600), rtnw::vec3(278, 278, 0), 40.0f},
        {rtnw::vec3(13, 2, 3), rtnw::vec3(0, 0, 0), 20.0f},
        {rtnw::vec3(278, 50, 100), rtnw::vec3(278, 300, 400), 150.0f},
    };
    const int frames[][2] = {{64, 64}, {50, 37}, {500, 500}};
    for (const auto &v : views)
        for (const auto &f : frames) {
            const int nx = f[0], ny = f[1];
            const rtnw::camera c(v.from, v.at, rtnw::vec3(0, 1, 0), v.vfov, float(nx) / float(ny), 0.0f, 10.0f, 0.0f, 1.0f);
            const rt_camera_desc cam = c.desc();
            (void)rtnw::empty_fast_scene_ok(low, &cam);
            std::vector<uint32_t> xy = raster(0, 0, nx, ny), bits;
            size_t n = 0;
            const bool ok = rtnw::empty_pixel_bits(low, &cam, nx, ny, xy.data(), xy.size(), &bits, &n);
            EXPECT(ok);
            EXPECT(bits.size() == (xy.size() + 31) / 32 && popcount(bits) == n && n <= xy.size());
            if (nx != 50) continue;
            // the same pixels in another order (a stride that is coprime to their number), as a job of 1 x 1 tiles gives them
            std::vector<uint32_t> perm(xy.size()), pbits;
            for (size_t k = 0; k < xy.size(); k++) perm[k] = xy[(k * 7) % xy.size()];
            size_t pn = 0;
            EXPECT(rtnw::empty_pixel_bits(low, &cam, nx, ny, perm.data(), perm.size(), &pbits, &pn) && pn == n);
            for (size_t k = 0; k < xy.size() && pbits.size() == bits.size(); k++) {
                const size_t src = (k * 7) % xy.size();
                EXPECT(((pbits[k >> 5] >> (k & 31)) & 1u) == ((bits[src >> 5] >> (src & 31)) & 1u));
            }
        }
    // the far corner of the largest frame, and two pixels a frame apart
    const rtnw::camera c(views[0].from, views[0].at, rtnw::vec3(0, 1, 0), 40.0f, 1.0f, 0.0f, 10.0f, 0.0f, 1.0f);
    const rt_camera_desc cam = c.desc();
    std::vector<uint32_t> corner = raster(65535 - 13, 65535 - 9, 13, 9), bits;
    size_t n = 0;
    EXPECT(rtnw::empty_pixel_bits(low, &cam, 65535, 65535, corner.data(), corner.size(), &bits, &n) && n <= corner.size());
    const uint32_t apart[2] = {0u, 65534u | (65534u << 16)};
    EXPECT(!rtnw::empty_pixel_bits(low, &cam, 65535, 65535, apart, 2, &bits, &n) && n == 0 && popcount(bits) == 0);
    EXPECT(!rtnw::empty_pixel_bits(low, &cam, 64, 64, corner.data(), corner.size(), &bits, &n));   // pixels outside the frame
    EXPECT(!rtnw::empty_pixel_bits(low, &cam, 64, 64, corner.data(), 0, &bits, &n));
    // a camera whose edge vectors do not span space, and one that is not finite
    rt_camera_desc flat = cam;
    for (int k = 0; k < 3; k++) flat.vertical[k] = flat.horizontal[k];
    EXPECT(!rtnw::empty_fast_scene_ok(low, &flat));
    EXPECT(!rtnw::empty_pixel_bits(low, &flat, 64, 64, raster(0, 0, 8, 8).data(), 64, &bits, &n));
    rt_camera_desc inf = cam;
    inf.origin[1] = INFINITY;
    EXPECT(!rtnw::empty_fast_scene_ok(low, &inf));
    std::printf("%s: %d primitives, %d media: done\n", name, fs->desc.nprims, fs->desc.nmedia);
}

}  // namespace

int main() {
    for (const char *name : {"random_scene", "random_motion", "two_spheres", "edge_empty", "edge_single", "edge_degenerate",
                             "edge_chains", "simple_light", "test", "cornell_box", "cornell_smoke", "final"})
        scene(name);
    EXPECT(rtnw::empty_fast_render_ok(0.0f, 1, 0, true) && !rtnw::empty_fast_render_ok(-1.0f, 1, 0, true) &&
           !rtnw::empty_fast_render_ok(0.001f, 2, 0, true) && !rtnw::empty_fast_render_ok(0.001f, 1, RT_FLAG_RIGHT_FOLD, true) &&
           !rtnw::empty_fast_render_ok(0.001f, 1, 0, false) && !rtnw::empty_fast_render_ok(NAN, 1, 0, true));
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
