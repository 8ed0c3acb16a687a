// tests/native/host_sanitize.cpp — drives the host side of librt_hip.so (scene
// builders, flattening, every BVH form, the PNG decoder, the C ABI's host-only
// helpers and its error paths, and the lowering of every built-in scene to the image of the
// device's arrays, whose invariants are checked here, and the job arithmetic of job_plan.cpp:
// pixel orders, sample batches and claim sizes, as properties, up to the ABI's limits: tiles at the
// far corner of a 65535 x 65535 frame, jobs that end at sample index 0xFFFFFFFE, the rank
// split's largest block) in a build whose host objects carry
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_sanitizers.py; the
// device code object is linked in unsanitised, as the GPU sanitizer is not
// available).  Exit 0 = every call returned as expected and no sanitizer fired.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include <unistd.h>

#include "rt_hip.h"
#include "../rt_layout.h"
#include "bvh.h"
#include "rtnw.h"
#include "scene_lower.h"
#include "job_plan.h"

namespace {

int failures = 0;
#define EXPECT(c)                                                          \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::printf("FAIL %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, rt_last_error()); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

// rtnw::lower_scene under the knobs set by the caller: what the kernel relies on in the image.
void lowering(const char *name, const rt_scene_desc *d) {
    const int before = failures;
    rtnw::LoweredScene L;
    EXPECT(rtnw::validate_desc(d) == RT_OK);
    EXPECT(rtnw::lower_scene(d, &L) == RT_OK);
    if (L.image.empty()) { EXPECT(!"empty image"); return; }
    const size_t node_bytes = L.bvh_width == 4 ? sizeof(rt_dnode4) : L.bvh_width == 8 ? sizeof(rt_dnode8)
                            : L.bvh_width == RT_BVH_CW8 ? sizeof(rt_dnode8q) : sizeof(rt_dnode2);
    const size_t nstaged = (size_t)L.nprims + (L.scan ? 0 : (size_t)L.cell_n);
    // the arrays in the order they are staged: offset, bytes (0: empty, a sentinel)
    const struct { const char *what; size_t off, bytes; } arr[] = {
        {"nodes", L.nodes, (size_t)L.nnodes * node_bytes},
        {"prims", L.prims, nstaged * sizeof(rt_dprim)},
        {"bprims", L.bprims, (size_t)d->nboundary * sizeof(rt_dprim)},
        {"media", L.media, (size_t)d->nmedia * sizeof(rt_dmedium)},
        {"mats", L.mats, (size_t)d->nmaterials * sizeof(rt_dmaterial)},
        {"texs", L.texs, (size_t)d->ntextures * sizeof(rt_dtexture)},
        {"insts", L.insts, (size_t)d->ninstances * sizeof(rt_dinstance)},
        {"groups", L.groups, (size_t)L.ngroups * sizeof(rt_dgroup)},
        {"ranvec", L.ranvec, 256 * 4 * sizeof(float)},
        {"perm", L.perm, 768 * sizeof(int32_t)},
        {"texels", L.texels, d->nimages > 0 ? (size_t)d->image_bytes : 0},
    };
    const size_t n = sizeof arr / sizeof arr[0];
    int sentinels = 0;
    for (size_t i = 0; i < n; i++) {
        // 256-B aligned, inside the image, and up to the next array (the image's end for the last)
        const size_t end = i + 1 < n ? arr[i + 1].off : L.image.size(), bytes = arr[i].bytes ? arr[i].bytes : 256;
        EXPECT(arr[i].off % 256 == 0 && arr[i].off < L.image.size());
        EXPECT(arr[i].off + bytes <= end && end <= L.image.size());
        EXPECT(i + 1 == n ? end == arr[i].off + bytes : end == ((arr[i].off + bytes + 255) & ~(size_t)255));
        if (failures != before) { std::printf("  (%s: %s)\n", name, arr[i].what); return; }
        if (arr[i].bytes) continue;
        sentinels++;   // an empty array: one zeroed 256-B block
        for (size_t b = 0; b < 256; b++) EXPECT(L.image[arr[i].off + b] == 0);
    }
    EXPECT(L.nprims == d->nprims && L.has_bvh == (d->nprims > 0));
    // the order words over [0, nprims): a permutation of the input indices, the pre-scanned first, ascending
    std::vector<rt_dprim> prims(nstaged);
    if (nstaged) std::memcpy(prims.data(), L.image.data() + L.prims, nstaged * sizeof(rt_dprim));
    std::vector<char> seen(L.nprims, 0);
    for (int i = 0; i < L.nprims; i++) {
        const int o = prims[i].m[3];
        EXPECT(o >= 0 && o < L.nprims && !seen[o]);
        if (o >= 0 && o < L.nprims) seen[o] = 1;
    }
    EXPECT(L.nprescan >= 0 && L.nprescan <= RT_PRESCAN_MAX && L.nprescan <= L.nprims);
    for (int i = 1; i < L.nprescan && i < L.nprims; i++) EXPECT(prims[i - 1].m[3] < prims[i].m[3]);
    // the medium cell's copies follow, each naming an input primitive
    EXPECT(L.cell_n >= 0 && L.cell_n <= RT_CELL_MAX);
    if (!L.scan && L.cell_n) EXPECT(L.cell_first == L.nprims);
    for (size_t i = L.nprims; i < nstaged; i++) EXPECT(prims[i].m[3] >= 0 && prims[i].m[3] < L.nprims);
    if (L.scan) {
        EXPECT(L.nprescan == 0 && L.cell_n == 0 && L.ngroups >= 1);
        int total = 0;
        for (int g = 0; g < L.ngroups; g++) {
            rt_dgroup grp;
            std::memcpy(&grp, L.image.data() + L.groups + g * sizeof grp, sizeof grp);
            EXPECT(grp.first == total && grp.count > 0);
            total += grp.count;
        }
        EXPECT(total == L.nprims);
    } else {
        EXPECT(L.ngroups == 0);
    }
    if (!std::strcmp(name, "edge_empty")) {   // nothing but sentinels and the Perlin tables
        EXPECT(L.has_bvh == 0 && L.nprims == 0 && !L.scan && L.cell_n == 0);
        EXPECT(sentinels == (int)n - 2 - (d->nmaterials > 0) - (d->ntextures > 0));
    }
}

void scenes() {
    const char *names[] = {"final", "random_scene", "cornell_box", "cornell_smoke", "random_motion", "simple_light",
                           "two_spheres", "test", "earth", "edge_empty", "edge_single", "edge_degenerate"};
    for (const char *nm : names) {
        rt_scene_desc *d = nullptr;
        EXPECT(rt_builtin_scene_desc(nm, &d) == RT_OK);
        if (!d) continue;
        std::vector<char> buf(1 << 20);
        const int64_t need = rt_scene_desc_dump(d, buf.data(), (int64_t)buf.size());
        EXPECT(need > 0 || d->nprims == 0);
        EXPECT(rt_scene_desc_dump(d, buf.data(), 16) == need);   // truncated: same length, no overrun
        for (const char *w : {"2", "4", "8", "8q"}) {
            setenv("RTNW_BVH_WIDTH", w, 1);
            const rtnw::BvhResult r = rtnw::build_bvh(d->prims, d->nprims, d->instances, d->time0, d->time1);
            EXPECT((int)r.order.size() == d->nprims);
            lowering(nm, d);
            if (w[0] == '2' && !w[1])
                for (const char *knob : {"RTNW_SCAN", "RTNW_PRESCAN", "RTNW_CELL"}) {
                    setenv(knob, "0", 1);
                    lowering(nm, d);
                    unsetenv(knob);
                }
        }
        unsetenv("RTNW_BVH_WIDTH");
        // no GPU in the sanitizer run: the upload must fail cleanly (RT_ERR_HIP), not crash
        rt_scene *s = nullptr;
        const int rc = rt_scene_create(d, 0, &s);
        EXPECT(rc == RT_OK || rc == RT_ERR_HIP);
        if (s) rt_scene_destroy(s);
        rt_scene_desc_free(d);
    }
    rt_scene_desc *d = nullptr;
    EXPECT(rt_builtin_scene_desc("no_such_scene", &d) == RT_ERR_INVALID);
    EXPECT(rt_builtin_scene_desc(nullptr, &d) == RT_ERR_INVALID);
}

void png(const char *path) {
    std::ifstream f(path, std::ios::binary);
    std::vector<unsigned char> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    EXPECT(!file.empty());
    int x = 0, y = 0, comp = 0;
    std::string err;
    unsigned char *img = rtnw::png_decode(file.data(), file.size(), &x, &y, &comp, &err);
    EXPECT(img != nullptr && x > 0 && y > 0 && comp >= 3);
    std::free(img);
    // every truncation and single-byte corruptions must fail (or decode) without a fault
    for (size_t n = 0; n < file.size(); n += 1 + n / 8) {
        unsigned char *p = rtnw::png_decode(file.data(), n, &x, &y, &comp, &err);
        std::free(p);
    }
    std::vector<unsigned char> bad = file;
    for (size_t i = 8; i < bad.size(); i += 97) {
        const unsigned char keep = bad[i];
        bad[i] ^= 0x5A;
        unsigned char *p = rtnw::png_decode(bad.data(), bad.size(), &x, &y, &comp, &err);
        std::free(p);
        bad[i] = keep;
    }
}

void abi_helpers() {
    rt_camera_desc cam;
    const float from[3] = {478, 278, -600}, at[3] = {278, 278, 0}, up[3] = {0, 1, 0};
    EXPECT(rt_camera_init(&cam, from, at, up, 40, 1.0f, 0.0f, 10.0f, 0.0f, 1.0f) == RT_OK);
    const int nx = 37, ny = 23;
    std::vector<float> mean(3 * nx * ny);
    for (size_t i = 0; i < mean.size(); i++) mean[i] = (float)std::fmod(i * 0.37, 1.7) - 0.2f;
    mean[5] = NAN;
    mean[7] = INFINITY;
    std::vector<uint8_t> rgb(3 * nx * ny);
    rt_quantize(mean.data(), nx * ny, rgb.data());
    const int64_t need = rt_ppm_text(rgb.data(), nx, ny, nullptr, 0);
    std::vector<char> text(need + 1);
    EXPECT(rt_ppm_text(rgb.data(), nx, ny, text.data(), (int64_t)text.size()) == need);
    EXPECT(rt_ppm_text(rgb.data(), nx, ny, text.data(), 10) == need);
    // pixel interleave + unpack for every world size up to 8
    for (int world = 1; world <= 8; world++) {
        std::vector<float> image(3 * nx * ny, -1.0f);
        int64_t total = 0;
        for (int r = 0; r < world; r++) {
            const int64_t n = rt_rank_pixels(nx, ny, r, world, nullptr, 0);
            std::vector<int32_t> tiles(4 * n);
            EXPECT(rt_rank_pixels(nx, ny, r, world, tiles.data(), n) == n);
            std::vector<float> packed(3 * n, (float)r);
            EXPECT(rt_unpack_tiles(packed.data(), tiles.data(), n, nx, ny, image.data()) == RT_OK);
            total += n;
        }
        EXPECT(total == (int64_t)nx * ny);
        for (float v : image) EXPECT(v >= 0.0f);
    }
    // checkpoint round trip and the damaged-file paths
    char path[] = "/tmp/rt_sanitize_ckpt_XXXXXX";
    const int fd = mkstemp(path);
    EXPECT(fd >= 0);
    if (fd >= 0) close(fd);
    rt_checkpoint h{};
    h.nx = nx; h.ny = ny; h.samples_done = 7; h.max_depth = 50; h.t_min = 0.001f; h.seed = 99; h.count = mean.size();
    EXPECT(rt_checkpoint_write(path, &h, mean.data()) == RT_OK);
    rt_checkpoint g{};
    std::vector<float> back(mean.size());
    EXPECT(rt_checkpoint_read(path, &g, back.data(), back.size()) == RT_OK);
    EXPECT(std::memcmp(back.data(), mean.data(), back.size() * 4) == 0);
    EXPECT(rt_checkpoint_read(path, &g, back.data(), 3) != RT_OK);   // capacity too small
    {
        std::fstream f(path, std::ios::in | std::ios::out | std::ios::binary);
        f.seekp(sizeof(rt_checkpoint) + 40);
        f.put('\x7f');
    }
    EXPECT(rt_checkpoint_read(path, &g, back.data(), back.size()) != RT_OK);   // checksum
    {
        std::ofstream f(path, std::ios::binary | std::ios::trunc);
        f.write("RTCK", 4);
    }
    EXPECT(rt_checkpoint_read(path, &g, nullptr, 0) != RT_OK);   // truncated header
    std::remove(path);
    EXPECT(rt_checkpoint_read("/nonexistent/dir/x.ckpt", &g, nullptr, 0) != RT_OK);
    EXPECT(rt_version() != nullptr);
}


// ---------------------------------------------------------------- job_plan.cpp
struct Tile { int x0, y0, w, h; };

// The undivided order's rule, per entry: the pixel of output index `o` (tile t, column xx, row
// yy) and its sort key (tile, band of 8 rows, column, row).
struct Where { size_t t; int xx, yy; };
Where where_of(const std::vector<Tile> &tiles, uint32_t o) {
    uint32_t base = 0;
    for (size_t t = 0; t < tiles.size(); t++) {
        const uint32_t n = (uint32_t)tiles[t].w * (uint32_t)tiles[t].h;
        if (o - base < n) return {t, (int)((o - base) % (uint32_t)tiles[t].w), (int)((o - base) / (uint32_t)tiles[t].w)};
        base += n;
    }
    return {tiles.size(), 0, 0};
}

void tile_order(const std::vector<Tile> &tiles, int nx, int ny, const rtnw::DeepTest &deep) {
    std::vector<int32_t> flat;
    size_t total = 0;
    for (const Tile &t : tiles) {
        for (int v : {t.x0, t.y0, t.w, t.h}) flat.push_back(v);
        total += (size_t)t.w * t.h;
    }
    std::vector<uint32_t> xy, oi, dxy, doi;
    uint32_t nd0 = 7, nd = 7;
    EXPECT(rtnw::tile_job_order(flat.data(), (int)tiles.size(), nx, ny, rtnw::DeepTest(), &xy, &oi, &nd0) == RT_OK);
    EXPECT(xy.size() == total && oi.size() == total && nd0 == 0);
    if (xy.size() != total || oi.size() != total) return;
    // a permutation of the tiles' pixels, each entry naming its own pixel's place in the output
    std::vector<uint32_t> pos(total, UINT32_MAX);
    for (size_t k = 0; k < total; k++) {
        EXPECT(oi[k] < total && pos[oi[k]] == UINT32_MAX);
        if (oi[k] >= total) return;
        pos[oi[k]] = (uint32_t)k;
        const Where p = where_of(tiles, oi[k]);
        EXPECT(p.t < tiles.size() && xy[k] == ((uint32_t)(tiles[p.t].x0 + p.xx) | ((uint32_t)(tiles[p.t].y0 + p.yy) << 16)));
    }
    // tile after tile; in a tile band after band; a band of r rows is runs of r entries, each one
    // column with y ascending (r = 8 in a full band: runs start at multiples of 8)
    size_t k = 0;
    for (const Tile &t : tiles)
        for (int by = 0; by < t.h; by += 8) {
            const int r = std::min(8, t.h - by);
            for (int xx = 0; xx < t.w; xx++)
                for (int i = 0; i < r; i++, k++)
                    EXPECT((int)(xy[k] & 0xFFFFu) == t.x0 + xx && (int)(xy[k] >> 16) == t.y0 + by + i);
        }
    if (!deep) return;
    // deep pixels first, each group in the undivided list's order
    EXPECT(rtnw::tile_job_order(flat.data(), (int)tiles.size(), nx, ny, deep, &dxy, &doi, &nd) == RT_OK);
    EXPECT(dxy.size() == total && doi.size() == total);
    if (dxy.size() != total || doi.size() != total) return;
    size_t ndeep = 0;
    for (size_t i = 0; i < total; i++) ndeep += deep((int)(xy[i] & 0xFFFFu), (int)(xy[i] >> 16));
    EXPECT(nd == (ndeep == total ? 0 : ndeep));
    for (size_t i = 0; i < total; i++) {
        EXPECT(doi[i] < total);
        if (doi[i] >= total) return;
        EXPECT(dxy[i] == xy[pos[doi[i]]]);
        EXPECT(deep((int)(dxy[i] & 0xFFFFu), (int)(dxy[i] >> 16)) == (i < ndeep));
        if (i && i != ndeep) EXPECT(pos[doi[i - 1]] < pos[doi[i]]);
    }
}

void tile_orders() {
    const rtnw::DeepTest half = [](int x, int y) { return 2 * x + 3 * y < 40; };
    const rtnw::DeepTest all = [](int, int) { return true; };
    const int sizes[][2] = {{1, 1}, {8, 8}, {9, 7}, {500, 3}};
    for (const auto &sz : sizes)
        for (const rtnw::DeepTest &d : {rtnw::DeepTest(), half, all}) tile_order({{0, 0, sz[0], sz[1]}}, sz[0], sz[1], d);
    for (const rtnw::DeepTest &d : {rtnw::DeepTest(), half}) {
        tile_order({{3, 2, 5, 11}, {20, 9, 13, 10}}, 40, 24, d);
        tile_order({{65532, 65532, 3, 3}}, 65535, 65535, d);
    }
    tile_order({{65532, 65532, 3, 3}}, 65535, 65535, [](int x, int) { return x == 65534; });
    // 8 x 8 tiles in the corners and at the centre of the largest frame, packed in one job: the
    // coordinates round-trip through x | y << 16 (tile_order compares every entry with its tile's)
    const std::vector<Tile> far = {{65527, 65527, 8, 8}, {65527, 0, 8, 8}, {0, 65527, 8, 8}, {32764, 32763, 8, 8},
                                   {65534, 65534, 1, 1}};
    for (const rtnw::DeepTest &d : {rtnw::DeepTest(), rtnw::DeepTest([](int x, int y) { return ((x ^ y) & 1) != 0; })})
        tile_order(far, 65535, 65535, d);
    {
        std::vector<uint32_t> xy, oi;
        uint32_t nd = 0;
        const int32_t corner[4] = {65527, 65527, 8, 8};
        EXPECT(rtnw::tile_job_order(corner, 1, 65535, 65535, rtnw::DeepTest(), &xy, &oi, &nd) == RT_OK && xy.size() == 64);
        if (xy.size() == 64) {
            EXPECT(xy.front() == (65527u | (65527u << 16)) && xy.back() == (65534u | (65534u << 16)));
            EXPECT((int)(xy.back() & 0xFFFFu) == 65534 && (int)(xy.back() >> 16) == 65534);
        }
    }
    // final's own deep balls under the preset camera at 40 x 24, as prepare_job asks
    rt_scene_desc *d = nullptr;
    EXPECT(rt_builtin_scene_desc("final", &d) == RT_OK);
    rtnw::LoweredScene L;
    if (d) EXPECT(rtnw::lower_scene(d, &L) == RT_OK);
    EXPECT(!L.deep_balls.empty());
    rt_camera_desc cam;
    const float from[3] = {228, 278, -800}, at[3] = {278, 278, 0}, up[3] = {0, 1, 0};
    EXPECT(rt_camera_init(&cam, from, at, up, 40, 40.0f / 24.0f, 0.0f, 10.0f, 0.0f, 1.0f) == RT_OK);
    const rtnw::DeepTest real = [&](int x, int y) { return rtnw::deep_pixel(L, &cam, x, y, 40, 24); };
    int nreal = 0;
    for (int y = 0; y < 24; y++)
        for (int x = 0; x < 40; x++) nreal += real(x, y);
    EXPECT(nreal > 0 && nreal < 40 * 24);
    tile_order({{0, 0, 40, 24}}, 40, 24, real);
    tile_order({{0, 0, 17, 24}, {17, 0, 23, 24}}, 40, 24, real);
    if (d) rt_scene_desc_free(d);
    // tiles that are empty or leave the image
    std::vector<uint32_t> xy, oi;
    uint32_t nd = 0;
    const int32_t bad[][4] = {{0, 0, 0, 4}, {0, 0, 4, 0}, {-1, 0, 4, 4}, {0, -1, 4, 4}, {30, 0, 11, 4}, {0, 20, 4, 5},
                              {40, 0, 1, 1}, {1, 0, 2147483647, 1}, {2147483647, 0, 1, 1}};
    for (const auto &t : bad) EXPECT(rtnw::tile_job_order(t, 1, 40, 24, rtnw::DeepTest(), &xy, &oi, &nd) == RT_ERR_INVALID);
    const int32_t ok[4] = {0, 0, 4, 4};
    EXPECT(rtnw::tile_job_order(ok, 1, 65536, 24, rtnw::DeepTest(), &xy, &oi, &nd) == RT_ERR_INVALID);
    EXPECT(rtnw::tile_job_order(ok, 1, 40, 24, rtnw::DeepTest(), &xy, &oi, &nd) == RT_OK && xy.size() == 16);
}

// Where a frame's pixel comes in the adaptive sweep: (block row, block column, column, row).
uint64_t sweep_key(uint32_t slot, int w) {
    const uint32_t xx = slot % (uint32_t)w, yy = slot / (uint32_t)w;
    return ((uint64_t)(yy / 8) << 48) | ((uint64_t)(xx / 8) << 32) | ((uint64_t)xx << 16) | yy;
}

void active_orders() {
    const int frames[][2] = {{1, 1}, {8, 8}, {9, 17}, {40, 24}};
    // the frame's origin: near the image's, and so that the frame ends at pixel (65534, 65534)
    const int origins[][2] = {{5, 3}, {65527, 65527}};
    for (const auto &org : origins)
    for (const auto &fr : frames) {
        const int w = fr[0], h = fr[1], x0 = org[0], y0 = org[1];
        if (x0 + w > 65535 || y0 + h > 65535) continue;
        const uint32_t npix = (uint32_t)w * (uint32_t)h;
        std::vector<uint8_t> deep(npix);
        for (uint32_t o = 0; o < npix; o++) deep[o] = (o % (uint32_t)w) * 2 + (o / (uint32_t)w) < (uint32_t)w;
        for (int pattern = 0; pattern < 4; pattern++)
            for (int with_deep = 0; with_deep < 2; with_deep++) {
                std::vector<uint8_t> flags(npix);
                uint32_t lcg = 12345u + (uint32_t)pattern;
                uint32_t nactive = 0;
                for (uint32_t o = 0; o < npix; o++) {
                    lcg = lcg * 1664525u + 1013904223u;
                    flags[o] = pattern == 0 ? 1 : pattern == 1 ? 0 : pattern == 2 ? ((o % (uint32_t)w + o / (uint32_t)w) & 1) : (lcg >> 24) & 1;
                    nactive += flags[o];
                }
                rtnw::ActiveJobState st;   // reused over two passes, as a frame does
                if (with_deep) st.deep = deep;
                std::vector<uint32_t> xy(npix + 1, 0), slot(npix + 1, 0);
                for (int pass = 0; pass < 2; pass++) {
                    uint32_t nd = 99;
                    EXPECT(rtnw::active_job_order("t", flags.data(), x0, y0, w, h, nactive, &st, xy.data(), slot.data(), &nd) == RT_OK);
                    std::vector<char> seen(npix, 0);
                    uint32_t want_deep = 0;
                    for (uint32_t o = 0; o < npix; o++) want_deep += with_deep && flags[o] && deep[o];
                    EXPECT(nd == want_deep);
                    for (uint32_t k = 0; k < nactive; k++) {
                        const uint32_t o = slot[k];
                        EXPECT(o < npix && flags[o] && !seen[o]);
                        if (o >= npix) return;
                        seen[o] = 1;
                        EXPECT(xy[k] == ((uint32_t)(x0 + (int)(o % (uint32_t)w)) | ((uint32_t)(y0 + (int)(o / (uint32_t)w)) << 16)));
                        // as the kernel unpacks them
                        EXPECT((int)(xy[k] & 0xFFFFu) == x0 + (int)(o % (uint32_t)w) && (int)(xy[k] >> 16) == y0 + (int)(o / (uint32_t)w));
                        if (with_deep) EXPECT((deep[o] != 0) == (k < nd));
                        if (k && k != nd) EXPECT(sweep_key(slot[k - 1], w) < sweep_key(o, w));
                    }
                }
                // a count that is not the flags' own
                uint32_t nd = 0;
                EXPECT(rtnw::active_job_order("t", flags.data(), x0, y0, w, h, nactive + 1, &st, xy.data(), slot.data(), &nd) ==
                       RT_ERR_HIP);
                EXPECT(std::strstr(rt_last_error(), "disagree") != nullptr);
            }
    }
}

// rt_megakernel.h refill: claim k of a launch covers [base, end) — restated here.
void claim_range(const rtnw::BatchLaunch &l, uint64_t k, uint64_t *base, uint64_t *end) {
    const uint64_t big = std::min<uint64_t>(k, l.nbig);
    const uint64_t b64 = big * l.claim + (k - big) * l.claim_tail;
    *base = std::min<uint64_t>(b64, l.nitems);
    *end = std::min<uint64_t>(*base + (k < l.nbig ? l.claim : l.claim_tail), l.nitems);
}

void batch_checks(const rtnw::BatchPlan &pl, uint64_t b, uint64_t npix, int spp, int chunk, uint64_t waves, uint32_t ndeep,
                  int claim_x64, int tail_claims, uint64_t *s_end) {
    const uint32_t off = 1000u;
    const rtnw::BatchLaunch l = rtnw::plan_batch(pl, b, npix, spp, chunk, off, waves, ndeep, claim_x64, tail_claims);
    EXPECT(l.ns >= 1 && l.nchunks >= 1 && (uint64_t)l.nchunks <= pl.per);
    EXPECT(((uint64_t)l.ns + chunk - 1) / chunk == (uint64_t)l.nchunks);
    EXPECT(l.sample_offset == off + (uint32_t)(b * pl.per * (uint64_t)chunk));   // contiguous: where the previous ended
    if (s_end) {
        EXPECT(*s_end == b * pl.per * (uint64_t)chunk);
        *s_end += (uint64_t)l.ns;
    }
    const uint64_t nitems = npix * (uint64_t)l.nchunks;
    EXPECT(nitems <= 0xFFFFFFFFull - 64 && l.nitems == nitems);
    EXPECT(l.ndeep_items == (uint64_t)ndeep * (uint64_t)l.nchunks);
    if (claim_x64 < 0) EXPECT(l.claim >= 64 && l.claim <= 512 && l.claim % 64 == 0);
    else EXPECT(l.claim == (uint64_t)std::max(1, claim_x64) * 64);
    EXPECT(l.claim_tail == 64);
    // every item is in exactly one claim: the big claims end inside the launch, the tail claims
    // go on from there without a gap, and a 32-bit base + size does not wrap
    const uint64_t big_end = (uint64_t)l.nbig * l.claim;
    EXPECT(big_end <= nitems);
    const uint64_t ntail = (nitems - big_end + l.claim_tail - 1) / l.claim_tail;
    EXPECT(big_end + ntail * l.claim_tail >= nitems);
    EXPECT((uint64_t)l.nbig + ntail + 4096 * 2 < 0xFFFFFFFFull);   // the claim counter, with every wave's last look
    const uint64_t ks[] = {0, 1, l.nbig ? l.nbig - 1 : 0, l.nbig, l.nbig + 1, l.nbig + ntail - 1, l.nbig + ntail};
    for (uint64_t k : ks) {
        uint64_t b0, e0, b1, e1;
        claim_range(l, k, &b0, &e0);
        claim_range(l, k + 1, &b1, &e1);
        EXPECT(e0 == b1 || (b0 == nitems && b1 == nitems));
        EXPECT(b0 + std::max<uint32_t>(l.claim, l.claim_tail) <= 0xFFFFFFFFull || k >= l.nbig);
        EXPECT(b0 + l.claim_tail <= 0xFFFFFFFFull);
        if (k == 0) EXPECT(b0 == 0);
        EXPECT(k < l.nbig + ntail ? b0 < nitems : b0 == nitems);   // nbig + ntail claims, none empty
    }
}

void batch_plans() {
    const uint64_t npixs[] = {1, 63, 64, 65, 250000, 1000000, 65535ull * 65535ull, 0xFFFFFFFFull - 64, 0xFFFFFFFFull - 63};
    const int spps[] = {1, 2, 7, 1000, 2147483647}, chunks[] = {1, 2, 16, 2147483647};
    const uint64_t waves_[] = {1, 64, 4096};
    const int overrides[][2] = {{-1, -1}, {1, 0}, {8, 4}, {1000, -1}};
    for (uint64_t npix : npixs)
        for (int spp : spps)
            for (int chunk : chunks)
                for (uint64_t budget : {(uint64_t)1, (uint64_t)12, npix * 12 * 2, (uint64_t)16 << 30}) {
                    rtnw::BatchPlan pl{};
                    const int rc = rtnw::plan_batches(npix, spp, chunk, budget, 12, &pl);
                    if (npix > 0xFFFFFFFFull - 64) {
                        EXPECT(rc == RT_ERR_INVALID && std::strstr(rt_last_error(), "job too large") != nullptr);
                        continue;
                    }
                    EXPECT(rc == RT_OK);
                    EXPECT(pl.nchunks_total == ((uint64_t)spp + chunk - 1) / chunk);
                    EXPECT(pl.per >= 1 && pl.nbatches >= 1);
                    EXPECT(pl.nbatches * pl.per >= pl.nchunks_total && pl.nchunks_total > (pl.nbatches - 1) * pl.per);
                    EXPECT((pl.per - 1) * pl.nbatches < pl.nchunks_total);   // equalised: no smaller per does it in as many
                    EXPECT(npix * pl.per <= 0xFFFFFFFFull - 64);
                    // within the budget unless one chunk of every pixel is already over it
                    EXPECT(npix * pl.per * 12 <= budget || pl.per == 1);
                    const uint32_t ndeep = (uint32_t)(npix / 3);
                    for (uint64_t waves : waves_)
                        for (const auto &ov : overrides) {
                            if (pl.nbatches <= 64) {   // every batch: the samples add up
                                uint64_t s_end = 0;
                                for (uint64_t b = 0; b < pl.nbatches; b++)
                                    batch_checks(pl, b, npix, spp, chunk, waves, ndeep, ov[0], ov[1], &s_end);
                                EXPECT(s_end == (uint64_t)spp);
                            } else {                   // both ends and the middle; the offsets tie them together
                                for (uint64_t b : {(uint64_t)0, (uint64_t)1, pl.nbatches / 2, pl.nbatches - 2, pl.nbatches - 1})
                                    batch_checks(pl, b, npix, spp, chunk, waves, ndeep, ov[0], ov[1], nullptr);
                                const rtnw::BatchLaunch last =
                                    rtnw::plan_batch(pl, pl.nbatches - 1, npix, spp, chunk, 0, waves, ndeep, ov[0], ov[1]);
                                EXPECT((uint64_t)last.sample_offset + (uint64_t)last.ns == (uint64_t)spp);
                            }
                        }
                }
    // the feature pass: whole samples within the slab, fewer than 2^31 items per launch
    for (uint64_t npix : {(uint64_t)1, (uint64_t)65, (uint64_t)250000, (uint64_t)0x7FFFFFFF, (uint64_t)65535 * 65535})
        for (int spp : spps) {
            uint64_t per = 0;
            const int rc = rtnw::plan_feature_batches(npix, spp, 32, 256ull << 20, &per);
            if (npix > 0x7FFFFFFFull) { EXPECT(rc == RT_ERR_INVALID); continue; }
            EXPECT(rc == RT_OK && per >= 1 && per <= (uint64_t)spp && npix * per < 0x80000000ull);
            EXPECT(npix * per * 32 <= (256ull << 20) || per == 1);
        }
}

// The sample range's rule, every batch of a job that ends at the last legal index, and the rank
// split's block limit (include/rt_hip.h, rt_render_params and rt_rank_tiles).
void limits() {
    EXPECT(rtnw::sample_range_ok(0, 1) && rtnw::sample_range_ok(0, 2147483647) && rtnw::sample_range_ok(0xFFFFFFFEu, 1));
    EXPECT(rtnw::sample_range_ok(0xFFFFFFFFu - 2147483647u, 2147483647) && rtnw::sample_range_ok(0xFFFFFFF8u, 7));
    EXPECT(!rtnw::sample_range_ok(0xFFFFFFFFu, 1) && !rtnw::sample_range_ok(0xFFFFFFF9u, 7) && !rtnw::sample_range_ok(0xFFFFFFFEu, 7));
    EXPECT(!rtnw::sample_range_ok(0x80000001u, 2147483647) && !rtnw::sample_range_ok(0, 0) && !rtnw::sample_range_ok(5, -1));
    // a legal job that ends at index 0xFFFFFFFE: no batch starts below the job's offset (a wrapped
    // sum would) or ends past 0xFFFFFFFF, each starts where the one before ended, the last at the limit
    const uint64_t npixs[] = {1, 64, 65535, 65535ull * 65535ull};
    const int spps[] = {1, 7, 1000, 2147483647}, chunks[] = {1, 3, 2147483647};
    for (uint64_t npix : npixs)
        for (int spp : spps)
            for (int chunk : chunks)
                for (uint64_t budget : {(uint64_t)1, npix * 12 * 2, (uint64_t)16 << 30}) {
                    const uint32_t off = 0xFFFFFFFFu - (uint32_t)spp;
                    EXPECT(rtnw::sample_range_ok(off, spp));
                    rtnw::BatchPlan pl{};
                    EXPECT(rtnw::plan_batches(npix, spp, chunk, budget, 12, &pl) == RT_OK);
                    uint64_t want = off;
                    std::vector<uint64_t> bs;
                    if (pl.nbatches <= 64)
                        for (uint64_t b = 0; b < pl.nbatches; b++) bs.push_back(b);
                    else
                        bs = {0, 1, pl.nbatches / 2, pl.nbatches - 2, pl.nbatches - 1};
                    for (uint64_t b : bs) {
                        const rtnw::BatchLaunch l = rtnw::plan_batch(pl, b, npix, spp, chunk, off, 64, 0, -1, -1);
                        EXPECT(l.ns >= 1 && l.sample_offset >= off);
                        EXPECT((uint64_t)l.sample_offset + (uint64_t)l.ns <= 0xFFFFFFFFull);
                        EXPECT((uint64_t)l.sample_offset == (uint64_t)off + b * pl.per * (uint64_t)chunk);
                        if (pl.nbatches <= 64) {
                            EXPECT((uint64_t)l.sample_offset == want);
                            want += (uint64_t)l.ns;
                        }
                        if (b + 1 == pl.nbatches) EXPECT((uint64_t)l.sample_offset + (uint64_t)l.ns == 0xFFFFFFFFull);
                    }
                }
    // rt_rank_tiles: 65535 is the largest block (one block holds any frame); above it nx + block - 1
    // would overflow for INT_MAX: refused, for every layout
    for (int layout : {RT_LAYOUT_BLOCKS, RT_LAYOUT_INTERLEAVED, RT_LAYOUT_LATTICE}) {
        EXPECT(rt_rank_tiles(37, 23, 0, 1, layout, 65535, nullptr, 0) == 37 * 23);
        EXPECT(rt_rank_tiles(65535, 9, 1, 2, layout, 65535, nullptr, 0) == (layout == RT_LAYOUT_BLOCKS ? 0 : layout == RT_LAYOUT_LATTICE ? 0 : 32767 * 9));
        for (int block : {65536, 2147483647}) {
            EXPECT(rt_rank_tiles(37, 23, 0, 1, layout, block, nullptr, 0) == RT_ERR_INVALID);
            EXPECT(std::strstr(rt_last_error(), "block") != nullptr);
        }
        // the widest frame, two block rows: the ranks' pixels partition it
        const int nx = 65535, ny = 9, world = 3;
        std::vector<uint8_t> seen((size_t)nx * ny, 0);
        int64_t total = 0;
        for (int r = 0; r < world; r++) {
            const int64_t n = rt_rank_tiles(nx, ny, r, world, layout, 0, nullptr, 0);
            EXPECT(n >= 0);
            if (n < 0) continue;
            std::vector<int32_t> t((size_t)n * 4);
            EXPECT(rt_rank_tiles(nx, ny, r, world, layout, 0, t.data(), n) == n);
            for (int64_t k = 0; k < n; k++) {
                const int x = t[4 * k], y = t[4 * k + 1];
                EXPECT(x >= 0 && x < nx && y >= 0 && y < ny && t[4 * k + 2] == 1 && t[4 * k + 3] == 1);
                if (x >= 0 && x < nx && y >= 0 && y < ny) seen[(size_t)y * nx + x]++;
            }
            total += n;
        }
        EXPECT(total == (int64_t)nx * ny);
        size_t once = 0;
        for (uint8_t v : seen) once += v == 1;
        EXPECT(once == seen.size());
    }
}

// The side units' staging regions (job_plan.h Regions; capi_internal.h Staging): rt_temporal's ten,
// in its order and in floats, at the smallest and the largest image: each starts where the one
// before ended (no overlap, no gap) and the total is the sum, without wrapping in size_t.
void staging_regions() {
    for (size_t npix : {(size_t)1, (size_t)0x7FFFFFFF}) {
        const size_t per_pixel[10] = {8, 8, 3, 3, 3, 2, 2, 2, 1, 1};   // guides x 2, colour x 3, moments x 3, len x 2
        rtnw::Regions plan;
        size_t sum = 0;
        for (size_t k : per_pixel) {
            const rtnw::Region r = plan.add(npix * k);
            EXPECT(r.at == sum && r.n == npix * k);
            if (k == 8) EXPECT(r.at % 4 == 0);   // the guides are read by 16-B loads
            sum += r.n;
            EXPECT(plan.total == sum);
        }
        EXPECT(sum == npix * 33 && sum / 33 == npix && sum * sizeof(float) / sizeof(float) == sum);
    }
}

}  // namespace

int main(int argc, char **argv) {
    setvbuf(stdout, nullptr, _IONBF, 0);
    if (argc > 1) setenv("RTNW_EARTH_PNG", argv[1], 1);
    scenes();
    if (argc > 1) png(argv[1]);
    abi_helpers();
    tile_orders();
    active_orders();
    batch_plans();
    limits();
    staging_regions();
    std::printf(failures ? "FAILED %d\n" : "OK\n", failures);
    return failures ? 1 : 0;
}
