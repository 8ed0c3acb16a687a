// capi_util.cpp — the part of the C ABI that needs no scene: the error message, device
// helpers, the math probe, the camera, quantize and PPM, checkpoints, built-in descriptors.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>

#include "capi_internal.h"
#include "rtnw.h"

static thread_local std::string g_err;

// shared with every other unit: sets the thread-local message rt_last_error() returns
int rt_internal_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

extern "C" {

const char *rt_last_error(void) { return g_err.c_str(); }
const char *rt_version(void) { return "rt_hip 1 (gfx950 persistent megakernel)"; }

int rt_device_count(int *out) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *out = 0; return hip_fail(e, "hipGetDeviceCount"); }
    *out = n;
    return RT_OK;
}

int rt_device_alloc(int device, uint64_t bytes, void **out) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc(out, bytes));
    return RT_OK;
}
int rt_device_free(void *ptr) {
    HIP_TRY(hipFree(ptr));
    return RT_OK;
}
int rt_copy_to_host(void *dst, const void *src, uint64_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}
int rt_copy_to_device(void *dst_dev, const void *src, uint64_t bytes) {
    HIP_TRY(hipMemcpy(dst_dev, src, bytes, hipMemcpyHostToDevice));
    return RT_OK;
}

int rt_math_probe(int fn, const float *a, const float *b, float *out, int64_t n) {
    if (fn < 0 || fn > 5 || n < 0 || n > (1 << 30) || (n && (!a || !out || (fn >= 4 && !b))))
        return fail(RT_ERR_INVALID, "rt_math_probe: bad arguments");
    if (n == 0) return RT_OK;
    const size_t bytes = (size_t)n * sizeof(float);
    DevBuf buf;
    if (int rc = buf.reserve(3 * bytes)) return rc;
    float *d = (float *)buf.p;
    hipError_t e = hipMemcpy(d, a, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && fn >= 4) e = hipMemcpy(d + n, b, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rt_launch_math_probe(fn, d, d + n, d + 2 * n, (int)n, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d + 2 * n, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "rt_math_probe");
    return RT_OK;
}

int rt_camera_init(rt_camera_desc *out, const float lookfrom[3], const float lookat[3], const float vup[3], float vfov,
                   float aspect, float aperture, float focus_dist, float t0, float t1) {
    if (!out || !lookfrom || !lookat || !vup) return fail(RT_ERR_INVALID, "rt_camera_init: null argument");
    rtnw::camera c(rtnw::vec3(lookfrom[0], lookfrom[1], lookfrom[2]), rtnw::vec3(lookat[0], lookat[1], lookat[2]),
                   rtnw::vec3(vup[0], vup[1], vup[2]), vfov, aspect, aperture, focus_dist, t0, t1);
    *out = c.desc();
    return RT_OK;
}

// ---------------------------------------------------------------- resolve
void rt_quantize(const float *mean, int64_t n, uint8_t *rgb) {   // main.cpp:316-325
    for (int64_t q = 0; q < n; q++) {
        for (int k = 0; k < 3; k++) {
            const float c = std::sqrt(mean[3 * q + k]);
            int iv = int(255.99 * c);
            iv = iv > 255 ? 255 : iv;
            rgb[3 * q + k] = (uint8_t)iv;
        }
    }
}

int64_t rt_ppm_text(const uint8_t *rgb, int nx, int ny, char *buf, int64_t cap) {   // main.cpp:297, 327-330
    std::string s = "P3\n" + std::to_string(nx) + " " + std::to_string(ny) + "\n255\n";
    for (int64_t q = 0; q < (int64_t)nx * ny; q++)
        s += std::to_string(rgb[3 * q]) + " " + std::to_string(rgb[3 * q + 1]) + " " + std::to_string(rgb[3 * q + 2]) + "\n";
    if (buf && cap >= (int64_t)s.size()) std::memcpy(buf, s.data(), s.size());
    return (int64_t)s.size();
}

// ------------------------------------------------ checkpoint / resume
// File = rt_checkpoint header, `count` floats (the per-pixel sums as rt_render_tiles
// packs them), FNV-1a 64 of those bytes.  Written to <path>.tmp, then renamed, so a
// crash leaves either the previous checkpoint or the new one, never a torn file (the
// reference's row-by-row PPM write, main.cpp:330, leaves a truncated image).
static uint64_t fnv1a(const void *p, size_t n) {
    const uint8_t *b = (const uint8_t *)p;
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}

int rt_checkpoint_write(const char *path, const rt_checkpoint *hdr, const float *sums) {
    if (!path || !hdr || (!sums && hdr->count)) return fail(RT_ERR_INVALID, "rt_checkpoint_write: null argument");
    rt_checkpoint h = *hdr;
    h.magic = RT_CHECKPOINT_MAGIC;
    h.version = RT_CHECKPOINT_VERSION;
    const std::string tmp = std::string(path) + ".tmp";
    FILE *f = std::fopen(tmp.c_str(), "wb");
    if (!f) return fail(RT_ERR_INVALID, std::string("cannot open ") + tmp);
    const size_t bytes = (size_t)h.count * sizeof(float);
    const uint64_t sum = fnv1a(sums, bytes);
    bool ok = std::fwrite(&h, sizeof h, 1, f) == 1 && (bytes == 0 || std::fwrite(sums, 1, bytes, f) == bytes) &&
              std::fwrite(&sum, sizeof sum, 1, f) == 1;
    ok = (std::fclose(f) == 0) && ok;
    if (!ok || std::rename(tmp.c_str(), path) != 0) {
        std::remove(tmp.c_str());
        return fail(RT_ERR_INVALID, std::string("cannot write checkpoint ") + path);
    }
    return RT_OK;
}

int rt_checkpoint_read(const char *path, rt_checkpoint *hdr, float *sums, uint64_t cap) {
    if (!path || !hdr) return fail(RT_ERR_INVALID, "rt_checkpoint_read: null argument");
    FILE *f = std::fopen(path, "rb");
    if (!f) return fail(RT_ERR_INVALID, std::string("cannot open ") + path);
    rt_checkpoint h;
    int rc = RT_OK;
    // the file's own size bounds `count` before anyone sizes a buffer by it: header +
    // count floats + the 8-byte checksum, and count = 3 x (pixels of a job <= nx x ny)
    long fsize = -1;
    if (std::fseek(f, 0, SEEK_END) == 0) fsize = std::ftell(f);
    std::rewind(f);
    if (std::fread(&h, sizeof h, 1, f) != 1 || h.magic != RT_CHECKPOINT_MAGIC || h.version != RT_CHECKPOINT_VERSION) {
        rc = fail(RT_ERR_INVALID, std::string("not a checkpoint: ") + path);
    } else if (h.nx <= 0 || h.ny <= 0 || h.count % 3 != 0 || h.count > 3ull * (uint64_t)h.nx * (uint64_t)h.ny ||
               fsize < (long)(sizeof h + sizeof(uint64_t)) ||
               // the payload's size by division: count * 4 would wrap for a crafted count
               ((uint64_t)fsize - sizeof h - sizeof(uint64_t)) % sizeof(float) != 0 ||
               ((uint64_t)fsize - sizeof h - sizeof(uint64_t)) / sizeof(float) != h.count) {
        rc = fail(RT_ERR_INVALID, std::string("corrupt checkpoint header (count / image size / file size): ") + path);
    } else if (sums) {   // sums == NULL: header only (to size the buffer)
        if (h.count > cap) {
            rc = fail(RT_ERR_INVALID, "checkpoint larger than the buffer");
        } else {
            const size_t bytes = (size_t)h.count * sizeof(float);
            uint64_t sum = 0;
            if ((bytes && std::fread(sums, 1, bytes, f) != bytes) || std::fread(&sum, sizeof sum, 1, f) != 1)
                rc = fail(RT_ERR_INVALID, std::string("truncated checkpoint: ") + path);
            else if (sum != fnv1a(sums, bytes))
                rc = fail(RT_ERR_INVALID, std::string("checkpoint checksum mismatch: ") + path);
        }
    }
    std::fclose(f);
    if (rc == RT_OK) *hdr = h;
    return rc;
}

// ------------------------------------------------------- host scene building
static std::mutex g_desc_mu;
static std::map<const rt_scene_desc *, std::unique_ptr<rtnw::flat_scene>> g_descs;

int rt_builtin_scene_desc(const char *name, rt_scene_desc **out) {
    if (!name || !out) return fail(RT_ERR_INVALID, "rt_builtin_scene_desc: null argument");
    std::lock_guard<std::mutex> lk(g_desc_mu);
    float t0, t1;
    rtnw::hitable *world = rtnw::build_named_scene(name, &t0, &t1);
    if (!world) return fail(RT_ERR_INVALID, std::string("unknown scene: ") + name);
    std::unique_ptr<rtnw::flat_scene> fs;
    try {
        fs = rtnw::flatten_world(world, t0, t1);
    } catch (const std::exception &ex) {
        return fail(RT_ERR_UNSUPPORTED, ex.what());
    }
    *out = &fs->desc;
    g_descs[&fs->desc] = std::move(fs);
    return RT_OK;
}

void rt_scene_desc_free(rt_scene_desc *d) {
    std::lock_guard<std::mutex> lk(g_desc_mu);
    g_descs.erase(d);
}

int64_t rt_scene_desc_dump(const rt_scene_desc *d, char *buf, int64_t cap) {
    if (!d) return fail(RT_ERR_INVALID, "null descriptor");
    const std::string s = rtnw::dump_desc(d);
    if (buf && cap >= (int64_t)s.size()) std::memcpy(buf, s.data(), s.size());
    return (int64_t)s.size();
}

}  // extern "C"
