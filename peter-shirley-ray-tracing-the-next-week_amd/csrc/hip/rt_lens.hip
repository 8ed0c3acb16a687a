// rt_lens.hip — lens renders: the rays of a perspective, orthographic, fisheye or
// equirectangular camera made on the device, and the resolve of what the radiance and ray
// queries return for them (rt_hip.h rt_lens_rays / rt_render_lens).
//
//   rt_lens_generate   one lane per (pixel, sample): the sample's stream started at the renders'
//                      own key, the two jitter draws, the model's ray and the time draw, into an
//                      rt_path_ray (and an rt_ray) record.  RT_LENS_PERSPECTIVE is camera_ray
//                      (rt_camera.h), the statement rt_features.hip traces.
//   rt_lens_resolve    adds a pixel's samples in sample order (float32): radiance, the moments
//                      of y = (r + g) + b and, from the samples' rt_hit records, the guides;
//                      the means are the sums times float(1.0 / n), as in rt_resolve.
//
// The exact float32 statement of the models is tests/test_lens_spec.py.  Compiled with
// -ffp-contract=off like the megakernel.
#include "rt_lens.h"
#include "rt_hip.h"
#include "rt_device.h"
#include "rt_camera.h"

namespace {

#define RT_LENS_PI 0x1.921fb6p+1f       // float(pi)
#define RT_LENS_2PI 0x1.921fb6p+2f      // float(2 pi)
#define RT_LENS_HALF_PI 0x1.921fb6p+0f  // float(pi / 2)

__global__ __launch_bounds__(RT_BLOCK) void rt_lens_generate(const RtKernelArgs A, const RtLensArgs L, int x0, int y0, int w,
                                                             uint32_t p0, uint32_t np, uint32_t total, uint64_t stride,
                                                             F4v *__restrict__ rays, F4v *__restrict__ trays) {
    rtl_lds_init(threadIdx.x);   // rt_libm.h's sine constants
    __syncthreads();
    const uint32_t gid = blockIdx.x * RT_BLOCK + threadIdx.x;
    const bool valid = gid < total;   // the lanes past the end compute item 0 again and store nothing
    const uint32_t it = valid ? gid : 0u;
    const uint32_t k = it / np, p = it - k * np, q = p0 + p;
    const int x = x0 + (int)(q % (uint32_t)w), j = A.ny - 1 - (y0 + (int)(q / (uint32_t)w));
    const uint32_t sample = A.sample_offset + k;
    const uint32_t pixel = (uint32_t)j * (uint32_t)A.nx + (uint32_t)x;
    const uint64_t skey = seed_key(A.seed);

    Ray r;
    uint32_t skip = 3;   // two jitter draws and the time draw
    if (L.model == RT_LENS_PERSPECTIVE) {
        uint32_t rejected;
        r = camera_ray(A, x, j, sample, skey, rejected);
        skip = 5u + 2u * rejected;
    } else {
        Rng g;
        g.start(sample_key(skey, pixel, sample), false);
        const float s = div_rn((float)((double)x + g.next()), (float)A.nx, A.rnx);   // as camera_ray's
        const float t = div_rn((float)((double)j + g.next()), (float)A.ny, A.rny);
        const float span = A.ct1 - A.ct0;   // camera.h:54; a closed shutter consumes the draw unused
        double u = 0.0;
        if (span != 0.0f) u = g.next(); else g.skip();
        r.time = (float)((double)A.ct0 + u * (double)span);
        const V3 org = mk(A.org[0], A.org[1], A.org[2]), cu = mk(A.cu[0], A.cu[1], A.cu[2]), cv = mk(A.cv[0], A.cv[1], A.cv[2]),
                 cw = mk(L.cw[0], L.cw[1], L.cw[2]);
        r.o = org;
        if (L.model == RT_LENS_ORTHOGRAPHIC) {
            const V3 hor = mk(A.hor[0], A.hor[1], A.hor[2]), ver = mk(A.ver[0], A.ver[1], A.ver[2]);
            r.o = add(add(org, scale(s - 0.5f, hor)), scale(t - 0.5f, ver));
            r.d = neg(cw);
        } else if (L.model == RT_LENS_FISHEYE) {   // equidistant
            const float fx = 2.0f * s - 1.0f, fy = 2.0f * t - 1.0f;
            const float rr = sqrtf(fx * fx + fy * fy);
            const float theta = rr * L.fov_k;
            const float st = rt_sinf(theta), ct = rt_sinf(RT_LENS_HALF_PI - theta);
            if (rr > 1.0f) r.d = mk(0.f, 0.f, 0.f);   // outside the image circle: no ray
            else if (rr == 0.0f) r.d = neg(cw);
            else r.d = sub(add(scale((st * fx) / rr, cu), scale((st * fy) / rr, cv)), scale(ct, cw));
        } else {   // RT_LENS_EQUIRECT
            const float sp = rt_sinf(RT_LENS_2PI * (s - 0.5f)), se = rt_sinf(RT_LENS_PI * (t - 0.5f));
            const float ce = rt_sinf(RT_LENS_PI * (1.0f - t)), cp = rt_sinf(RT_LENS_2PI * (0.75f - s));
            r.d = sub(add(scale(ce * sp, cu), scale(se, cv)), scale(ce * cp, cw));
        }
    }
    if (!valid) return;
    const size_t at = ((size_t)k * stride + p) * 3;   // sample-major: a wave's lanes write consecutive records
    rays[at + 0] = F4v{r.o.x, r.o.y, r.o.z, r.time};
    rays[at + 1] = F4v{r.d.x, r.d.y, r.d.z, __uint_as_float(skip)};
    rays[at + 2] = F4v{__uint_as_float(pixel), __uint_as_float(sample), 0.f, 0.f};
    if (trays) {
        trays[at + 0] = F4v{r.o.x, r.o.y, r.o.z, A.tmin};
        trays[at + 1] = F4v{r.d.x, r.d.y, r.d.z, RT_INF};
        trays[at + 2] = F4v{r.time, 0.f, 0.f, 0.f};
    }
}

__global__ __launch_bounds__(256) void rt_lens_resolve(const float4 *__restrict__ rad, const float4 *__restrict__ hits,
                                                       uint32_t np, int ns, float k, int first, int last,
                                                       float *__restrict__ rgb, float *__restrict__ mom,
                                                       float4 *__restrict__ guides) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    float cx = 0.f, cy = 0.f, cz = 0.f, m1 = 0.f, m2 = 0.f;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), g = a;
    if (!first) {   // a later batch of the pixel's samples: the sums so far are in the outputs
        cx = rgb[3 * (size_t)p]; cy = rgb[3 * (size_t)p + 1]; cz = rgb[3 * (size_t)p + 2];
        if (mom) { m1 = mom[2 * (size_t)p]; m2 = mom[2 * (size_t)p + 1]; }
        if (guides) { a = guides[(size_t)p * 2]; g = guides[(size_t)p * 2 + 1]; }
    }
#pragma unroll 4
    for (int c = 0; c < ns; ++c) {   // the loads run ahead; the adds stay in sample order
        const float4 v = rad[(size_t)c * np + p];
        cx = cx + v.x;
        cy = cy + v.y;
        cz = cz + v.z;
        const float y = (v.x + v.y) + v.z;
        m1 = m1 + y;
        m2 = m2 + y * y;
    }
    if (guides) {
#pragma unroll 4
        for (int c = 0; c < ns; ++c) {   // rt_hit: (prim, material, t, depth) (normal, albedo.r) (albedo.gb, 0, 0)
            const float4 *h = hits + ((size_t)c * np + p) * 3;
            const float4 h0 = h[0], h1 = h[1], h2 = h[2];
            const float cov = __float_as_int(h0.x) >= 0 ? 1.0f : 0.0f;
            a.x = a.x + h1.w; a.y = a.y + h2.x; a.z = a.z + h2.y; a.w = a.w + cov;
            g.x = g.x + h1.x; g.y = g.y + h1.y; g.z = g.z + h1.z; g.w = g.w + h0.w;
        }
        if (last) {
            a.x = a.x * k; a.y = a.y * k; a.z = a.z * k; a.w = a.w * k;
            g.x = g.x * k; g.y = g.y * k; g.z = g.z * k; g.w = g.w * k;
        }
        guides[(size_t)p * 2] = a;
        guides[(size_t)p * 2 + 1] = g;
    }
    if (mom) { mom[2 * (size_t)p] = m1; mom[2 * (size_t)p + 1] = m2; }
    if (last) { cx = cx * k; cy = cy * k; cz = cz * k; }
    rgb[3 * (size_t)p] = cx;
    rgb[3 * (size_t)p + 1] = cy;
    rgb[3 * (size_t)p + 2] = cz;
}

}  // namespace

extern "C" hipError_t rt_launch_lens_generate(const RtKernelArgs *a, const RtLensArgs *l, int x0, int y0, int w, uint32_t p0,
                                              uint32_t np, int ns, uint64_t stride, void *rays, void *trace_rays,
                                              hipStream_t stream) {
    const uint64_t total = (uint64_t)np * (uint64_t)(ns > 0 ? ns : 0);
    if (total == 0) return hipSuccess;
    if (total >= 0x80000000ull || w <= 0 || stride < np || !rays) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((total + RT_BLOCK - 1) / RT_BLOCK);
    hipLaunchKernelGGL(rt_lens_generate, dim3(blocks), dim3(RT_BLOCK), 0, stream, *a, *l, x0, y0, w, p0, np, (uint32_t)total,
                       stride, (F4v *)rays, (F4v *)trace_rays);
    return hipGetLastError();
}

extern "C" hipError_t rt_launch_lens_resolve(const void *radiance, const void *hits, uint32_t np, int ns, float k, int first,
                                             int last, float *rgb, float *moments, float *guides, hipStream_t stream) {
    if (np == 0) return hipSuccess;
    if (!radiance || !rgb || (guides && !hits)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rt_lens_resolve, dim3((np + 255) / 256), dim3(256), 0, stream, (const float4 *)radiance,
                       (const float4 *)hits, np, ns, k, first, last, rgb, moments, (float4 *)guides);
    return hipGetLastError();
}

// the unit announces its launchers to the host when it is linked in
static const bool lens_unit_linked = (rt_lens_launch = RtLensLaunch{rt_launch_lens_generate, rt_launch_lens_resolve}, true);
