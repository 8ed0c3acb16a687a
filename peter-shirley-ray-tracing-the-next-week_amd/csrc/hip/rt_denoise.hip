// rt_denoise.hip — edge-avoiding à-trous wavelet filter guided by the first-hit features
// and the per-pixel variance (Dammertz et al. 2010, with the variance
// guidance of Schied et al. 2017 and, on request, their 3 x 3 pre-filter of the variance).
//
//   rt_denoise_prepare   packs two float4 planes per pixel: G = (normal.xyz, depth) and
//                        E = (colour / a', variance of the mean of the demodulated luminance).
//   rt_denoise_atrous    one iteration over a 5 x 5 footprint with taps `step` pixels apart.
//
// One lane per pixel, a wave on 64 consecutive pixels of a row: a tap row of a wave is one
// coalesced 1-KiB dwordx4 load per plane, and a tap is two 16-B loads.  No LDS, no scratch.
//
// Only add, subtract, multiply, IEEE divide, max, min and fabs, compiled with
// -ffp-contract=off: a fixed sequence of float32 operations, which tests/test_denoise_spec.py
// restates in numpy and the GPU tests compare bit for bit.  The statement of the filter is
// that file, and tests/test_denoise_varfilter_spec.py for the variance pre-filter; the
// expressions below follow them operation by operation.
#include "rt_denoise.h"

namespace {

#define RT_DN_ALBEDO_MIN 0.01f

__device__ __forceinline__ float3 demod_albedo(float4 a, int demodulate) {
    if (!demodulate) return make_float3(1.0f, 1.0f, 1.0f);
    return make_float3(fmaxf(a.x, RT_DN_ALBEDO_MIN), fmaxf(a.y, RT_DN_ALBEDO_MIN), fmaxf(a.z, RT_DN_ALBEDO_MIN));
}

__global__ __launch_bounds__(256) void rt_denoise_prepare(uint32_t npix, const float *__restrict__ color,
                                                          const float4 *__restrict__ guides,
                                                          const float *__restrict__ moments,
                                                          const int32_t *__restrict__ spp, int uniform_spp, int demodulate,
                                                          float4 *__restrict__ G, float4 *__restrict__ E) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const float3 a = demod_albedo(guides[(size_t)p * 2], demodulate);
    G[p] = guides[(size_t)p * 2 + 1];
    const float *c = color + (size_t)p * 3;
    float v = 0.f;
    if (moments) {
        const float Nf = (float)(spp ? spp[p] : uniform_spp);
        if (Nf >= 2.0f) {   // one sample carries no variance: v stays 0
            const float m1 = moments[(size_t)p * 2], m2 = moments[(size_t)p * 2 + 1];
            const float s = ((a.x + a.y) + a.z) * (float)(1.0 / 3.0);
            v = fmaxf(0.f, m2 - (m1 * m1) / Nf) / ((Nf - 1.0f) * Nf) / (s * s);
        }
    }
    E[p] = make_float4(c[0] / a.x, c[1] / a.y, c[2] / a.z, v);
}

// kVar: the luminance weight (moments were present); kVf: its denominator from the 3 x 3
// Gaussian of the input variance (rt_denoise_params.variance_filter; only with kVar);
// kLast: write colour * a' to out_rgb
template <bool kVar, bool kVf, bool kLast>
__global__ __launch_bounds__(256) void rt_denoise_atrous(int nx, int ny, int step, float sc2, float sz,
                                                         const float4 *__restrict__ G, const float4 *__restrict__ Ein,
                                                         float4 *__restrict__ Eout, const float4 *__restrict__ guides,
                                                         int demodulate, float *__restrict__ out_rgb) {
    const int x = (int)(blockIdx.x * 64 + threadIdx.x), y = (int)(blockIdx.y * 4 + threadIdx.y);
    if (x >= nx || y >= ny) return;
    const size_t p = (size_t)y * nx + x;
    const float4 Gp = G[p], Ep = Ein[p];
    const float lp = (Ep.x + Ep.y) + Ep.z;
    float vc = Ep.w;
    if (kVar && kVf) {
        // SVGF's pre-filter: the direct neighbours whatever `step` is, a neighbour outside the
        // image replaced by the centre.  The products g * g are powers of two: only the adds round.
        const float g[3] = {0.25f, 0.5f, 0.25f};
        vc = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx, qy = y + dy;
                const bool in = qx >= 0 && qx < nx && qy >= 0 && qy < ny;
                vc = vc + (g[dy + 1] * g[dx + 1]) * Ein[in ? (size_t)qy * nx + qx : p].w;
            }
        }
    }
    const float lden = sc2 * vc + 1e-8f;
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.f, sx = 0.f, sy = 0.f, sb = 0.f, sv = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (dy == 0 && dx == 0) {   // the centre: no edge stopping, and no difference to add
                const float w = h[2] * h[2];
                sw = sw + w;
                sv = sv + (w * w) * Ep.w;
                continue;
            }
            const int qx = x + step * dx, qy = y + step * dy;
            const bool in = qx >= 0 && qx < nx && qy >= 0 && qy < ny;
            const size_t q = in ? (size_t)qy * nx + qx : p;   // a tap outside the image: the centre's data, weight 0
            const float4 Gq = G[q], Eq = Ein[q];
            float wn = fmaxf(0.f, (Gp.x * Gq.x + Gp.y * Gq.y) + Gp.z * Gq.z);
#pragma unroll
            for (int k = 0; k < 7; ++k) wn = wn * wn;   // power 128
            const float xz = fabsf(Gp.w - Gq.w) / (sz * fminf(Gp.w, Gq.w) + 1e-6f);
            const float wz = 1.0f / (1.0f + xz * xz);
            float w = ((h[dy + 2] * h[dx + 2]) * wn) * wz;
            if (kVar) {
                const float dl = lp - ((Eq.x + Eq.y) + Eq.z);
                w = w * (1.0f / (1.0f + (dl * dl) / lden));
            }
            w = in ? w : 0.f;
            sw = sw + w;
            sx = sx + w * (Eq.x - Ep.x);
            sy = sy + w * (Eq.y - Ep.y);
            sb = sb + w * (Eq.z - Ep.z);
            sv = sv + (w * w) * Eq.w;
        }
    }
    // sum(w e(q)) / sum(w) as e(p) + sum(w (e(q) - e(p))) / sum(w): a pixel whose guides
    // reject every neighbour keeps its value exactly
    const float ex = Ep.x + sx / sw, ey = Ep.y + sy / sw, ez = Ep.z + sb / sw;
    if (kLast) {
        const float3 a = demod_albedo(guides[p * 2], demodulate);
        out_rgb[p * 3 + 0] = ex * a.x;
        out_rgb[p * 3 + 1] = ey * a.y;
        out_rgb[p * 3 + 2] = ez * a.z;
    } else {
        Eout[p] = make_float4(ex, ey, ez, sv / (sw * sw));
    }
}

}  // namespace

extern "C" hipError_t rt_launch_denoise_prepare(uint32_t npix, const float *color, const float *guides,
                                                const float *moments, const int32_t *spp, int uniform_spp,
                                                int demodulate, float4 *G, float4 *E, hipStream_t stream) {
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_denoise_prepare, dim3((npix + 255) / 256), dim3(256), 0, stream, npix, color,
                       (const float4 *)guides, moments, spp, uniform_spp, demodulate, G, E);
    return hipGetLastError();
}

extern "C" hipError_t rt_launch_denoise_atrous(int nx, int ny, int step, float sigma_color, float sigma_depth,
                                               int use_var, int variance_filter, const float4 *G, const float4 *E_in,
                                               float4 *E_out, const float *guides, int demodulate, float *out_rgb,
                                               hipStream_t stream) {
    if (nx <= 0 || ny <= 0) return hipSuccess;
    const dim3 grid((unsigned)((nx + 63) / 64), (unsigned)((ny + 3) / 4)), block(64, 4);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    const float sc2 = sigma_color * sigma_color, sz = sigma_depth * (float)step;
    const float4 *gd = (const float4 *)guides;
#define RT_DN_LAUNCH(V, F, L) \
    hipLaunchKernelGGL((rt_denoise_atrous<V, F, L>), grid, block, 0, stream, nx, ny, step, sc2, sz, G, E_in, E_out, gd, demodulate, out_rgb)
    if (use_var && variance_filter) { if (out_rgb) RT_DN_LAUNCH(true, true, true); else RT_DN_LAUNCH(true, true, false); }
    else if (use_var) { if (out_rgb) RT_DN_LAUNCH(true, false, true); else RT_DN_LAUNCH(true, false, false); }
    else { if (out_rgb) RT_DN_LAUNCH(false, false, true); else RT_DN_LAUNCH(false, false, false); }   // no moments: the switch has no effect
#undef RT_DN_LAUNCH
    return hipGetLastError();
}

// the unit announces its launchers to the host when it is linked in
static const bool denoise_unit_linked =
    (rt_denoise_launch = RtDenoiseLaunch{rt_launch_denoise_prepare, rt_launch_denoise_atrous}, true);
