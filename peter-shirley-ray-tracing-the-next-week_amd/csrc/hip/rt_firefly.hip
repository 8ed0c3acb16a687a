// rt_firefly.hip — guide-aware firefly clamp ahead of the denoiser.
//
//   rt_firefly_clamp<R>   a pixel whose demodulated luminance l exceeds k * (mean of l over the
//                         neighbours within R whose guides resemble its own) + floor is scaled
//                         down to that bound, with its moments; every other pixel is copied.
//
// One lane per pixel, blocks of 64 x 4, a wave on 64 consecutive pixels of a row.  A block
// stages what a tap reads — l, the raw albedo's sum s, the normal and the depth: 24 B — for its
// pixels and a halo of R in LDS ((64+2R) x (4+2R) cells, 16.4 KiB at R = 3), from coalesced
// 16-B guide loads; cells outside the image carry depth -1 and are skipped.  The (2R+1)^2 - 1
// taps then come from LDS, a ds_read_b128 and a ds_read_b64 each, consecutive lanes on
// consecutive cells.  No scratch.
//
// Only add, subtract, multiply, IEEE divide, max, min, fabs and comparisons, compiled with
// -ffp-contract=off: the statement is tests/test_firefly_spec.py's firefly_ref in numpy
// float32, which the GPU tests compare bit for bit; the expressions below follow it operation
// by operation.  It is a Jacobi pass: every value read is an input.
#include "rt_firefly.h"

namespace {

#define RT_FF_ALBEDO_MIN 0.01f   // rt_denoise.hip's demodulation floor

template <int R>
__global__ __launch_bounds__(256) void rt_firefly_clamp(int nx, int ny, const float *__restrict__ color,
                                                        const float4 *__restrict__ guides, const float *moments,
                                                        rt_firefly_params fp, float *__restrict__ out,
                                                        float *out_moments, float *__restrict__ ratio_out) {
    constexpr int W = 64 + 2 * R, H = 4 + 2 * R;
    __shared__ float4 sNZ[W * H];   // normal.xyz, depth (-1: outside the image)
    __shared__ float2 sLS[W * H];   // l, s
    const int x0 = (int)(blockIdx.x * 64) - R, y0 = (int)(blockIdx.y * 4) - R;
    for (int c = (int)(threadIdx.y * 64 + threadIdx.x); c < W * H; c += 256) {
        const int qx = x0 + c % W, qy = y0 + c / W;
        float4 nz = make_float4(0.f, 0.f, 0.f, -1.0f);
        float2 ls = make_float2(0.f, 0.f);
        if (qx >= 0 && qx < nx && qy >= 0 && qy < ny) {
            const size_t q = (size_t)qy * nx + qx;
            const float4 a = guides[q * 2];
            nz = guides[q * 2 + 1];
            const float *cq = color + q * 3;
            const float ax = fp.demodulate ? fmaxf(a.x, RT_FF_ALBEDO_MIN) : 1.0f;
            const float ay = fp.demodulate ? fmaxf(a.y, RT_FF_ALBEDO_MIN) : 1.0f;
            const float az = fp.demodulate ? fmaxf(a.z, RT_FF_ALBEDO_MIN) : 1.0f;
            ls.x = (cq[0] / ax + cq[1] / ay) + cq[2] / az;
            ls.y = (a.x + a.y) + a.z;   // the raw albedo, whatever demodulate says
        }
        sNZ[c] = nz;
        sLS[c] = ls;
    }
    __syncthreads();
    const int x = (int)(blockIdx.x * 64 + threadIdx.x), y = (int)(blockIdx.y * 4 + threadIdx.y);
    if (x >= nx || y >= ny) return;
    const int cp = ((int)threadIdx.y + R) * W + (int)threadIdx.x + R;
    const float4 Np = sNZ[cp];
    const float lp = sLS[cp].x, sp = sLS[cp].y;
    int cnt = 0;
    float sum = 0.0f;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const float4 Nq = sNZ[cp + dy * W + dx];
            const float2 Lq = sLS[cp + dy * W + dx];
            const float dn = (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z;
            const bool sim = Nq.w >= 0.0f && dn >= fp.cos_normal &&
                             fabsf(Np.w - Nq.w) <= fp.sigma_depth * fminf(Np.w, Nq.w) + 1e-6f &&
                             fabsf(sp - Lq.y) <= fp.sigma_albedo * fminf(sp, Lq.y) + 1e-6f;
            cnt += sim ? 1 : 0;
            sum = sim ? sum + Lq.x : sum;
        }
    }
    const size_t p = (size_t)y * nx + x;
    const float c0 = color[p * 3], c1 = color[p * 3 + 1], c2 = color[p * 3 + 2];
    float o0 = c0, o1 = c1, o2 = c2, ratio = 1.0f;   // an untouched pixel is the input bit for bit
    bool clamped = false;
    if (cnt >= fp.min_similar) {
        const float bound = fp.k * (sum / (float)cnt) + fp.floor;
        clamped = lp > bound;
        if (clamped) {
            const float4 a = guides[p * 2];
            const float ax = fp.demodulate ? fmaxf(a.x, RT_FF_ALBEDO_MIN) : 1.0f;
            const float ay = fp.demodulate ? fmaxf(a.y, RT_FF_ALBEDO_MIN) : 1.0f;
            const float az = fp.demodulate ? fmaxf(a.z, RT_FF_ALBEDO_MIN) : 1.0f;
            ratio = bound / lp;
            o0 = ((c0 / ax) * ratio) * ax;
            o1 = ((c1 / ay) * ratio) * ay;
            o2 = ((c2 / az) * ratio) * az;
        }
    }
    out[p * 3] = o0;
    out[p * 3 + 1] = o1;
    out[p * 3 + 2] = o2;
    if (ratio_out) ratio_out[p] = ratio;
    if (out_moments) {   // may be `moments` itself: a lane reads and writes its own pixel only
        const float m1 = moments[p * 2], m2 = moments[p * 2 + 1];
        out_moments[p * 2] = clamped ? m1 * ratio : m1;
        out_moments[p * 2 + 1] = clamped ? (m2 * ratio) * ratio : m2;
    }
}

}  // namespace

extern "C" hipError_t rt_launch_firefly(int nx, int ny, const float *color, const float *guides, const float *moments,
                                        const rt_firefly_params *fp, float *out, float *out_moments, float *ratio,
                                        hipStream_t stream) {
    if (nx <= 0 || ny <= 0) return hipSuccess;
    const dim3 grid((unsigned)((nx + 63) / 64), (unsigned)((ny + 3) / 4)), block(64, 4);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    const float4 *gd = (const float4 *)guides;
#define RT_FF_LAUNCH(R) \
    hipLaunchKernelGGL((rt_firefly_clamp<R>), grid, block, 0, stream, nx, ny, color, gd, moments, *fp, out, out_moments, ratio)
    switch (fp->radius) {
    case 1: RT_FF_LAUNCH(1); break;
    case 2: RT_FF_LAUNCH(2); break;
    case 3: RT_FF_LAUNCH(3); break;
    default: return hipErrorInvalidValue;
    }
#undef RT_FF_LAUNCH
    return hipGetLastError();
}

// the unit announces its launcher to the host when it is linked in
static const bool firefly_unit_linked = (rt_firefly_launch = RtFireflyLaunch{rt_launch_firefly}, true);
