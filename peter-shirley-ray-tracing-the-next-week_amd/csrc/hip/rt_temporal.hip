// rt_temporal.hip — reprojected frame history ahead of the denoiser.
//
//   rt_temporal_accumulate   blends the current frame into the previous call's output: a pixel
//                            with coverage 1 is carried to the world by its depth, seen through
//                            the previous camera, and takes the history's colour, per-sample
//                            moments and length from the bilinear taps there whose guides agree
//                            with its own; with equal cameras from its own pixel, untested.
//
// One lane per pixel, blocks of 64 x 4, a wave on 64 consecutive pixels of a row.  The pixel's
// own guides come as two 16-B loads; the four taps are gathered from global memory (two 16-B
// guide loads and the length each, colour and moments only for a tap that counts): where a
// block's pixels land in the previous frame is not bounded, so there is no LDS tile.  The two
// cameras travel by value in the kernel arguments and stay in SGPRs.  No scratch.
//
// Only add, subtract, multiply, IEEE divide, sqrtf, floorf, max, min, fabs and comparisons,
// compiled with -ffp-contract=off: the statement is tests/test_temporal_spec.py's temporal_ref
// in numpy float32, which the GPU tests compare bit for bit; the expressions below follow it
// operation by operation.  It is a Jacobi pass: every value read is an input.
#include "rt_temporal.h"

namespace {

__device__ __forceinline__ float dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

__global__ __launch_bounds__(256) void rt_temporal_accumulate(
    int nx, int ny, int mode, const float *__restrict__ cur_color, const float4 *__restrict__ cur_guides,
    const float *cur_moments, const float *__restrict__ h_color, const float4 *__restrict__ h_guides,
    const float *__restrict__ h_moments, const int32_t *__restrict__ h_len, float *__restrict__ o_color, float *o_moments,
    int32_t *__restrict__ o_len, rt_camera_desc cam, rt_camera_desc prev, rt_temporal_params tp) {
    const int x = (int)(blockIdx.x * 64 + threadIdx.x);
    if (x >= nx) return;
    const bool have = cur_moments != nullptr;
    const float fnx = (float)nx, fny = (float)ny, nf = (float)tp.frame_spp;
    // grid.y is capped (rt_launch_temporal): a block walks the rows it stands for
    for (int64_t yy = (int64_t)blockIdx.y * 4 + threadIdx.y; yy < ny; yy += (int64_t)gridDim.y * 4) {
        const int y = (int)yy;
        const size_t p = (size_t)y * nx + x;
        const float cf0 = cur_color[p * 3], cf1 = cur_color[p * 3 + 1], cf2 = cur_color[p * 3 + 2];
        float s1 = 0.0f, s2 = 0.0f;
        if (have) {
            s1 = cur_moments[p * 2];
            s2 = cur_moments[p * 2 + 1];
        }
        bool use = false;
        int nh = 0;
        float ch0 = 0.0f, ch1 = 0.0f, ch2 = 0.0f, u1 = 0.0f, u2 = 0.0f;
        if (mode == RT_TEMPORAL_STATIC) {   // its own pixel, weight 1, no tests
            const int l = h_len[p];
            nh = min(l, tp.max_history);
            if (nh > 0) {
                use = true;
                ch0 = h_color[p * 3];
                ch1 = h_color[p * 3 + 1];
                ch2 = h_color[p * 3 + 2];
                if (have) {
                    const float fl = (float)l;
                    u1 = h_moments[p * 2] / fl;
                    u2 = h_moments[p * 2 + 1] / fl;
                }
            }
        } else if (mode == RT_TEMPORAL_REPROJECT) {
            const float4 A = cur_guides[p * 2], N = cur_guides[p * 2 + 1];
            if (A.w == 1.0f) {
                const float s = ((float)x + 0.5f) / fnx, t = ((float)(ny - 1 - y) + 0.5f) / fny;
                const float e0 = ((cam.lower_left_corner[0] + s * cam.horizontal[0]) + t * cam.vertical[0]) - cam.origin[0];
                const float e1 = ((cam.lower_left_corner[1] + s * cam.horizontal[1]) + t * cam.vertical[1]) - cam.origin[1];
                const float e2 = ((cam.lower_left_corner[2] + s * cam.horizontal[2]) + t * cam.vertical[2]) - cam.origin[2];
                const float k = N.w / sqrtf(dot3(e0, e1, e2, e0, e1, e2));
                const float d0 = (cam.origin[0] + e0 * k) - prev.origin[0];
                const float d1 = (cam.origin[1] + e1 * k) - prev.origin[1];
                const float d2 = (cam.origin[2] + e2 * k) - prev.origin[2];
                const float dw = dot3(d0, d1, d2, prev.w[0], prev.w[1], prev.w[2]);
                if (dw < 0.0f) {   // in front of the previous camera
                    const float a0 = prev.lower_left_corner[0] - prev.origin[0];
                    const float a1 = prev.lower_left_corner[1] - prev.origin[1];
                    const float a2 = prev.lower_left_corner[2] - prev.origin[2];
                    const float tau = dot3(a0, a1, a2, prev.w[0], prev.w[1], prev.w[2]) / dw;
                    const float r0 = d0 * tau - a0, r1 = d1 * tau - a1, r2 = d2 * tau - a2;
                    const float sp = dot3(r0, r1, r2, prev.horizontal[0], prev.horizontal[1], prev.horizontal[2]) /
                                     dot3(prev.horizontal[0], prev.horizontal[1], prev.horizontal[2], prev.horizontal[0],
                                          prev.horizontal[1], prev.horizontal[2]);
                    const float tq = dot3(r0, r1, r2, prev.vertical[0], prev.vertical[1], prev.vertical[2]) /
                                     dot3(prev.vertical[0], prev.vertical[1], prev.vertical[2], prev.vertical[0],
                                          prev.vertical[1], prev.vertical[2]);
                    const float fx = sp * fnx - 0.5f, fy = (float)(ny - 1) - (tq * fny - 0.5f);
                    const float zp = sqrtf(dot3(d0, d1, d2, d0, d1, d2));
                    const float bx = floorf(fx), by = floorf(fy);
                    const float wx1 = fx - bx, wy1 = fy - by, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
                    float W = 0.0f, C0 = 0.0f, C1 = 0.0f, C2 = 0.0f, m1 = 0.0f, m2 = 0.0f;
                    int nmin = 0x7FFFFFFF;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            const float qxf = bx + (float)i, qyf = by + (float)j;
                            const float w = (i ? wx1 : wx0) * (j ? wy1 : wy0);
                            // a NaN or infinite position fails these; only then are the integers taken
                            bool in = w > 0.0f && qxf >= 0.0f && qxf < fnx && qyf >= 0.0f && qyf < fny;
                            const int qx = in ? (int)qxf : 0, qy = in ? (int)qyf : 0;
                            in = in && qx < nx && qy < ny;   // float(nx) may have rounded up
                            if (in) {
                                const size_t q = (size_t)qy * nx + qx;
                                const int lq = h_len[q];
                                const float4 Aq = h_guides[q * 2], Nq = h_guides[q * 2 + 1];
                                const float dn = dot3(N.x, N.y, N.z, Nq.x, Nq.y, Nq.z);
                                const bool ok = lq > 0 && Aq.w == 1.0f && dn >= tp.cos_normal &&
                                                fabsf(zp - Nq.w) <= tp.sigma_depth * fminf(zp, Nq.w) + 1e-6f;
                                if (ok) {
                                    W = W + w;
                                    C0 = C0 + w * h_color[q * 3];
                                    C1 = C1 + w * h_color[q * 3 + 1];
                                    C2 = C2 + w * h_color[q * 3 + 2];
                                    if (have) {
                                        const float fl = (float)lq;
                                        m1 = m1 + w * (h_moments[q * 2] / fl);
                                        m2 = m2 + w * (h_moments[q * 2 + 1] / fl);
                                    }
                                    nmin = min(nmin, lq);
                                }
                            }
                        }
                    }
                    if (W > 0.0f) {
                        nh = min(nmin, tp.max_history);
                        if (nh > 0) {
                            use = true;
                            ch0 = C0 / W;
                            ch1 = C1 / W;
                            ch2 = C2 / W;
                            u1 = m1 / W;
                            u2 = m2 / W;
                        }
                    }
                }
            }
        }
        float o0 = cf0, o1 = cf1, o2 = cf2, om1 = s1, om2 = s2;   // no history: the frame bit for bit
        int n = tp.frame_spp;
        if (use) {
            n = nh + tp.frame_spp;   // below 2^24: float(n) is exact
            const float fn = (float)n, a = nf / fn;
            o0 = ch0 + (cf0 - ch0) * a;
            o1 = ch1 + (cf1 - ch1) * a;
            o2 = ch2 + (cf2 - ch2) * a;
            om1 = (u1 + (s1 / nf - u1) * a) * fn;
            om2 = (u2 + (s2 / nf - u2) * a) * fn;
        }
        o_color[p * 3] = o0;
        o_color[p * 3 + 1] = o1;
        o_color[p * 3 + 2] = o2;
        o_len[p] = n;
        if (o_moments) {   // may be cur's moments: a lane reads and writes its own pixel only
            o_moments[p * 2] = om1;
            o_moments[p * 2 + 1] = om2;
        }
    }
}

}  // namespace

extern "C" hipError_t rt_launch_temporal(int nx, int ny, int mode, const rt_temporal_frame *cur, const rt_camera_desc *cam,
                                         const rt_temporal_frame *hist, const rt_camera_desc *prev_cam,
                                         const rt_temporal_params *tp, const rt_temporal_frame *out, hipStream_t stream) {
    if (nx <= 0 || ny <= 0) return hipSuccess;
    if (mode != RT_TEMPORAL_FIRST && mode != RT_TEMPORAL_STATIC && mode != RT_TEMPORAL_REPROJECT) return hipErrorInvalidValue;
    if (mode != RT_TEMPORAL_FIRST && (!hist || !prev_cam)) return hipErrorInvalidValue;
    const int64_t rows = ((int64_t)ny + 3) / 4;
    const dim3 grid((unsigned)(((int64_t)nx + 63) / 64), (unsigned)(rows < 65535 ? rows : 65535)), block(64, 4);
    const rt_temporal_frame none = {nullptr, nullptr, nullptr, nullptr};
    const rt_temporal_frame &h = mode == RT_TEMPORAL_FIRST ? none : *hist;
    hipLaunchKernelGGL(rt_temporal_accumulate, grid, block, 0, stream, nx, ny, mode, cur->color, (const float4 *)cur->guides,
                       cur->moments, h.color, (const float4 *)h.guides, cur->moments ? h.moments : nullptr, h.len,
                       (float *)out->color, cur->moments ? (float *)out->moments : nullptr, (int32_t *)out->len, *cam,
                       mode == RT_TEMPORAL_FIRST ? *cam : *prev_cam, *tp);
    return hipGetLastError();
}

// the unit announces its launcher to the host when it is linked in
static const bool temporal_unit_linked = (rt_temporal_launch = RtTemporalLaunch{rt_launch_temporal}, true);
