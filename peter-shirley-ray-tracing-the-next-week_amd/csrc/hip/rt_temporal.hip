// rt_temporal.hip — reprojected frame history ahead of the denoiser.
//
//   rt_temporal_accumulate   blends the current frame into the previous call's output: a pixel
//                            with coverage 1 is carried to the world by its depth, seen through
//                            the previous camera, and takes the history's colour, per-sample
//                            moments and length from the bilinear taps there whose guides agree
//                            with its own; with equal cameras from its own pixel, untested.
//   rt_temporal_accumulate_clamped   the same under unequal cameras with the history colour clipped
//                            to the colour box of the current frame's neighbourhood:
//                            the block's pixels and their halo are staged in LDS, the gather stays.
//   rt_temporal_accumulate_cover     the clamped form, at any radius from 0, with a history for the
//                            pixels the two above give none: a pixel that misses the
//                            geometry is reprojected by its direction, a partly covered one by the
//                            class of its dominant part; it also writes where a history came from.
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

// c clipped to mean +- gamma standard deviations of a window of n values with sum S1 and sum of squares S2
__device__ __forceinline__ float clip_to_box(float c, float S1, float S2, float n, float gamma) {
    const float m = S1 / n;
    float var = S2 / n - m * m;
    var = var < 0.0f ? 0.0f : var;
    const float sd = sqrtf(var);
    const float lo = m - gamma * sd, hi = m + gamma * sd;
    return c < lo ? lo : (c > hi ? hi : c);
}

// rt_temporal_accumulate's reprojection branch, operation for operation, for the clamped kernel
// (sharing it with that kernel moved its registers from 79 to 82 VGPRs, so its text stays as it
// was): the history of pixel (x, y), p = y * nx + x, under unequal cameras.  Sets use, nh, the
// history colour ch and per-sample moments u where it finds one; leaves them otherwise.
__device__ __forceinline__ void reproject_history(
    int x, int y, size_t p, int nx, int ny, bool have, const float4 *__restrict__ cur_guides,
    const float *__restrict__ h_color, const float4 *__restrict__ h_guides, const float *__restrict__ h_moments,
    const int32_t *__restrict__ h_len, const rt_camera_desc &cam, const rt_camera_desc &prev, const rt_temporal_params &tp,
    bool &use, int &nh, float &ch0, float &ch1, float &ch2, float &u1, float &u2) {
    const float fnx = (float)nx, fny = (float)ny;
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

// The clamped form's tile of the current frame's colour: a block's 64 x 4 pixels and a halo of
// RT_TEMPORAL_CLAMP_MAX_RADIUS on every side, a plane per channel (a wave reads 64 consecutive floats).
constexpr int TILE_W = 64 + 2 * RT_TEMPORAL_CLAMP_MAX_RADIUS, TILE_H = 4 + 2 * RT_TEMPORAL_CLAMP_MAX_RADIUS;

// rt_temporal_accumulate under unequal cameras with one step between the history fetch and the
// blend: the history colour is clipped, per channel, to mean +- gamma standard deviations of the
// current frame's colours within `radius` of the pixel (tests/test_temporal_clamp_spec.py's
// temporal_clamped_ref).  The window's colours come from the LDS tile; cells outside
// the image are not read from memory and hold zero.  Every lane of a block stays for the tile loads and the
// barriers; only lanes on a pixel go further.  R is the window's radius (its loops unroll, and
// the tile's extent stays out of the SGPRs, which the two cameras fill).
template <int R>
__global__ __launch_bounds__(256) void rt_temporal_accumulate_clamped(
    int nx, int ny, const float *__restrict__ cur_color, const float4 *__restrict__ cur_guides, const float *cur_moments,
    const float *__restrict__ h_color, const float4 *__restrict__ h_guides, const float *__restrict__ h_moments,
    const int32_t *__restrict__ h_len, float *__restrict__ o_color, float *o_moments, int32_t *__restrict__ o_len,
    int32_t *__restrict__ clipped, rt_camera_desc cam, rt_camera_desc prev, rt_temporal_params tp, float gamma) {
    __shared__ float tile[3][TILE_H][TILE_W];
    constexpr int r = R, tw = 64 + 2 * r, th = 4 + 2 * r;
    const int x0 = (int)(blockIdx.x * 64), x = x0 + (int)threadIdx.x;
    const int tid = (int)(threadIdx.y * 64 + threadIdx.x);
    const bool have = cur_moments != nullptr;
    const float nf = (float)tp.frame_spp;
    // grid.y is capped (rt_launch_temporal_clamped): a block walks the row blocks it stands for
    for (int64_t yb = (int64_t)blockIdx.y * 4; yb < ny; yb += (int64_t)gridDim.y * 4) {
        const int y0 = (int)yb, y = y0 + (int)threadIdx.y;
        __syncthreads();   // the previous row block's window sums are done with the tile
        for (int i = tid; i < th * tw * 3; i += 256) {   // a tile row is tw * 3 consecutive floats of the frame
            const int row = i / (tw * 3), rem = i - row * (tw * 3), col = rem / 3, c = rem - col * 3;
            const int gx = x0 - r + col, gy = y0 - r + row;
            const bool in = gx >= 0 && gx < nx && gy >= 0 && gy < ny;   // a cell outside the image is not read
            tile[c][row][col] = in ? cur_color[((size_t)gy * nx + gx) * 3 + c] : 0.0f;
        }
        __syncthreads();
        if (x < nx && y < ny) {
            const size_t p = (size_t)y * nx + x;
            const int tx = (int)threadIdx.x + r, ty = (int)threadIdx.y + r;
            const float cf0 = tile[0][ty][tx], cf1 = tile[1][ty][tx], cf2 = tile[2][ty][tx];
            float s1 = 0.0f, s2 = 0.0f;
            if (have) {
                s1 = cur_moments[p * 2];
                s2 = cur_moments[p * 2 + 1];
            }
            bool use = false;
            int nh = 0, mask = 0;
            float ch0 = 0.0f, ch1 = 0.0f, ch2 = 0.0f, u1 = 0.0f, u2 = 0.0f;
            reproject_history(x, y, p, nx, ny, have, cur_guides, h_color, h_guides, h_moments, h_len, cam, prev, tp, use, nh,
                              ch0, ch1, ch2, u1, u2);
            if (use) {
                // cells outside the image hold zero: S + 0 is S bit for bit (a sum that starts at +0 is never -0),
                // so every cell of the window is added and only the count knows the border
                const int cnt = (min(x + r, nx - 1) - max(x - r, 0) + 1) * (min(y + r, ny - 1) - max(y - r, 0) + 1);
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, q0 = 0.0f, q1 = 0.0f, q2 = 0.0f;
#pragma unroll
                for (int dy = -r; dy <= r; ++dy) {
#pragma unroll
                    for (int dx = -r; dx <= r; ++dx) {
                        const float v0 = tile[0][ty + dy][tx + dx], v1 = tile[1][ty + dy][tx + dx], v2 = tile[2][ty + dy][tx + dx];
                        a0 = a0 + v0;
                        a1 = a1 + v1;
                        a2 = a2 + v2;
                        q0 = q0 + v0 * v0;
                        q1 = q1 + v1 * v1;
                        q2 = q2 + v2 * v2;
                    }
                }
                const float fc = (float)cnt;
                const float k0 = clip_to_box(ch0, a0, q0, fc, gamma), k1 = clip_to_box(ch1, a1, q1, fc, gamma),
                            k2 = clip_to_box(ch2, a2, q2, fc, gamma);
                mask = (k0 != ch0 ? 1 : 0) | (k1 != ch1 ? 2 : 0) | (k2 != ch2 ? 4 : 0);
                if (have && mask) {   // the mean moves with the colour, the per-sample variance stays
                    const float yo = (ch0 + ch1) + ch2, yn = (k0 + k1) + k2;
                    float w1 = u1 + (yn - yo);
                    w1 = w1 < 0.0f ? 0.0f : w1;
                    float v = u2 - u1 * u1;
                    v = v < 0.0f ? 0.0f : v;
                    u1 = w1;
                    u2 = v + w1 * w1;
                }
                ch0 = k0;
                ch1 = k1;
                ch2 = k2;
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
            if (clipped) clipped[p] = mask;
        }
    }
}

// reproject_history with the two classes of rt_temporal_cover (tests/test_temporal_cover_spec.py's
// temporal_cover_ref), a text of its own so that the two kernels above keep theirs.
// A surface pixel (coverage c == 1, or with `edges` c >= 0.5) is carried to the world by the hit
// samples' depth N.w / c and tests its taps by their hit samples' normal and depth; a background
// pixel (with `background`: c == 0, or with `edges` c < 0.5) is a point at infinity, d = e, and
// takes every tap of its class; both need |c - c_q| <= sigma_coverage.  src receives the class of
// the history found (rt_hip.h's RT_TEMPORAL_SRC_*), and stays otherwise.
__device__ __forceinline__ void reproject_history_cover(
    int x, int y, size_t p, int nx, int ny, bool have, const float4 *__restrict__ cur_guides,
    const float *__restrict__ h_color, const float4 *__restrict__ h_guides, const float *__restrict__ h_moments,
    const int32_t *__restrict__ h_len, const rt_camera_desc &cam, const rt_camera_desc &prev, const rt_temporal_params &tp,
    bool background, bool edges, float sigma_coverage, bool &use, int &nh, float &ch0, float &ch1, float &ch2, float &u1,
    float &u2, int &src) {
    // Branches nest exec masks in SGPRs, which the two cameras fill: a lane outside both classes or
    // behind the previous camera computes on, with values that no test passes, and reads nothing.
    const float fnx = (float)nx, fny = (float)ny;
    const float4 A = cur_guides[p * 2], N = cur_guides[p * 2 + 1];
    const float c = A.w;
    const bool surf = c == 1.0f || (edges && c >= 0.5f);
    const bool back = !surf && background && (c == 0.0f || (edges && c < 0.5f));
    const float s = ((float)x + 0.5f) / fnx, t = ((float)(ny - 1 - y) + 0.5f) / fny;
    const float e0 = ((cam.lower_left_corner[0] + s * cam.horizontal[0]) + t * cam.vertical[0]) - cam.origin[0];
    const float e1 = ((cam.lower_left_corner[1] + s * cam.horizontal[1]) + t * cam.vertical[1]) - cam.origin[1];
    const float e2 = ((cam.lower_left_corner[2] + s * cam.horizontal[2]) + t * cam.vertical[2]) - cam.origin[2];
    // the hit samples' means; c == 1 leaves the bits as they are
    const float n0 = N.x / c, n1 = N.y / c, n2 = N.z / c;
    const float k = (N.w / c) / sqrtf(dot3(e0, e1, e2, e0, e1, e2));
    // the background is a point at infinity: d = e
    const float d0 = surf ? (cam.origin[0] + e0 * k) - prev.origin[0] : e0;
    const float d1 = surf ? (cam.origin[1] + e1 * k) - prev.origin[1] : e1;
    const float d2 = surf ? (cam.origin[2] + e2 * k) - prev.origin[2] : e2;
    const float dw = dot3(d0, d1, d2, prev.w[0], prev.w[1], prev.w[2]);
    const bool front = (surf || back) && dw < 0.0f;   // in a class, and in front of the previous camera
    const float a0 = prev.lower_left_corner[0] - prev.origin[0];
    const float a1 = prev.lower_left_corner[1] - prev.origin[1];
    const float a2 = prev.lower_left_corner[2] - prev.origin[2];
    const float tau = dot3(a0, a1, a2, prev.w[0], prev.w[1], prev.w[2]) / dw;
    const float r0 = d0 * tau - a0, r1 = d1 * tau - a1, r2 = d2 * tau - a2;
    const float sp = dot3(r0, r1, r2, prev.horizontal[0], prev.horizontal[1], prev.horizontal[2]) /
                     dot3(prev.horizontal[0], prev.horizontal[1], prev.horizontal[2], prev.horizontal[0],
                          prev.horizontal[1], prev.horizontal[2]);
    const float tq = dot3(r0, r1, r2, prev.vertical[0], prev.vertical[1], prev.vertical[2]) /
                     dot3(prev.vertical[0], prev.vertical[1], prev.vertical[2], prev.vertical[0], prev.vertical[1],
                          prev.vertical[2]);
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
            bool in = front && w > 0.0f && qxf >= 0.0f && qxf < fnx && qyf >= 0.0f && qyf < fny;
            const int qx = in ? (int)qxf : 0, qy = in ? (int)qyf : 0;
            in = in && qx < nx && qy < ny;   // float(nx) may have rounded up
            if (in) {
                const size_t q = (size_t)qy * nx + qx;
                const int lq = h_len[q];
                const float4 Aq = h_guides[q * 2], Nq = h_guides[q * 2 + 1];
                const float cq = Aq.w;
                // a tap outside the surface class may divide by zero here: its class test fails
                const float dn = dot3(n0, n1, n2, Nq.x / cq, Nq.y / cq, Nq.z / cq), zq = Nq.w / cq;
                const bool ok_s = (cq == 1.0f || (edges && cq >= 0.5f)) && dn >= tp.cos_normal &&
                                  fabsf(zp - zq) <= tp.sigma_depth * fminf(zp, zq) + 1e-6f;
                const bool ok_b = cq == 0.0f || (edges && cq < 0.5f);
                const bool ok = lq > 0 && fabsf(c - cq) <= sigma_coverage && (surf ? ok_s : ok_b);
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
    nh = min(nmin, tp.max_history);
    use = W > 0.0f && nh > 0;   // W > 0 only where a tap counted
    if (use) {
        ch0 = C0 / W;
        ch1 = C1 / W;
        ch2 = C2 / W;
        u1 = m1 / W;
        u2 = m2 / W;
        src = (surf ? RT_TEMPORAL_SRC_SURFACE : RT_TEMPORAL_SRC_BACKGROUND) |
              ((c != 0.0f && c != 1.0f) ? RT_TEMPORAL_SRC_EDGE : 0);
    }
}

// rt_temporal_accumulate_clamped with reproject_history_cover in reproject_history's place, for
// unequal cameras at any radius: R = 0 has no clamp, no tile and no barrier (the frame's colour
// comes from global memory, `clipped` receives 0), R >= 1 stages the tile and clips as the clamped
// kernel does, on every pixel that found a history, whatever its class.  `classes` carries
// rt_temporal_cover_params' two switches (bit 0 background, bit 1 edges).
template <int R>
__global__ __launch_bounds__(256) void rt_temporal_accumulate_cover(
    int nx, int ny, const float *__restrict__ cur_color, const float4 *__restrict__ cur_guides, const float *cur_moments,
    const float *__restrict__ h_color, const float4 *__restrict__ h_guides, const float *__restrict__ h_moments,
    const int32_t *__restrict__ h_len, float *__restrict__ o_color, float *o_moments, int32_t *__restrict__ o_len,
    int32_t *__restrict__ clipped, int32_t *__restrict__ source, rt_camera_desc cam, rt_camera_desc prev,
    rt_temporal_params tp, float gamma, int classes, float sigma_coverage) {
    __shared__ float tile[R ? 3 : 1][R ? TILE_H : 1][R ? TILE_W : 1];   // unused, and dropped, at R = 0
    constexpr int r = R, tw = 64 + 2 * r, th = 4 + 2 * r;
    const int x0 = (int)(blockIdx.x * 64), x = x0 + (int)threadIdx.x;
    const int tid = (int)(threadIdx.y * 64 + threadIdx.x);
    const bool have = cur_moments != nullptr;
    const float nf = (float)tp.frame_spp;
    // grid.y is capped (rt_launch_temporal_cover): a block walks the row blocks it stands for.  ny is below
    // 2^31 and a step at most 4 * 65535, so an unsigned row never wraps (and costs one SGPR, not two)
    for (unsigned yb = blockIdx.y * 4u; yb < (unsigned)ny; yb += gridDim.y * 4u) {
        const int y0 = (int)yb, y = y0 + (int)threadIdx.y;
        if constexpr (R > 0) {
            __syncthreads();   // the previous row block's window sums are done with the tile
            for (int i = tid; i < th * tw * 3; i += 256) {   // a tile row is tw * 3 consecutive floats of the frame
                const int row = i / (tw * 3), rem = i - row * (tw * 3), col = rem / 3, c = rem - col * 3;
                const int gx = x0 - r + col, gy = y0 - r + row;
                const bool in = gx >= 0 && gx < nx && gy >= 0 && gy < ny;   // a cell outside the image is not read
                tile[c][row][col] = in ? cur_color[((size_t)gy * nx + gx) * 3 + c] : 0.0f;
            }
            __syncthreads();
        }
        if (x < nx && y < ny) {
            const size_t p = (size_t)y * nx + x;
            const int tx = (int)threadIdx.x + r, ty = (int)threadIdx.y + r;
            float cf0, cf1, cf2;
            if constexpr (R > 0) {
                cf0 = tile[0][ty][tx];
                cf1 = tile[1][ty][tx];
                cf2 = tile[2][ty][tx];
            } else {
                cf0 = cur_color[p * 3];
                cf1 = cur_color[p * 3 + 1];
                cf2 = cur_color[p * 3 + 2];
            }
            float s1 = 0.0f, s2 = 0.0f;
            if (have) {
                s1 = cur_moments[p * 2];
                s2 = cur_moments[p * 2 + 1];
            }
            bool use = false;
            int nh = 0, mask = 0, src = RT_TEMPORAL_SRC_NONE;
            float ch0 = 0.0f, ch1 = 0.0f, ch2 = 0.0f, u1 = 0.0f, u2 = 0.0f;
            reproject_history_cover(x, y, p, nx, ny, have, cur_guides, h_color, h_guides, h_moments, h_len, cam, prev, tp,
                                    (classes & 1) != 0, (classes & 2) != 0, sigma_coverage, use, nh, ch0, ch1, ch2, u1, u2, src);
            if constexpr (R > 0) {
                if (use) {
                    // cells outside the image hold zero: S + 0 is S bit for bit (a sum that starts at +0 is never -0),
                    // so every cell of the window is added and only the count knows the border
                    const int cnt = (min(x + r, nx - 1) - max(x - r, 0) + 1) * (min(y + r, ny - 1) - max(y - r, 0) + 1);
                    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, q0 = 0.0f, q1 = 0.0f, q2 = 0.0f;
#pragma unroll
                    for (int dy = -r; dy <= r; ++dy) {
#pragma unroll
                        for (int dx = -r; dx <= r; ++dx) {
                            const float v0 = tile[0][ty + dy][tx + dx], v1 = tile[1][ty + dy][tx + dx],
                                        v2 = tile[2][ty + dy][tx + dx];
                            a0 = a0 + v0;
                            a1 = a1 + v1;
                            a2 = a2 + v2;
                            q0 = q0 + v0 * v0;
                            q1 = q1 + v1 * v1;
                            q2 = q2 + v2 * v2;
                        }
                    }
                    const float fc = (float)cnt;
                    const float k0 = clip_to_box(ch0, a0, q0, fc, gamma), k1 = clip_to_box(ch1, a1, q1, fc, gamma),
                                k2 = clip_to_box(ch2, a2, q2, fc, gamma);
                    mask = (k0 != ch0 ? 1 : 0) | (k1 != ch1 ? 2 : 0) | (k2 != ch2 ? 4 : 0);
                    if (have && mask) {   // the mean moves with the colour, the per-sample variance stays
                        const float yo = (ch0 + ch1) + ch2, yn = (k0 + k1) + k2;
                        float w1 = u1 + (yn - yo);
                        w1 = w1 < 0.0f ? 0.0f : w1;
                        float v = u2 - u1 * u1;
                        v = v < 0.0f ? 0.0f : v;
                        u1 = w1;
                        u2 = v + w1 * w1;
                    }
                    ch0 = k0;
                    ch1 = k1;
                    ch2 = k2;
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
            if (clipped) clipped[p] = mask;
            if (source) source[p] = src;
        }
    }
}

// rt_temporal_cover's `source` under equal cameras: rt_temporal_accumulate's static branch uses
// the history of pixel p when min(len, max_history) > 0.
__global__ __launch_bounds__(256) void rt_temporal_mark_same(int64_t npix, const int32_t *__restrict__ h_len, int max_history,
                                                             int32_t *__restrict__ source) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (int64_t)gridDim.x * 256)
        source[p] = min(h_len[p], max_history) > 0 ? RT_TEMPORAL_SRC_SAME : RT_TEMPORAL_SRC_NONE;
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

extern "C" hipError_t rt_launch_temporal_clamped(int nx, int ny, int mode, const rt_temporal_frame *cur,
                                                 const rt_camera_desc *cam, const rt_temporal_frame *hist,
                                                 const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                                                 const rt_temporal_clamp_params *cp, const rt_temporal_frame *out,
                                                 int32_t *clipped, hipStream_t stream) {
    if (nx <= 0 || ny <= 0) return hipSuccess;
    if (cp->radius < 0 || cp->radius > RT_TEMPORAL_CLAMP_MAX_RADIUS) return hipErrorInvalidValue;   // the tile's halo
    // nothing is clamped: rt_temporal itself (the caller has zeroed `clipped`)
    if (!rt_temporal_clamps(mode, cp)) return rt_launch_temporal(nx, ny, mode, cur, cam, hist, prev_cam, tp, out, stream);
    if (!hist || !prev_cam) return hipErrorInvalidValue;
    const int64_t rows = ((int64_t)ny + 3) / 4;
    const dim3 grid((unsigned)(((int64_t)nx + 63) / 64), (unsigned)(rows < 65535 ? rows : 65535)), block(64, 4);
    const auto kernel = cp->radius == 1 ? rt_temporal_accumulate_clamped<1>
                        : cp->radius == 2 ? rt_temporal_accumulate_clamped<2> : rt_temporal_accumulate_clamped<3>;
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, nx, ny, cur->color, (const float4 *)cur->guides, cur->moments,
                       hist->color, (const float4 *)hist->guides, cur->moments ? hist->moments : nullptr, hist->len,
                       (float *)out->color, cur->moments ? (float *)out->moments : nullptr, (int32_t *)out->len, clipped, *cam,
                       *prev_cam, *tp, cp->gamma);
    return hipGetLastError();
}

extern "C" hipError_t rt_launch_temporal_cover(int nx, int ny, int mode, const rt_temporal_frame *cur,
                                               const rt_camera_desc *cam, const rt_temporal_frame *hist,
                                               const rt_camera_desc *prev_cam, const rt_temporal_params *tp,
                                               const rt_temporal_clamp_params *cp, const rt_temporal_cover_params *vp,
                                               const rt_temporal_frame *out, int32_t *clipped, int32_t *source,
                                               hipStream_t stream) {
    if (nx <= 0 || ny <= 0) return hipSuccess;
    if (cp->radius < 0 || cp->radius > RT_TEMPORAL_CLAMP_MAX_RADIUS) return hipErrorInvalidValue;   // the tile's halo
    // no class applies: rt_temporal itself (the caller has filled `clipped` and `source`)
    if (mode != RT_TEMPORAL_REPROJECT) return rt_launch_temporal(nx, ny, mode, cur, cam, hist, prev_cam, tp, out, stream);
    if (!hist || !prev_cam) return hipErrorInvalidValue;
    const int64_t rows = ((int64_t)ny + 3) / 4;
    const dim3 grid((unsigned)(((int64_t)nx + 63) / 64), (unsigned)(rows < 65535 ? rows : 65535)), block(64, 4);
    const auto kernel = cp->radius == 0 ? rt_temporal_accumulate_cover<0>
                        : cp->radius == 1 ? rt_temporal_accumulate_cover<1>
                        : cp->radius == 2 ? rt_temporal_accumulate_cover<2> : rt_temporal_accumulate_cover<3>;
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, nx, ny, cur->color, (const float4 *)cur->guides, cur->moments,
                       hist->color, (const float4 *)hist->guides, cur->moments ? hist->moments : nullptr, hist->len,
                       (float *)out->color, cur->moments ? (float *)out->moments : nullptr, (int32_t *)out->len, clipped, source,
                       *cam, *prev_cam, *tp, cp->gamma, (vp->background ? 1 : 0) | (vp->edges ? 2 : 0), vp->sigma_coverage);
    return hipGetLastError();
}

extern "C" hipError_t rt_launch_temporal_same(int nx, int ny, const int32_t *hist_len, int max_history, int32_t *source,
                                              hipStream_t stream) {
    if (nx <= 0 || ny <= 0 || !source) return hipSuccess;
    if (!hist_len) return hipErrorInvalidValue;
    const int64_t npix = (int64_t)nx * ny, blocks = (npix + 255) / 256;
    hipLaunchKernelGGL(rt_temporal_mark_same, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(256), 0, stream, npix,
                       hist_len, max_history, source);
    return hipGetLastError();
}

// the unit announces its launchers to the host when it is linked in
static const bool temporal_unit_linked =
    (rt_temporal_launch = RtTemporalLaunch{rt_launch_temporal, rt_launch_temporal_clamped, rt_launch_temporal_cover,
                                           rt_launch_temporal_same},
     true);
