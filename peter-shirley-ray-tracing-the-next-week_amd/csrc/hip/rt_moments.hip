// rt_moments.hip — per-pixel moments and the adaptive driver's device steps.
//
//   rt_resolve_moments   rt_resolve (rt_kernel.hip) — the same adds in the same sample
//                        order, the same FIRST / LAST / SUM_IN / RAW modes — that in the
//                        same pass over the slab keeps two more running floats per pixel:
//                        the sum and the sum of squares of the work items' channel sums.
//   rt_adaptive_select   the convergence decision of rt_render_adaptive (rt_hip.h), FP64.
//   rt_adaptive_test     the same decision for rt_render_adaptive_guarded: it retires nobody
//                        and writes a `fail` byte per pixel instead.
//   rt_adaptive_guard    retires the active pixels whose (2r+1)^2 window holds no failing pixel.
//   rt_adaptive_finish   each pixel's mean over its own sample count.
//
// Compiled with -ffp-contract=off like the megakernel: y * y and the add that follows stay
// two roundings, and the select's FP64 expression is the one numpy float64 evaluates.
#include "rt_moments.h"
#include "rt_kernel.h"

template <int SF>   // floats per slab item (rt_slab_floats)
__global__ __launch_bounds__(256) void rt_resolve_moments(const float *__restrict__ slab, uint32_t npix, int nchunks,
                                                          float k, float4 *__restrict__ acc, int mode,
                                                          const uint32_t *__restrict__ out_index, float *__restrict__ out,
                                                          float *__restrict__ mom) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const size_t o = out_index[p];
    float cx = 0.f, cy = 0.f, cz = 0.f, m1 = 0.f, m2 = 0.f;
    if (!(mode & RT_RESOLVE_FIRST)) {   // a later batch: the sums from acc, the moments in place
        const float4 a = acc[p];
        cx = a.x; cy = a.y; cz = a.z;
        m1 = mom[2 * o];
        m2 = mom[2 * o + 1];
    } else if (mode & RT_RESOLVE_SUM_IN) {
        cx = out[3 * o + 0]; cy = out[3 * o + 1]; cz = out[3 * o + 2];
        m1 = mom[2 * o];
        m2 = mom[2 * o + 1];
    }
#pragma unroll 8
    for (int c = 0; c < nchunks; ++c) {   // the loads run ahead; the adds stay in item order
        const float *v = slab + ((size_t)c * npix + p) * SF;
        const float r = v[0], g = v[1], b = v[2];
        cx = cx + r;
        cy = cy + g;
        cz = cz + b;
        const float y = (r + g) + b;
        m1 = m1 + y;
        m2 = m2 + y * y;
    }
    mom[2 * o] = m1;
    mom[2 * o + 1] = m2;
    if (!(mode & RT_RESOLVE_LAST)) {
        acc[p] = make_float4(cx, cy, cz, 0.f);
        return;
    }
    if (!(mode & RT_RESOLVE_RAW)) { cx = k * cx; cy = k * cy; cz = k * cz; }
    out[3 * o + 0] = cx;
    out[3 * o + 1] = cy;
    out[3 * o + 2] = cz;
}

__global__ __launch_bounds__(256) void rt_adaptive_select(uint32_t npix, int added, float tol, float floor,
                                                          const float *__restrict__ mom, int32_t *__restrict__ spp,
                                                          uint8_t *__restrict__ active, uint32_t *__restrict__ counters) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = i < npix && active[i] != 0;
    bool conv = false;
    if (act) {
        const int n = spp[i] + added;
        spp[i] = n;
        if (tol > 0.f) {   // tolerance <= 0: never, whatever the moments
            const double N = (double)n, S1 = (double)mom[2 * (size_t)i], S2 = (double)mom[2 * (size_t)i + 1];
            const double lhs = N * S2 - S1 * S1;
            const double t = S1 + (double)floor * N;
            const double rhs = (((double)tol * (double)tol) * (N - 1.0)) * (t * t);
            conv = lhs <= rhs;   // a NaN compares false: not converged
        }
        if (conv) active[i] = 0;
    }
    // one atomic per wave and counter
    const unsigned long long bc = __ballot(conv), ba = __ballot(act && !conv);
    if ((threadIdx.x & 63) == 0) {
        if (ba) atomicAdd(&counters[0], (uint32_t)__popcll(ba));
        if (bc) atomicAdd(&counters[1], (uint32_t)__popcll(bc));
    }
}

// rt_adaptive_select's decision, kept apart from the retirement: fail[i] = active and not
// converged, for every pixel of the frame (a retired pixel never fails).  The counts move as
// in the select; the active flags and the counters are rt_adaptive_guard's to update.
__global__ __launch_bounds__(256) void rt_adaptive_test(uint32_t npix, int added, float tol, float floor,
                                                        const float *__restrict__ mom, int32_t *__restrict__ spp,
                                                        const uint8_t *__restrict__ active, uint8_t *__restrict__ fail) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const bool act = active[i] != 0;
    bool conv = false;
    if (act) {
        const int n = spp[i] + added;
        spp[i] = n;
        if (tol > 0.f) {   // tolerance <= 0: never, whatever the moments
            const double N = (double)n, S1 = (double)mom[2 * (size_t)i], S2 = (double)mom[2 * (size_t)i + 1];
            const double lhs = N * S2 - S1 * S1;
            const double t = S1 + (double)floor * N;
            const double rhs = (((double)tol * (double)tol) * (N - 1.0)) * (t * t);
            conv = lhs <= rhs;   // a NaN compares false: not converged
        }
    }
    fail[i] = act && !conv;
}

// The neighbourhood guard: an active pixel leaves the active set iff no pixel of its
// (2r+1) x (2r+1) window, clipped to the w x h frame, fails.  One lane per pixel, a wave on
// 64 consecutive pixels of a row, a block on 64 x 4 pixels (rt_denoise.hip's shape).  The
// block stages its fail bytes and a halo of r in LDS, cells outside the frame as 0; the
// window's OR is separable: along the rows into `hd`, then down the columns.  At most ten
// byte loads from global memory per lane (1600 cells over 256 lanes at r = 8) and 6 (2r+1)
// LDS reads, against (2r+1)^2 global loads for the direct form; no scratch.
#define RT_GUARD_RMAX 8
__global__ __launch_bounds__(256) void rt_adaptive_guard(int w, int h, int r, const uint8_t *__restrict__ fail,
                                                         uint8_t *__restrict__ active, uint32_t *__restrict__ counters) {
    __shared__ uint8_t tile[4 + 2 * RT_GUARD_RMAX][64 + 2 * RT_GUARD_RMAX];
    __shared__ uint8_t hd[4 + 2 * RT_GUARD_RMAX][64];
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    const int bx = (int)blockIdx.x * 64, by = (int)blockIdx.y * 4;
    const int tw = 64 + 2 * r, th = 4 + 2 * r;
    for (int cy = ty; cy < th; cy += 4) {
        const int gy = by - r + cy;
        for (int cx = tx; cx < tw; cx += 64) {
            const int gx = bx - r + cx;
            const bool in = gx >= 0 && gx < w && gy >= 0 && gy < h;
            tile[cy][cx] = in ? fail[(size_t)gy * w + gx] : (uint8_t)0;   // nothing exists outside the frame
        }
    }
    __syncthreads();
    for (int cy = ty; cy < th; cy += 4) {
        uint32_t any = 0;
        for (int k = 0; k <= 2 * r; ++k) any |= tile[cy][tx + k];
        hd[cy][tx] = (uint8_t)any;
    }
    __syncthreads();
    uint32_t hold = 0;
    for (int k = 0; k <= 2 * r; ++k) hold |= hd[ty + k][tx];
    const int x = bx + tx, y = by + ty;
    const size_t p = (size_t)y * w + x;
    const bool act = x < w && y < h && active[p] != 0;
    const bool retire = act && hold == 0;
    if (retire) active[p] = 0;
    // one atomic per wave and counter (a wave is a row of the block)
    const unsigned long long bc = __ballot(retire), ba = __ballot(act && !retire);
    if (tx == 0) {
        if (ba) atomicAdd(&counters[0], (uint32_t)__popcll(ba));
        if (bc) atomicAdd(&counters[1], (uint32_t)__popcll(bc));
    }
}

__global__ __launch_bounds__(256) void rt_adaptive_finish(uint32_t npix, const int32_t *__restrict__ spp,
                                                          float *__restrict__ sums) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float k = (float)(1.0 / (double)(float)spp[i]);   // vec3.h:134-141
    float *v = sums + 3 * (size_t)i;
    v[0] = k * v[0];
    v[1] = k * v[1];
    v[2] = k * v[2];
}

extern "C" hipError_t rt_launch_resolve_moments(const float *slab, int slab_floats, uint32_t npix, int nchunks, float k,
                                                float4 *acc, int mode, const uint32_t *out_index, float *out, float *mom,
                                                hipStream_t stream) {
    if (npix == 0) return hipSuccess;
    if (slab_floats != 3 && slab_floats != 4) return hipErrorInvalidValue;
    const unsigned blocks = (npix + 255) / 256;
    if (slab_floats == 3)
        hipLaunchKernelGGL(rt_resolve_moments<3>, dim3(blocks), dim3(256), 0, stream, slab, npix, nchunks, k, acc, mode,
                           out_index, out, mom);
    else
        hipLaunchKernelGGL(rt_resolve_moments<4>, dim3(blocks), dim3(256), 0, stream, slab, npix, nchunks, k, acc, mode,
                           out_index, out, mom);
    return hipGetLastError();
}

extern "C" hipError_t rt_launch_adaptive_select(uint32_t npix, int added, float tol, float floor, const float *mom,
                                                int32_t *spp, uint8_t *active, uint32_t *counters, hipStream_t stream) {
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_adaptive_select, dim3((npix + 255) / 256), dim3(256), 0, stream, npix, added, tol, floor, mom, spp,
                       active, counters);
    return hipGetLastError();
}

extern "C" hipError_t rt_launch_adaptive_test(uint32_t npix, int added, float tol, float floor, const float *mom,
                                              int32_t *spp, const uint8_t *active, uint8_t *fail, hipStream_t stream) {
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_adaptive_test, dim3((npix + 255) / 256), dim3(256), 0, stream, npix, added, tol, floor, mom, spp,
                       active, fail);
    return hipGetLastError();
}

extern "C" hipError_t rt_launch_adaptive_guard(int w, int h, int r, const uint8_t *fail, uint8_t *active,
                                               uint32_t *counters, hipStream_t stream) {
    if (w <= 0 || h <= 0) return hipSuccess;
    if (r < 0 || r > RT_GUARD_RMAX) return hipErrorInvalidValue;   // the LDS tile holds a halo of 8
    const dim3 grid((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4)), block(64, 4);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rt_adaptive_guard, grid, block, 0, stream, w, h, r, fail, active, counters);
    return hipGetLastError();
}

extern "C" hipError_t rt_launch_adaptive_finish(uint32_t npix, const int32_t *spp, float *sums, hipStream_t stream) {
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_adaptive_finish, dim3((npix + 255) / 256), dim3(256), 0, stream, npix, spp, sums);
    return hipGetLastError();
}

// the unit announces its launchers to the host when it is linked in
static const bool moments_unit_linked =
    (rt_moments_launch = RtMomentsLaunch{rt_launch_resolve_moments, rt_launch_adaptive_select, rt_launch_adaptive_finish,
                                         rt_launch_adaptive_test, rt_launch_adaptive_guard},
     true);
