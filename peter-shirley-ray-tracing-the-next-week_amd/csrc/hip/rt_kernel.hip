// rt_kernel.hip — the megakernel's main unit: the plain, count and profile variants of
// rt_megakernel (rt_megakernel.h; each feature set x {BVH in HBM, BVH2 in LDS, flat scan}, and
// the wide BVHs' all-feature variants), the resolve and math-probe kernels, and the launch
// interface of rt_kernel.h.  The right-fold and ray-source variants are units of their own
// (rt_kernel_fold.hip, rt_kernel_rays.hip), which announce themselves when linked in: this
// object links and runs everything else without them.
#include "rt_kernel_launch.h"

namespace {

// Adds one sample batch's partial sums to each pixel's running sum, in sample
// order (main.cpp:311 `col += temp`, one add per sample with one sample per work
// item), so the image does not depend on how the samples were split into batches
// (capi_render.cpp bounds the slab per launch).  The last batch applies `col /= float(ns)`
// as the reciprocal multiply of vec3.h:134-141.
__global__ __launch_bounds__(256) void rt_resolve(const float *__restrict__ slab, uint32_t npix, int nchunks, float k,
                                                  float4 *__restrict__ acc, int mode,
                                                  const uint32_t *__restrict__ out_index, float *__restrict__ out) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const uint32_t o = out_index[p];
    V3 col = mk(0, 0, 0);
    if (!(mode & RT_RESOLVE_FIRST)) {
        const float4 a = acc[p];
        col = mk(a.x, a.y, a.z);
    } else if (mode & RT_RESOLVE_SUM_IN) {
        col = mk(out[3 * (size_t)o + 0], out[3 * (size_t)o + 1], out[3 * (size_t)o + 2]);
    }
#pragma unroll 8
    for (int c = 0; c < nchunks; ++c) {   // the loads run ahead; the adds stay in sample order
        const float *v = slab + ((size_t)c * npix + p) * RT_SLAB_FLOATS;
        col = add(col, mk(v[0], v[1], v[2]));
    }
    if (!(mode & RT_RESOLVE_LAST)) {
        acc[p] = make_float4(col.x, col.y, col.z, 0.f);
        return;
    }
    if (!(mode & RT_RESOLVE_RAW)) col = scale(k, col);
    out[3 * (size_t)o + 0] = col.x;
    out[3 * (size_t)o + 1] = col.y;
    out[3 * (size_t)o + 2] = col.z;
}

// Diagnostic (rt_math_probe): the device's float transcendentals on n inputs, for the
// GPU tests to compare with glibc — fn 0 rt_sinf, 1 ocml sinf, 2 rt_asinf, 3 ocml asinf,
// 4 rt_atan2f(a, b), 5 ocml atan2f(a, b) (rt_libm.h; the ocml forms are what the
// megakernel used until round 5).
__global__ __launch_bounds__(256) void rt_math_probe_kernel(int fn, const float *__restrict__ a,
                                                            const float *__restrict__ b, float *__restrict__ out, int n) {
    rtl_lds_init(threadIdx.x);
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = a[i];
    float r;
    switch (fn) {
    case 0: r = rt_sinf(x); break;
    case 1: r = sinf(x); break;
    case 2: r = rt_asinf(x); break;
    case 3: r = asinf(x); break;
    case 4: r = rt_atan2f(x, b[i]); break;
    default: r = atan2f(x, b[i]); break;
    }
    out[i] = r;
}
}  // namespace

extern "C" hipError_t rt_launch_math_probe(int fn, const float *a, const float *b, float *out, int n, hipStream_t stream) {
    hipLaunchKernelGGL(rt_math_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, fn, a, b, out, n);
    return hipGetLastError();
}

// --------------------------------------------------------------- launchers
template <int kWidth, int kFeat, int kSearch>
static hipError_t launch_variant(const RtKernelArgs *a, int grid, int mode, hipStream_t stream) {
    return with_mode(mode, [=](auto count, auto prof) { return launch_one<count, prof, kWidth, kFeat, kSearch>(a, grid, stream); });
}

template <int kSearch>
static hipError_t launch_features(const RtKernelArgs *a, int grid, int mode, hipStream_t stream) {
    return with_variant(a->features, [=](auto feat) { return launch_variant<2, feat, kSearch>(a, grid, mode, stream); });
}

// the fold unit's launcher, set by that unit's static initialiser: this object links and
// runs every other variant without it (a fold launch is then an error, not another kernel)
extern "C" RtFoldLaunch rt_fold_launch;
RtFoldLaunch rt_fold_launch = nullptr;
extern "C" int rt_megakernel_has_fold(void) { return rt_fold_launch != nullptr; }
// The width-2 BVH and the flat scan run the scene's feature variant (rt_kernel_launch.h
// with_variant) with the search the scene was planned for; the wide BVHs (4, 8, compressed 8)
// run the all-feature variant from HBM.
extern "C" hipError_t rt_launch_megakernel(const RtKernelArgs *a, int grid, int mode, hipStream_t stream) {
    if (mode == RT_LAUNCH_FOLD) return rt_fold_launch ? rt_fold_launch(a, grid, stream) : hipErrorInvalidDeviceFunction;
    if (!a->scan) {
        if (a->bvh_width == 4) return launch_variant<4, RT_FEAT_ALL, 0>(a, grid, mode, stream);
        if (a->bvh_width == 8) return launch_variant<8, RT_FEAT_ALL, 0>(a, grid, mode, stream);
        if (a->bvh_width == RT_BVH_CW8) return launch_variant<RT_BVH_CW8, RT_FEAT_ALL, 0>(a, grid, mode, stream);
    }
    return with_search(search_of(a), [=](auto search) { return launch_features<search>(a, grid, mode, stream); });
}

extern "C" int rt_slab_floats(void) { return RT_SLAB_FLOATS; }

extern "C" hipError_t rt_launch_resolve(const float *slab, uint32_t npix, int nchunks, float k, float4 *acc, int mode,
                                        const uint32_t *out_index, float *out, hipStream_t stream) {
    int blocks = (int)((npix + 255) / 256);
    hipLaunchKernelGGL(rt_resolve, dim3(blocks), dim3(256), 0, stream, slab, npix, nchunks, k, acc, mode, out_index, out);
    return hipGetLastError();
}

// occupancy is asked of the all-feature kernel of the width and search
template <int kWidth, int kSearch>
static hipError_t occupancy_width(int *blocks_per_cu, int mode) {
    return with_mode(mode, [=](auto count, auto prof) {
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, rt_megakernel<count, prof, kWidth, RT_FEAT_ALL, kSearch>, RT_BLOCK, 0);
    });
}

extern "C" hipError_t rt_megakernel_occupancy(int *blocks_per_cu, int mode, int width) {
    if (width == 0) return occupancy_width<2, 2>(blocks_per_cu, mode);
    if (width == 8) return occupancy_width<8, 0>(blocks_per_cu, mode);
    if (width == RT_BVH_CW8) return occupancy_width<RT_BVH_CW8, 0>(blocks_per_cu, mode);
    return width == 4 ? occupancy_width<4, 0>(blocks_per_cu, mode) : occupancy_width<2, 0>(blocks_per_cu, mode);
}

// the compiler's count of the BVH2-in-LDS variant's static LDS bytes (0 where no HIP device answers)
template <int kFeat>
static int lds_static_of() {
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, (const void *)rt_megakernel<false, false, 2, kFeat, 1>) != hipSuccess) return 0;
    return (int)fa.sharedSizeBytes;
}

// ... and the host's estimate of it, a restatement of rt_megakernel's __shared__ declarations
// (rt_megakernel.h) for kMode 1 without the ball waves: lds_stack (one placeholder row),
// lds_slots, lds_media, lds_cam, lds_mconst, lds_pre_key / lds_pre_uv / lds_pre_cp, lds_jump,
// the one-entry lds_pool_in / lds_pool_out, lds_pool_ctl, the one-entry lds_ranvec and
// lds_perm, and 256 B of slack for their alignment
static int rt_megakernel_lds_static_bytes() {
    return (int)(4 * 64 + (RT_LDS_BLOCK / 64) * 64 * sizeof(CoopSlot) + RT_LDS_MEDIA * sizeof(MediumRec) + 6 * 16 + 16 +
                 (RT_LDS_BLOCK / 64) * RT_PRE * (8 + 8 + 8) + RT_LCG_JUMPS * 16 + 2 * 80 + 16 + 16 + 4) + 256;
}

// LDS bytes per workgroup the BVH2-in-LDS variant for `features` needs with stacks of
// `stack_depth` entries: its static arrays (the compiled kernel's own count, or the
// estimate above where no HIP device answers), its node layout (rt_lds_split: 56 KiB of
// dword planes for the media variants, 64 KiB of float4 planes otherwise) and the
// stacks — what launch_one asks for, so the host's eligibility check and the launch agree.
extern "C" long rt_lds_need_bytes(int features, int stack_depth) {
    const int v = variant_of(features);
    int stat = with_variant(features, [](auto feat) { return lds_static_of<feat>(); });
    // (the ball waves' path pools and Perlin's tables: final()'s variant only, rt_megakernel kBall)
    stat = std::max(stat, rt_megakernel_lds_static_bytes() +
                              (v == RT_FEAT_MEDIA ? (RT_BALL_POOL + RT_NORM_POOL - 2) * 80 + 255 * 16 + 767 * 4 : 0));
    const long nodes = rt_lds_split(1, v, 2) ? lds_node_bytes<1>() : lds_node_bytes<0>();
    return (long)stat + nodes + (long)RT_LDS_STACK_BYTES((long)stack_depth);
}
