// rt_kernel_rays.hip — the ray-source variants of the megakernel (rt_hip.h rt_radiance_rays,
// rt_megakernel.h kRays) as a translation unit of their own, like
// rt_kernel_fold.hip: the kernel template instantiated for RT_FEAT_ALL, width 2, plain mode
// and the three search modes with the ray source, so that the unit compiles beside the others
// and leaves every other variant's code object as it was.
#include "rt_kernel_launch.h"

extern "C" hipError_t rt_launch_megakernel_rays(const RtKernelArgs *a, int grid, hipStream_t stream) {
    if (a->bvh_width != 2 || !a->rays || !a->radiance) return hipErrorInvalidValue;
    return with_search(search_of(a), [=](auto search) { return launch_one<false, false, 2, RT_FEAT_ALL, search, false, true>(a, grid, stream); });
}
extern "C" hipError_t rt_megakernel_rays_plan(int search, int stack_depth, int *blocks_per_cu, int *block_threads) {
    search &= 3;
    if (search == 3) return hipErrorInvalidValue;
    *block_threads = rt_mega_block(search | 8);
    // a property of the code objects, queried once per process (value + 1; 0: not yet): the LDS
    // variant's static LDS bytes, the others' resident workgroups per CU
    static std::atomic<int> known[3];
    int v = known[search].load(std::memory_order_acquire) - 1;
    if (v < 0) {
        const hipError_t e = with_search(search, [&v](auto s) {
            auto *k = rt_megakernel<false, false, 2, RT_FEAT_ALL, s | 8>;
            if (s != 1) return hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k, RT_BLOCK, 0);
            hipFuncAttributes fa;
            const hipError_t e = hipFuncGetAttributes(&fa, (const void *)k);
            v = (int)fa.sharedSizeBytes;
            return e;
        });
        if (e != hipSuccess) return e;
        known[search].store(v + 1, std::memory_order_release);
    }
    if (search == 1) {   // one workgroup per CU, if its LDS fits (what launch_one asks for)
        const long need = (long)v + (long)lds_node_bytes<rt_lds_split(1, RT_FEAT_ALL, 2)>() + (long)RT_LDS_STACK_BYTES((long)stack_depth);
        *blocks_per_cu = need <= RT_LDS_BUDGET ? 1 : 0;
    } else {
        *blocks_per_cu = v;
    }
    return hipSuccess;
}
// the unit announces its launchers to capi_radiance.cpp when it is linked in
static const bool rays_unit_linked = (rt_rays_launch = RtRaysLaunch{rt_launch_megakernel_rays, rt_megakernel_rays_plan}, true);
