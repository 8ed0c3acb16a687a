// rt_kernel_launch.h — how the megakernel's units (rt_kernel.hip, rt_kernel_fold.hip,
// rt_kernel_rays.hip) choose and launch a variant of rt_megakernel (rt_megakernel.h): the
// launch itself and one dispatch per runtime choice — feature variant, search mode,
// plain / count / profile — each written here once.  A dispatch hands its choice to a
// callable as a compile-time constant (std::integral_constant converts to the template
// argument); a unit instantiates exactly the kernels its callables name.
#pragma once
#include <atomic>
#include <type_traits>

#include "rt_megakernel.h"

template <int k>
using RtInt = std::integral_constant<int, k>;

template <bool kCount, bool kProf, int kWidth, int kFeat, int kLds, bool kFold = false, bool kRays = false>
static hipError_t launch_one(const RtKernelArgs *a, int grid, hipStream_t stream) {
    auto *k = rt_megakernel<kCount, kProf, kWidth, kFeat, kLds | (kFold ? 4 : 0) | (kRays ? 8 : 0)>;
    size_t dyn = 0;
    if (kLds == 1) {
        // the variant's node layout (rt_megakernel's kSplit): dword planes need 56 KiB, float4 planes 64
        dyn = lds_node_bytes<rt_lds_split(kLds, kFeat, kWidth)>() + RT_LDS_STACK_BYTES(a->stack_depth);
        // Dynamic LDS above the default limit: the attribute (the most any scene can
        // ask for) is set once per device and variant, recorded in an atomic bit mask
        // (thread-safe; calling hipFuncSetAttribute before every launch cost ~0.6 ms
        // of host time per render step).
        static std::atomic<uint64_t> done{0};
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const uint64_t bit = 1ull << (dev & 63);
        if (!(done.load(std::memory_order_acquire) & bit)) {
            // the most the budget leaves beside this variant's own static arrays
            hipFuncAttributes fa;
            e = hipFuncGetAttributes(&fa, (const void *)k);
            if (e != hipSuccess) return e;
            e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    RT_LDS_BUDGET - (int)fa.sharedSizeBytes);
            if (e != hipSuccess) return e;
            done.fetch_or(bit, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(k, dim3(grid), dim3(rt_mega_block(kLds | (kRays ? 8 : 0))), dyn, stream, *a);
    return hipGetLastError();
}

// The compiled feature variants of the width-2 kernels, and which of them runs a scene's
// features — the table: media only (final(), and scenes with no feature), instances
// (cornell_box), instances + media (cornell_smoke), checker + pre-scan without media (the
// random scenes; checker alone runs it too), every feature (any scene).  f is called with
// the variant's RT_FEAT_* as an RtInt; a new variant is one line here.
template <class F>
static auto with_variant(int features, F f) {
    switch (features) {
    case 0:
    case RT_FEAT_MEDIA: return f(RtInt<RT_FEAT_MEDIA>{});
    case RT_FEAT_INST: return f(RtInt<RT_FEAT_INST>{});
    case RT_FEAT_INST | RT_FEAT_MEDIA: return f(RtInt<RT_FEAT_INST | RT_FEAT_MEDIA>{});
    case RT_FEAT_CHECKER:
    case RT_FEAT_CHECKER | RT_FEAT_PRESCAN: return f(RtInt<RT_FEAT_CHECKER | RT_FEAT_PRESCAN>{});
    default: return f(RtInt<RT_FEAT_ALL>{});
    }
}
static int variant_of(int features) {
    return with_variant(features, [](auto feat) { return (int)feat; });
}

// The closest-hit search of a launch (rt_megakernel's kMode & 3): 2 the flat scan, 1 the BVH2
// in LDS, 0 the BVH in HBM.  f is called with it as an RtInt.
static int search_of(const RtKernelArgs *a) { return a->scan ? 2 : a->lds_nodes ? 1 : 0; }
template <class F>
static auto with_search(int search, F f) {
    if (search == 2) return f(RtInt<2>{});
    return search == 1 ? f(RtInt<1>{}) : f(RtInt<0>{});
}

// The launch modes of rt_kernel.h (0 plain, 1 count, 2 profile): f is called with
// rt_megakernel's kCount and kProf as bool constants.
template <class F>
static hipError_t with_mode(int mode, F f) {
    if (mode == 1) return f(std::true_type{}, std::false_type{});
    if (mode == 2) return f(std::false_type{}, std::true_type{});
    if (mode != 0) return hipErrorInvalidValue;
    return f(std::false_type{}, std::false_type{});
}
