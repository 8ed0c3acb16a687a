// rt_kernel_fold.hip — the right-fold variants of the megakernel (RT_FLAG_RIGHT_FOLD,
// rt_megakernel.h kFold) as a translation unit of their own: the kernel template instantiated
// for the fold variant of each width-2 one (each feature set x search mode, plain mode only),
// so that the units compile side by side and the parity mode adds nothing to the library's
// build time.
#include "rt_kernel_launch.h"

template <int kSearch>
static hipError_t launch_fold(const RtKernelArgs *a, int grid, hipStream_t stream) {
    return with_variant(a->features, [=](auto feat) { return launch_one<false, false, 2, feat, kSearch, true>(a, grid, stream); });
}

// plain mode, width 2 (capi_render.cpp checks both)
extern "C" hipError_t rt_launch_megakernel_fold(const RtKernelArgs *a, int grid, hipStream_t stream) {
    if (a->bvh_width != 2) return hipErrorInvalidValue;
    return with_search(search_of(a), [=](auto search) { return launch_fold<search>(a, grid, stream); });
}
// the unit announces its launcher to rt_launch_megakernel when it is linked in
extern "C" RtFoldLaunch rt_fold_launch;
static const bool fold_unit_linked = (rt_fold_launch = rt_launch_megakernel_fold, true);
