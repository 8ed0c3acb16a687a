// rt_kernel_knobs.hip — tests/test_device_knobs.py's unit, not part of the library: a
// device-only build of final()'s variant (BVH2 in LDS, media) and cornell_box's (flat scan,
// instances), with a non-default value of one compile-time knob — seconds instead of the whole
// variant set's minute — so no knob value goes uncompiled.
#include "rt_megakernel.h"

namespace {
template __global__ void rt_megakernel<false, false, 2, RT_FEAT_MEDIA, 1>(RtKernelArgs);
template __global__ void rt_megakernel<false, false, 2, RT_FEAT_INST, 2>(RtKernelArgs);
}  // namespace
