// rt_kernel_rays.hip — the ray-source variants of the megakernel (rt_hip.h rt_radiance_rays,
// rt_kernel.hip kRays) as a translation unit of their own, like
// rt_kernel_fold.hip: rt_kernel.hip's kernel and launch_one, instantiated for RT_FEAT_ALL,
// width 2 and the three search modes with the ray source, so that the unit compiles beside the
// others and leaves every other variant's code object as it was.
#define MEGAKERNEL_RAYS_UNIT 1
#include "rt_kernel.hip"
