// rt_kernel_fold.hip — the right-fold variants of the megakernel (RT_FLAG_RIGHT_FOLD,
// rt_kernel.hip kFold) as a translation unit of their own: rt_kernel.hip's kernel and
// launchers, instantiated for the fold variants only, so that the two units compile side
// by side and the parity mode adds nothing to the library's build time.
#define MEGAKERNEL_FOLD_UNIT 1
#include "rt_kernel.hip"
