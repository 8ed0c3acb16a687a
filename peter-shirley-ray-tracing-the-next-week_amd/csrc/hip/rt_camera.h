// rt_camera.h — the per-lane statement of the reference's camera (camera.h:41-56) that the side
// units share: rt_features.hip builds its samples' rays with it, rt_lens.hip the records of
// RT_LENS_PERSPECTIVE.  Device code; included after rt_device.h.
#pragma once
#include "rt_device.h"

namespace {

// camera.h:41-56 for one sample, sequentially per lane: the draws, in order, are the two
// jitters, the lens disk's candidates (two draws each, until one is accepted) and the time.
// kCount: `rejected` receives the candidates refused (the sample has spent 5 + 2 * rejected
// draws); without it the counter is no part of the code: rt_features' kernel is, instruction for
// instruction, what it was with the statement in its own file.
template <bool kCount>
__device__ __forceinline__ Ray camera_ray_t(const RtKernelArgs &A, int x, int j, uint32_t sample, uint64_t skey,
                                            uint32_t &rejected) {
    Rng g;
    g.start(sample_key(skey, (uint32_t)j * (uint32_t)A.nx + (uint32_t)x, sample), false);   // uint32_t: no signed overflow
    const float cu = div_rn((float)((double)x + g.next()), (float)A.nx, A.rnx);   // main.cpp:305-306
    const float cv = div_rn((float)((double)j + g.next()), (float)A.ny, A.rny);
    V3 disk;
    if (kCount) rejected = 0;
    for (;;) {   // camera.h:6-12
        const bool ok = DiskCand()(g.x, disk);
        g.skip2();
        if (ok) break;
        if (kCount) ++rejected;
    }
    CamView C;
    C.llc = mk(A.llc[0], A.llc[1], A.llc[2]); C.hor = mk(A.hor[0], A.hor[1], A.hor[2]);
    C.ver = mk(A.ver[0], A.ver[1], A.ver[2]); C.org = mk(A.org[0], A.org[1], A.org[2]);
    C.cu = mk(A.cu[0], A.cu[1], A.cu[2]); C.cv = mk(A.cv[0], A.cv[1], A.cv[2]);
    C.t0 = A.ct0; C.t1 = A.ct1; C.lens = A.lens;
    const V3 rd = scale(C.lens, disk);
    const V3 offset = add(scale(rd.x, C.cu), scale(rd.y, C.cv));
    const float span = C.t1 - C.t0;   // camera.h:54; a closed shutter consumes the draw unused
    double u = 0.0;
    if (span != 0.0f) u = g.next(); else g.skip();
    Ray r;
    r.time = (float)((double)C.t0 + u * (double)span);
    r.d = sub(sub(add(add(C.llc, scale(cu, C.hor)), scale(cv, C.ver)), C.org), offset);
    r.o = add(C.org, offset);
    return r;
}
__device__ __forceinline__ Ray camera_ray(const RtKernelArgs &A, int x, int j, uint32_t sample, uint64_t skey) {
    uint32_t none = 0;
    return camera_ray_t<false>(A, x, j, sample, skey, none);
}
__device__ __forceinline__ Ray camera_ray(const RtKernelArgs &A, int x, int j, uint32_t sample, uint64_t skey,
                                          uint32_t &rejected) {
    return camera_ray_t<true>(A, x, j, sample, skey, rejected);
}

}  // namespace
