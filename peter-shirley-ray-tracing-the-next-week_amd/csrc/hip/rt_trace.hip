// rt_trace.hip — ray queries: the closest surface hit, or whether there is any, of rays the
// caller supplies (rt_hip.h rt_trace_rays / rt_occluded).
//
//   rt_trace<false>   one lane per ray: its closest hit under hitable_list's (t, key) rule —
//                     the search rt_features.hip runs for a camera sample, started from the
//                     ray's own t_min and t_max — and the hit's record: the descriptor's
//                     primitive and material indices, t, t * |d|, the world normal and the
//                     material's colour, as the feature pass computes them.
//   rt_trace<true>    the same search left at the lane's first accepted hit, in the kernel's own
//                     body; no record.
//
// Constant media are ignored, as in the feature pass.  Compiled with -ffp-contract=off like
// the megakernel.
#include "rt_trace.h"
#include "rt_device.h"
#include "rt_colour.h"

namespace {

template <bool kAny>
__global__ __launch_bounds__(RT_BLOCK) void rt_trace(const RtKernelArgs A, const float4 *__restrict__ rays, uint32_t n,
                                                     int moving, float time0, float time1, float4 *__restrict__ hits,
                                                     uint8_t *__restrict__ occ) {
    __shared__ uint32_t lds_stack[RT_BLOCK / 64][RT_STACK_DEPTH][64];   // [wave][depth][lane], as the megakernel's
    if (!kAny) {
        rtl_lds_init(threadIdx.x);   // rt_libm.h's sine constants (the checker and noise textures)
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t *stk = &lds_stack[wave][0][lane];
    const uint32_t gid = blockIdx.x * RT_BLOCK + threadIdx.x;
    const bool inside = gid < n;   // the lanes past the end stay in the wave, idle
    const size_t at = inside ? (size_t)gid : 0;
    const float4 q0 = rays[at * 3 + 0], q1 = rays[at * 3 + 1], q2 = rays[at * 3 + 2];
    Ray r;
    r.o = mk(q0.x, q0.y, q0.z);
    r.d = mk(q1.x, q1.y, q1.z);
    r.time = q2.x;
    const float tmin = q0.w;
    const bool sane = finite_f(r.o.x) && finite_f(r.o.y) && finite_f(r.o.z) && finite_f(r.d.x) && finite_f(r.d.y) &&
                      finite_f(r.d.z) && finite_f(r.time) && finite_f(tmin) && !(q1.w != q1.w) &&
                      !(r.d.x == 0.f && r.d.y == 0.f && r.d.z == 0.f) &&
                      (!moving || (r.time >= time0 && r.time <= time1));
    const bool valid = inside && sane;   // an invalid ray's lane idles too

    // closest surface hit (hitable_list.h:20-32) below t_max: the initial key 0 is below no
    // sphere's (its list index) and above every rect's (-1 - index), so that at t == t_max a
    // sphere is refused (sphere.h:33: t < t_max) and a rect taken (aarect.h:52: t <= t_max)
    float best_t = q1.w >= RT_FLT_MAX ? RT_FLT_MAX : q1.w;   // +inf and FLT_MAX: the reference's MAXFLOAT
    int best_key = 0;
    uint32_t best_prim = RT_NO_PRIM;
    if (!kAny) {
        lane_closest_hit<true>(A, r, tmin, valid, stk, best_t, best_key, best_prim);
    } else {
        // Occlusion keeps the search in its own body, left at the lane's first accepted hit: behind
        // lane_closest_hit the scene's scalar argument loads no longer overlap the ray's loads, 0.2 us a
        // call (profiles/r19/kernel_times.md).  A change to lane_closest_hit belongs here too.
        auto test = [&](uint32_t q) {
            int key, kind;
            const float t = prim_t<true>(A.prims, A.insts, q, r, tmin, key, kind);
            keep_closest(true, t, key, q, best_t, best_key, best_prim);
        };
        auto done = [&]() { return best_prim != RT_NO_PRIM; };
        if (A.scan || !A.has_bvh) {   // a flat-scan scene: every primitive (at most RT_SCAN_MAX)
            const uint32_t np = A.has_bvh ? A.nprims : 0u;
            if (valid)
                for (uint32_t q = 0; q < np && !done(); ++q) test(q);
        } else {
            if (valid)
                for (uint32_t q = 0; q < (uint32_t)A.nprescan && !done(); ++q) test(q);   // kept out of the BVH (scene_lower.cpp)
            const GlobalNodes gnodes{A.nodes};
            Slab sl = make_slab<0>(r, tmin);
            slab_axis(sl.ix, sl.nox);
            slab_axis(sl.iy, sl.noy);
            slab_axis(sl.iz, sl.noz);
            Counters cnt;
            uint32_t node = A.root;
            int sp = 0;
            bool trav = valid && !done();
            while (wballot(trav) != 0ull) {
                if (trav) {
                    const uint32_t pleaf = descend<2, false, 1>(gnodes, node, sl, best_t, stk, sp, cnt);
                    if (pleaf != RT_EMPTY_CHILD) {
                        const uint32_t first = RT_LEAF_FIRST(pleaf), nleaf = RT_LEAF_COUNT(pleaf);
                        for (uint32_t q = 0; q < nleaf && !done(); ++q) test(first + q);
                    }
                    if (node == RT_EMPTY_CHILD || done()) trav = false;   // the stack is empty too (descend pops)
                }
            }
        }
    }

    const bool have = valid && best_prim != RT_NO_PRIM;
    if (kAny) {
        if (inside) occ[gid] = sane ? (have ? 1 : 0) : 255;
        return;
    }
    V3 alb = mk(1.0f, 1.0f, 1.0f), nrm = mk(0, 0, 0);
    float t = 0.f, depth = 0.f;
    int prim = sane ? RT_HIT_MISS : RT_HIT_INVALID, mat = -1;
    if (have) {
        const Hit hr = hit_guides(A, r, best_prim, best_t, alb, depth);
        nrm = hr.n;
        t = best_t;
        prim = fbits(A.prims[best_prim * 4 + 1].w);   // the descriptor's list index (scene_lower.cpp to_dprim)
        mat = hr.mat;
    }
    if (inside) {
        // written once and not read again by this kernel: three whole 16-B stores, streamed
        F4v *out = (F4v *)hits + (size_t)gid * 3;
        __builtin_nontemporal_store(F4v{__int_as_float(prim), __int_as_float(mat), t, depth}, out + 0);
        __builtin_nontemporal_store(F4v{nrm.x, nrm.y, nrm.z, alb.x}, out + 1);
        __builtin_nontemporal_store(F4v{alb.y, alb.z, 0.f, 0.f}, out + 2);
    }
}

}  // namespace

extern "C" hipError_t rt_launch_trace(const RtKernelArgs *a, const void *rays, uint32_t n, int moving, float time0, float time1,
                                      int any, void *hits, uint8_t *occ, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n >= 0x80000000u || a->bvh_width != 2 || !rays || (any ? !occ : !hits)) return hipErrorInvalidValue;
    const unsigned blocks = (n + RT_BLOCK - 1) / RT_BLOCK;
    if (any)
        hipLaunchKernelGGL(rt_trace<true>, dim3(blocks), dim3(RT_BLOCK), 0, stream, *a, (const float4 *)rays, n, moving, time0,
                           time1, (float4 *)nullptr, occ);
    else
        hipLaunchKernelGGL(rt_trace<false>, dim3(blocks), dim3(RT_BLOCK), 0, stream, *a, (const float4 *)rays, n, moving, time0,
                           time1, (float4 *)hits, (uint8_t *)nullptr);
    return hipGetLastError();
}

// the unit announces its launcher to the host when it is linked in
static const bool trace_unit_linked = (rt_trace_launch = RtTraceLaunch{rt_launch_trace}, true);
