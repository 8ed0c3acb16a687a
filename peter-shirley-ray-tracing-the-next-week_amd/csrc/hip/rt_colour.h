// rt_colour.h — one lane's work outside the megakernel's cooperative stages, shared by the first-hit
// feature pass (rt_features.hip) and the ray queries (rt_trace.hip): the closest-hit search and what
// both report of a hit, its material's colour, normal and distance.  Include after rt_device.h.
#pragma once
#include "rt_device.h"

namespace {

// perlin.h:64-74 for one lane, the octaves in the reference's order (coop_turb's values:
// octave k is noise(q * 2^k) weighted 2^-k, both exact)
__device__ __forceinline__ float turb_lane(const RtKernelArgs &A, V3 q) {
    float acc = 0.f, weight = 1.0f;
#pragma unroll 1
    for (int k = 0; k < 7; ++k) {
        const float s = (float)(1u << k);
        acc += weight * perlin_noise(A.ranvec, A.perm, mk(q.x * s, q.y * s, q.z * s));
        weight = (float)((double)weight * 0.5);
    }
    return fabsf(acc);
}

// The hit material's colour: its texture's value for the textured kinds (texture.h), the
// albedo of a metal, white for a dielectric.
__device__ __forceinline__ V3 material_colour(const RtKernelArgs &A, const Hit &hr) {
    const float4 m0 = A.mats[hr.mat * 2 + 0], m1 = A.mats[hr.mat * 2 + 1];
    const int kind = fbits(m0.x);
    if (kind == RT_MAT_METAL) return mk(m1.x, m1.y, m1.z);
    if (kind == RT_MAT_DIELECTRIC) return mk(1.0f, 1.0f, 1.0f);
    if (fbits(m1.w) & 2) return mk(m1.x, m1.y, m1.z);   // a constant texture, resolved by the host
    float4 t0, t1;
    const int tkind = tex_leaf<true>(A, fbits(m0.y), hr.p, t0, t1);
    if (tkind != RT_TEX_NOISE) return tex_value_leaf<true>(A, tkind, t0, t1, hr.u, hr.v);
    const float nscale = t0.w;                                                  // texture.h:52-56
    const float sv = 1 + rt_sinf(nscale * hr.p.x + 5 * turb_lane(A, scale(nscale, hr.p)));
    const float h = 0.5f * 1;
    return mk(sv * h, sv * h, sv * h);
}

#define RT_NO_PRIM 0xFFFFFFFFu

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// make_slab's planes for an axis the ray does not move along (or barely: a reciprocal that
// overflows) are plane * inf - origin * inf: NaN, or an infinity whose sign says nothing about
// whether the origin lies between the planes, and a box the ray runs through would be culled.
// With -o/d = NaN both planes are NaN on that axis, which box_span's min / max ignore: the
// axis culls nothing, and the primitive tests decide.
__device__ __forceinline__ void slab_axis(const F2 &inv, F2 &no) {
    const float q = finite_f(inv.x) && finite_f(no.x) ? no.x : __builtin_nanf("");
    no = F2{q, q};
}

// The closest surface hit of one lane's ray under hitable_list's (t, key) rule (hitable_list.h:20-32),
// from the caller's (best_t, best_key, best_prim): the upper end of the search and the key a tie at
// it is weighed against.  `valid` off: the lane idles in its wave; `stk`: its column of the wave's LDS
// stack.  kGuardAxes: slab_axis on the three axes, for rays a caller supplies.  A by value: with a
// reference the feature pass of final() at 1 spp measured 0.6 to 1.0 % slower (profiles/r19).
template <bool kGuardAxes>
__device__ __forceinline__ void lane_closest_hit(const RtKernelArgs A, const Ray &r, float tmin, bool valid, uint32_t *stk,
                                                 float &best_t, int &best_key, uint32_t &best_prim) {
    auto test = [&](uint32_t q) {
        int key, kind;
        const float t = prim_t<true>(A.prims, A.insts, q, r, tmin, key, kind);
        keep_closest(true, t, key, q, best_t, best_key, best_prim);
    };
    if (A.scan || !A.has_bvh) {   // a flat-scan scene: every primitive (at most RT_SCAN_MAX)
        const uint32_t n = A.has_bvh ? A.nprims : 0u;
        if (valid)
            for (uint32_t q = 0; q < n; ++q) test(q);
        return;
    }
    if (valid)
        for (uint32_t q = 0; q < (uint32_t)A.nprescan; ++q) test(q);   // kept out of the BVH (scene_lower.cpp)
    const GlobalNodes gnodes{A.nodes};
    Slab sl = make_slab<0>(r, tmin);
    if (kGuardAxes) {
        slab_axis(sl.ix, sl.nox);
        slab_axis(sl.iy, sl.noy);
        slab_axis(sl.iz, sl.noz);
    }
    Counters cnt;
    uint32_t node = A.root;
    int sp = 0;
    bool trav = valid;
    while (wballot(trav) != 0ull) {
        if (trav) {
            const uint32_t pleaf = descend<2, false, 1>(gnodes, node, sl, best_t, stk, sp, cnt);
            if (pleaf != RT_EMPTY_CHILD) {
                const uint32_t first = RT_LEAF_FIRST(pleaf), nleaf = RT_LEAF_COUNT(pleaf);
                for (uint32_t q = 0; q < nleaf; ++q) test(first + q);
            }
            if (node == RT_EMPTY_CHILD) trav = false;   // the stack is empty too (descend pops)
        }
    }
}

// What both units report of the hit at t on primitive `prim`: the record (returned: its normal,
// and its material index for the ray queries), the material's colour and the distance t * |d|.
__device__ __forceinline__ Hit hit_guides(const RtKernelArgs &A, const Ray &r, uint32_t prim, float t, V3 &alb, float &depth) {
    const Hit hr = prim_record<true, true>(A.prims, A.insts, A.mats, prim, r, t);
    alb = material_colour(A, hr);
    depth = t * len(r.d);
    return hr;
}

}  // namespace
