// rt_colour.h — the colour of a hit's material for one lane, outside the megakernel's
// cooperative shading stage: what the first-hit feature pass (rt_features.hip) and the ray
// queries (rt_trace.hip) report as a hit's albedo.  Include after rt_device.h.
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

}  // namespace
