// scene_lower.cpp — from a scene descriptor to the image of the device's arrays: descriptor
// validation, the pre-scan selection, the BVH, the flat-scan groups, the medium cell and the
// device records (rt_layout.h).  No HIP here: rt_scene_create (capi_scene.cpp) uploads the image.
#include "scene_lower.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

#include "../rt_layout.h"
#include "bvh.h"

namespace rtnw {
namespace {

int fail(int code, const std::string &msg) { return rt_internal_fail(code, msg); }

// stage() appends an array to the image at a 256-B aligned offset and returns the offset.
// An empty array is staged as one zeroed 256-B sentinel: no scene pointer the kernel
// receives is ever null, so a load the compiler speculates out of its branch (e.g. a
// texture record read for lanes that have none) reads zeros instead of faulting on an
// empty scene (edge_empty's illegal access).
template <class T>
size_t stage(std::vector<uint8_t> &image, const std::vector<T> &v) {
    const size_t off = (image.size() + 255) & ~(size_t)255;
    const size_t bytes = v.empty() ? std::max<size_t>(256, sizeof(T)) : v.size() * sizeof(T);
    image.resize(off + bytes, 0);
    if (!v.empty()) std::memcpy(image.data() + off, v.data(), bytes);
    return off;
}

int ibits(float f) { int i; std::memcpy(&i, &f, 4); return i; }
float fbits(int i) { float f; std::memcpy(&f, &i, 4); return f; }

// Pre-scan (BVH scenes): the largest primitives — box area >= RTNW_PRESCAN_AREA
// (default 10 %) of the scene box's, at most RT_PRESCAN_MAX — stay out of the BVH
// and are tested in lockstep before every descent (rt_megakernel.h): a primitive
// whose box spans the scene sits at the BVH's root and nearly every ray tests it
// anyway.  random_motion's ground sphere: c3 55.57 -> 52.15 ms; final()'s six
// largest (0.5 %: 2-3 % each) 59.08 -> 62.27 ms, so the threshold leaves them in
// the BVH.  RTNW_PRESCAN=0 keeps every primitive in the BVH.
void select_prescan(const rt_scene_desc *d, std::vector<int> &big, std::vector<int> &rest) {
    bool want = d->nprims > RT_SCAN_MAX;
    if (const char *e = std::getenv("RTNW_PRESCAN")) want = want && std::atoi(e) != 0;
    double frac = 0.10;
    if (const char *e = std::getenv("RTNW_PRESCAN_AREA")) frac = std::atof(e);
    std::vector<double> area(d->nprims, 0.0);
    if (want) {
        double slo[3] = {1e300, 1e300, 1e300}, shi[3] = {-1e300, -1e300, -1e300};
        for (int i = 0; i < d->nprims; i++) {
            float lo[3], hi[3];
            prim_bounds(d->prims[i], d->instances, d->time0, d->time1, lo, hi);
            for (int k = 0; k < 3; k++) { slo[k] = std::min(slo[k], (double)lo[k]); shi[k] = std::max(shi[k], (double)hi[k]); }
            const double x = (double)hi[0] - lo[0], y = (double)hi[1] - lo[1], z = (double)hi[2] - lo[2];
            area[i] = 2 * (x * y + y * z + z * x);
        }
        const double x = shi[0] - slo[0], y = shi[1] - slo[1], z = shi[2] - slo[2];
        const double sa = 2 * (x * y + y * z + z * x);
        std::vector<int> cand;
        for (int i = 0; i < d->nprims; i++) if (area[i] >= frac * sa) cand.push_back(i);
        std::stable_sort(cand.begin(), cand.end(), [&](int p, int q) { return area[p] > area[q]; });
        if ((int)cand.size() > RT_PRESCAN_MAX) cand.resize(RT_PRESCAN_MAX);
        std::sort(cand.begin(), cand.end());
        big = cand;
    }
    std::vector<char> is_big(d->nprims, 0);
    for (int i : big) is_big[i] = 1;
    for (int i = 0; i < d->nprims; i++) if (!is_big[i]) rest.push_back(i);
}

// The BVH over the primitives `rest`; its leaf order then names input primitives, the
// pre-scanned ones (`big`) first, with the leaf refs shifted past them.
BvhResult build_shifted_bvh(const rt_scene_desc *d, const std::vector<int> &big, const std::vector<int> &rest) {
    std::vector<rt_prim> rest_prims;
    rest_prims.reserve(rest.size());
    for (int i : rest) rest_prims.push_back(d->prims[i]);
    BvhResult bvh = build_bvh(rest_prims.data(), (int)rest_prims.size(), d->instances, d->time0, d->time1);
    for (int &o : bvh.order) o = rest[o];
    if (!big.empty()) {
        const uint32_t K = (uint32_t)big.size();
        auto shift = [&](uint32_t &ref) {
            if (ref != RT_EMPTY_CHILD && (ref & RT_LEAF_BIT))
                ref = RT_LEAF_REF(RT_LEAF_FIRST(ref) + K, RT_LEAF_COUNT(ref));
        };
        bvh.for_each_ref(shift);
        shift(bvh.root);
        bvh.order.insert(bvh.order.begin(), big.begin(), big.end());
    }
    return bvh;
}

// Flat scan instead of the BVH for scenes of at most RT_SCAN_MAX primitives
// (rt_layout.h rt_dgroup; RTNW_SCAN=0 keeps the BVH): primitives ordered by
// instance chain (list order within a chain), one group per chain.
// Returns whether the scene is scanned; `order` and `groups` are set only then.
bool flat_scan(const rt_scene_desc *d, int bvh_width, std::vector<int> &order, std::vector<rt_dgroup> &groups) {
    bool want = true;
    if (const char *e = std::getenv("RTNW_SCAN")) want = std::atoi(e) != 0;
    if (!(want && d->nprims >= 1 && d->nprims <= RT_SCAN_MAX && bvh_width == 2)) return false;
    order.resize(d->nprims);
    for (int i = 0; i < d->nprims; i++) order[i] = i;
    // by chain, then by kind within a chain (rt_dgroup: one loop per kind)
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        const rt_prim &px = d->prims[x], &py = d->prims[y];
        return px.instance != py.instance ? px.instance < py.instance : px.kind < py.kind;
    });
    for (int i = 0; i < d->nprims; i++) {
        const rt_prim &pr = d->prims[order[i]];
        float lo[3], hi[3];
        prim_bounds(pr, d->instances, d->time0, d->time1, lo, hi);
        if (groups.empty() || groups.back().instance != pr.instance) {
            rt_dgroup g{};
            g.first = i;
            g.instance = pr.instance;
            g.bx[0] = lo[0]; g.bx[1] = hi[0]; g.bx[2] = lo[1]; g.bx[3] = hi[1];
            g.bz[0] = lo[2]; g.bz[1] = hi[2];
            groups.push_back(g);
        }
        rt_dgroup &g = groups.back();
        // scan_group (rt_device.h) walks a group's runs in the enum order of the kinds,
        // from 8-bit counts packed at 8 * kind in `kinds` (yz rects in nyz)
        static_assert(RT_PRIM_SPHERE == 0 && RT_PRIM_MOVING_SPHERE == 1 && RT_PRIM_XY_RECT == 2 &&
                          RT_PRIM_XZ_RECT == 3 && RT_PRIM_YZ_RECT == 4,
                      "rt_dgroup.kinds packs the primitive kinds 0..3 by their enum value");
        static_assert(RT_SCAN_MAX < 256, "rt_dgroup.kinds holds 8-bit counts");
        g.count++;
        if (pr.kind == RT_PRIM_YZ_RECT) g.nyz++;
        else g.kinds += 1 << (8 * pr.kind);     // count <= RT_SCAN_MAX < 256 per kind
        g.bx[0] = std::min(g.bx[0], lo[0]); g.bx[1] = std::max(g.bx[1], hi[0]);
        g.bx[2] = std::min(g.bx[2], lo[1]); g.bx[3] = std::max(g.bx[3], hi[1]);
        g.bz[0] = std::min(g.bz[0], lo[2]); g.bz[1] = std::max(g.bz[1], hi[2]);
    }
    return true;
}

// Medium cell (BVH modes; rt_megakernel.h stages 3 and 6): a path inside a dense medium
// scatters there segment after segment (final(): a third of all segments start inside
// the subsurface sphere), and every segment's closest-hit search starts from the BVH
// root.  For one medium bounded by a sphere (c, R) — the densest such — the primitives
// whose boxes reach within R + m of c (m = R / 64 + 1e-3 |c|) are listed (at most
// RT_CELL_MAX, appended to the device primitives as copies: same record, same key); a
// ray starting within R + m / 2 of c tests just them, and if the nearest lies before the
// ray leaves that ball, no other primitive (all are outside R + m) can be nearer: the
// search ends there with the same (t, key) winner as the full one.  The kernel's ball
// waves gather such paths (RtKernelArgs.ball_waves).  RTNW_CELL=0 disables it.
void medium_cell(const rt_scene_desc *d, SceneInfo &s, std::vector<int> &order) {
    bool want = true;
    if (const char *e = std::getenv("RTNW_CELL")) want = std::atoi(e) != 0;
    double best_density = -1;
    std::vector<int> cell;
    for (int i = 0; want && i < d->nmedia; i++) {
        const rt_medium &m = d->media[i];
        if (m.boundary_count != 1) continue;
        const rt_prim &bp = d->boundary_prims[m.boundary_first];
        if (bp.kind != RT_PRIM_SPHERE || bp.instance >= 0 || !(m.density > best_density)) continue;
        const double c[3] = {bp.p[0], bp.p[1], bp.p[2]}, R = std::fabs((double)bp.p[3]);
        const double cmax = std::max(std::fabs(c[0]), std::max(std::fabs(c[1]), std::fabs(c[2])));
        const double mg = R / 64 + 1e-3 * cmax, reach = R + mg;
        if (!(R > 0) || !std::isfinite(reach)) continue;
        std::vector<int> near;
        for (int q = 0; q < d->nprims && (int)near.size() <= RT_CELL_MAX; q++) {
            float lo[3], hi[3];
            prim_bounds(d->prims[q], d->instances, d->time0, d->time1, lo, hi);
            double d2 = 0;
            for (int k = 0; k < 3; k++) {
                const double v = std::max(std::max((double)lo[k] - c[k], c[k] - (double)hi[k]), 0.0);
                d2 += v * v;
            }
            if (!(d2 > reach * reach)) near.push_back(q);   // (a NaN box counts as near)
        }
        if (near.empty() || (int)near.size() > RT_CELL_MAX) continue;
        best_density = m.density;
        s.cell_n = (int)near.size();
        for (int k = 0; k < 3; k++) s.cell_c[k] = (float)c[k];
        const double rk = R + mg / 2, rin = R * (1 - 1.0 / 1024);
        s.cell_r2 = (float)(rk * rk);
        s.cell_rin2 = (float)(rin * rin);   // (routing only: rays nearer the surface count as inside when heading in)
        cell = near;
    }
    s.cell_first = (int)order.size();
    for (int q : cell) order.push_back(q);
}

// Dense media (mean free path below half the boundary sphere's radius: final()'s
// subsurface sphere, not its scene-wide fog): paths that enter one random-walk to the
// depth cap, so the job lists the pixels whose primary rays enter one first and the
// kernel claims all their samples before the others' (prepare_job): the launch's
// last claims then hold few such paths, whose latency chains are its drain.
std::vector<float> dense_balls(const rt_scene_desc *d) {
    std::vector<float> balls;
    for (int i = 0; i < d->nmedia; i++) {
        const rt_medium &m = d->media[i];
        if (m.boundary_count != 1 || !(m.density > 0)) continue;
        const rt_prim &bp = d->boundary_prims[m.boundary_first];
        const float R = std::fabs(bp.p[3]);
        if (bp.kind != RT_PRIM_SPHERE || bp.instance >= 0 || !(1.0f / m.density < 0.5f * R)) continue;
        balls.insert(balls.end(), {bp.p[0], bp.p[1], bp.p[2], R});
    }
    return balls;
}

// ---------------------------------------------------------------- record conversion
rt_dprim to_dprim(const rt_prim &p, int order) {
    rt_dprim d{};
    const float *q = p.p;
    switch (p.kind) {
    case RT_PRIM_SPHERE:
        d.g0[0] = q[0]; d.g0[1] = q[1]; d.g0[2] = q[2]; d.g0[3] = q[3];
        break;
    case RT_PRIM_MOVING_SPHERE:
        // center(t) = c0 + ((t - t0) / (t1 - t0)) * (c1 - c0): the two differences
        // are float subtractions of the reference (sphere.h:82), computed once here.
        d.g0[0] = q[0]; d.g0[1] = q[1]; d.g0[2] = q[2]; d.g0[3] = q[8];
        d.g1[0] = q[3] - q[0]; d.g1[1] = q[4] - q[1]; d.g1[2] = q[5] - q[2]; d.g1[3] = q[6];
        d.g2[0] = q[7] - q[6];
        break;
    default:   // rects (k goes to m[1])
        d.g0[0] = q[0]; d.g0[1] = q[1]; d.g0[2] = q[2]; d.g0[3] = q[3];
        break;
    }
    d.m[0] = p.kind | (p.flip ? 1 << 8 : 0) | (p.material << 9);
    if (p.kind >= RT_PRIM_XY_RECT) {
        d.m[1] = ibits(q[4]);   // rect plane k
    } else {                    // spheres: RN(1/radius) for the normal's div_rn, 0 if not a normal float
        const float y = 1.0f / d.g0[3];
        d.m[1] = (std::isnormal(y)) ? ibits(y) : 0;
    }
    d.m[2] = p.instance;
    d.m[3] = order;
    return d;
}

std::vector<rt_dmaterial> to_dmaterials(const rt_scene_desc *d, SceneInfo &s) {
    // a material whose texture tree reaches an image needs the hit's (u, v)
    auto reads_uv = [&](int t) {
        std::vector<int> st{t};
        while (!st.empty()) {
            const int x = st.back();
            st.pop_back();
            if (x < 0) continue;
            if (d->textures[x].kind == RT_TEX_IMAGE) return true;
            if (d->textures[x].kind == RT_TEX_CHECKER) { st.push_back(d->textures[x].even); st.push_back(d->textures[x].odd); }
        }
        return false;
    };
    std::vector<rt_dmaterial> mats(d->nmaterials);
    for (int i = 0; i < d->nmaterials; i++) {
        const rt_material &m = d->materials[i];
        rt_dmaterial &o = mats[i];
        o.kind = m.kind;
        o.texture = m.texture;
        o.fuzz = m.fuzz;
        o.ref_idx = m.ref_idx;
        for (int k = 0; k < 3; k++) o.albedo[k] = m.albedo[k];
        if (m.kind == RT_MAT_DIELECTRIC) {
            // a dielectric has no albedo (material.h:99): its slots carry the per-material
            // constants of material.h:103-116 in the reference's float/double arithmetic
            const float r0 = (1 - m.ref_idx) / (1 + m.ref_idx);
            o.albedo[0] = (float)(1.0 / (double)m.ref_idx);   // ni_over_nt entering
            o.albedo[1] = r0 * r0;                            // schlick's r0^2
            o.albedo[2] = m.ref_idx * m.ref_idx;              // ref_idx^2 of the exit cosine
        }
        o.flags = (m.texture >= 0 && reads_uv(m.texture)) ? 1 : 0;
        s.has_uv |= o.flags != 0;
        // a textured material (lambertian, isotropic, diffuse_light) whose texture is a
        // constant: its color in the unused albedo slots, flag 2 (shade_begin then reads
        // no texture record: one dependent load fewer per shade)
        const bool textured = m.kind == RT_MAT_LAMBERTIAN || m.kind == RT_MAT_ISOTROPIC || m.kind == RT_MAT_DIFFUSE_LIGHT;
        if (textured && m.texture >= 0 && m.texture < d->ntextures &&
            d->textures[m.texture].kind == RT_TEX_CONSTANT) {
            for (int k = 0; k < 3; k++) o.albedo[k] = d->textures[m.texture].color[k];
            o.flags |= 2;
        }
        s.has_specular |= m.kind == RT_MAT_METAL || m.kind == RT_MAT_DIELECTRIC;
    }
    return mats;
}

// The ball waves' fused in-ball step (rt_megakernel.h stage 3) scatters a path at a medium without
// the shading stage: it is enabled only where that stage would do nothing else for any medium of
// the scene — each medium's material an isotropic whose texture is the constant resolved above
// (flag 2; final()'s two) — and the scene has a medium cell.  The constants go to the kernel
// arguments in list order.
void ball_fast_media(const rt_scene_desc *d, const std::vector<rt_dmaterial> &mats, SceneInfo &s) {
    s.ball_fast = false;
    if (s.cell_n <= 0 || d->nmedia < 1 || d->nmedia > 2) return;
    for (int i = 0; i < d->nmedia; i++) {
        const int m = d->media[i].material;
        if (m < 0 || m >= (int)mats.size() || mats[m].kind != RT_MAT_ISOTROPIC || !(mats[m].flags & 2)) return;
    }
    for (int i = 0; i < d->nmedia; i++)
        for (int k = 0; k < 3; k++) s.ball_alb[i][k] = mats[d->media[i].material].albedo[k];
    s.ball_fast = true;
}

std::vector<rt_dtexture> to_dtextures(const rt_scene_desc *d, SceneInfo &s) {
    std::vector<rt_dtexture> texs(d->ntextures);
    for (int i = 0; i < d->ntextures; i++) {
        const rt_texture &t = d->textures[i];
        rt_dtexture &o = texs[i];
        o.kind = t.kind;
        o.even = t.even;
        o.odd = t.odd;
        s.has_checker |= t.kind == RT_TEX_CHECKER;
        o.scale = t.scale;
        for (int k = 0; k < 3; k++) o.color[k] = t.color[k];
        if (t.kind == RT_TEX_IMAGE) {   // (kind, nx, ny, byte offset)
            const rt_image &im = d->images[t.image];
            o.even = im.nx;
            o.odd = im.ny;
            o.scale = fbits((int)im.offset);
        }
    }
    return texs;
}

std::vector<rt_dinstance> to_dinstances(const rt_scene_desc *d) {
    std::vector<rt_dinstance> insts(d->ninstances);
    for (int i = 0; i < d->ninstances; i++) {
        const rt_instance &in = d->instances[i];
        rt_dinstance &o = insts[i];
        o.nops = in.nops;
        for (int k = 0; k < in.nops; k++) {
            o.ops[k][0] = fbits((int)in.ops[k][0]);   // op code as integer bits
            for (int c = 1; c < 4; c++) o.ops[k][c] = in.ops[k][c];
        }
    }
    return insts;
}

std::vector<rt_dmedium> to_dmedia(const rt_scene_desc *d) {
    std::vector<rt_dmedium> media(d->nmedia);
    for (int i = 0; i < d->nmedia; i++) {
        media[i].first = d->media[i].boundary_first;
        media[i].count = d->media[i].boundary_count;
        media[i].neg_inv_density = -(1 / d->media[i].density);   // constant_medium.h:36
        media[i].material = d->media[i].material;
    }
    return media;
}

}  // namespace

int validate_desc(const rt_scene_desc *d) {
    if (!d) return fail(RT_ERR_INVALID, "null scene descriptor");
    if (d->abi_version != RT_ABI_VERSION) return fail(RT_ERR_INVALID, "rt_scene_desc.abi_version mismatch");
    if (d->nprims < 0 || d->nboundary < 0 || d->nmedia < 0 || d->nmaterials < 0 || d->ntextures < 0 || d->ninstances < 0)
        return fail(RT_ERR_INVALID, "negative count in scene descriptor");
    if (d->nprims > (1 << 24) - 1 || d->nboundary > (1 << 24) - 1) return fail(RT_ERR_INVALID, "too many primitives");
    if (d->nmaterials > (1 << 22)) return fail(RT_ERR_INVALID, "too many materials");
    if (!d->perlin_ranvec || !d->perlin_perm) return fail(RT_ERR_INVALID, "missing Perlin tables");
    if (d->nimages < 0 || d->image_bytes < 0 || (d->nimages > 0 && (!d->images || !d->image_data)))
        return fail(RT_ERR_INVALID, "bad image arrays");
    auto check_prim = [&](const rt_prim &p) -> int {
        if (p.kind < RT_PRIM_SPHERE || p.kind > RT_PRIM_YZ_RECT) return fail(RT_ERR_INVALID, "bad primitive kind");
        if (p.material < 0 || p.material >= d->nmaterials) return fail(RT_ERR_INVALID, "primitive material out of range");
        if (p.instance < -1 || p.instance >= d->ninstances) return fail(RT_ERR_INVALID, "primitive instance out of range");
        return RT_OK;
    };
    for (int i = 0; i < d->nprims; i++) if (int rc = check_prim(d->prims[i])) return rc;
    for (int i = 0; i < d->nboundary; i++) if (int rc = check_prim(d->boundary_prims[i])) return rc;
    for (int i = 0; i < d->nmedia; i++) {
        const rt_medium &m = d->media[i];
        if (m.boundary_first < 0 || m.boundary_count < 0 || m.boundary_first + m.boundary_count > d->nboundary)
            return fail(RT_ERR_INVALID, "medium boundary range out of range");
        // the device reads a medium's first boundary record unconditionally (load_media,
        // media_hit); dropping the medium instead would renumber the others' draw ordinals
        if (m.boundary_count == 0)
            return fail(RT_ERR_UNSUPPORTED, "medium " + std::to_string(i) + " has no boundary primitive (boundary_count 0)");
        if (m.material < 0 || m.material >= d->nmaterials) return fail(RT_ERR_INVALID, "medium material out of range");
    }
    for (int i = 0; i < d->ninstances; i++) {
        const rt_instance &in = d->instances[i];
        if (in.nops < 0 || in.nops > RT_MAX_INSTANCE_OPS) return fail(RT_ERR_INVALID, "instance chain too long");
        for (int k = 0; k < in.nops; k++) {
            const int op = (int)in.ops[k][0];
            if (op < RT_OP_TRANSLATE || op > RT_OP_FLIP) return fail(RT_ERR_INVALID, "bad instance op");
        }
    }
    for (int i = 0; i < d->ntextures; i++) {
        const rt_texture &t = d->textures[i];
        if (t.kind < RT_TEX_CONSTANT || t.kind > RT_TEX_IMAGE) return fail(RT_ERR_INVALID, "bad texture kind");
        if (t.kind == RT_TEX_IMAGE) {
            if (t.image < 0 || t.image >= d->nimages) return fail(RT_ERR_INVALID, "image texture index out of range");
            const rt_image &im = d->images[t.image];
            if (im.nx <= 0 || im.ny <= 0 || im.offset < 0 ||
                im.offset + (int64_t)3 * im.nx * im.ny > d->image_bytes || im.offset > 0x7FFFFFFF)
                return fail(RT_ERR_INVALID, "image texels out of range");
        }
        if (t.kind == RT_TEX_CHECKER) {
            if (t.even < 0 || t.even >= d->ntextures || t.odd < 0 || t.odd >= d->ntextures)
                return fail(RT_ERR_INVALID, "checker child out of range");
        }
    }
    // checker chains must terminate within the device's depth guard
    for (int i = 0; i < d->ntextures; i++) {
        std::vector<int> stack{i};
        std::vector<int> depth{0};
        while (!stack.empty()) {
            int t = stack.back(), dd = depth.back();
            stack.pop_back(); depth.pop_back();
            if (dd >= RT_MAX_CHECKER_DEPTH) return fail(RT_ERR_UNSUPPORTED, "checker textures nested too deep (or cyclic)");
            if (d->textures[t].kind == RT_TEX_CHECKER) {
                stack.push_back(d->textures[t].even); depth.push_back(dd + 1);
                stack.push_back(d->textures[t].odd); depth.push_back(dd + 1);
            }
        }
    }
    for (int i = 0; i < d->nmaterials; i++) {
        const rt_material &m = d->materials[i];
        if (m.kind < RT_MAT_LAMBERTIAN || m.kind > RT_MAT_ISOTROPIC) return fail(RT_ERR_INVALID, "bad material kind");
        const bool textured = m.kind == RT_MAT_LAMBERTIAN || m.kind == RT_MAT_DIFFUSE_LIGHT || m.kind == RT_MAT_ISOTROPIC;
        if (textured && (m.texture < 0 || m.texture >= d->ntextures)) return fail(RT_ERR_INVALID, "material texture out of range");
    }
    return RT_OK;
}

int lower_scene(const rt_scene_desc *d, LoweredScene *out) {
    PhaseTrace trace{"rt_scene_create"};
    LoweredScene &s = *out;
    s = LoweredScene();
    s.time0 = d->time0;
    s.time1 = d->time1;

    std::vector<int> big, rest;
    select_prescan(d, big, rest);
    BvhResult bvh;
    try {
        bvh = build_shifted_bvh(d, big, rest);
    } catch (const std::exception &ex) {
        return fail(RT_ERR_INVALID, std::string("BVH build failed: ") + ex.what());
    }
    trace("BVH build");

    std::vector<int> order = bvh.order;
    std::vector<rt_dgroup> groups;
    s.scan = flat_scan(d, bvh.width, order, groups);
    for (const rt_dgroup &g : groups) {   // the per-kind runs cover the group exactly
        const int runs = (g.kinds & 0xff) + ((g.kinds >> 8) & 0xff) + ((g.kinds >> 16) & 0xff) +
                         ((g.kinds >> 24) & 0xff) + g.nyz;
        if (runs != g.count) return fail(RT_ERR_INVALID, "flat scan: a group's kind counts do not add up");
    }
    if (!s.scan && d->nprims > 0) medium_cell(d, s, order);

    std::vector<rt_dprim> prims(order.size()), bprims(d->nboundary);
    for (int i = 0; i < (int)order.size(); i++) {
        const int src = order[i];
        prims[i] = to_dprim(d->prims[src], src);
        s.has_moving |= d->prims[src].kind == RT_PRIM_MOVING_SPHERE;
    }
    for (int i = 0; i < d->nboundary; i++) {
        bprims[i] = to_dprim(d->boundary_prims[i], i);
        s.has_moving |= d->boundary_prims[i].kind == RT_PRIM_MOVING_SPHERE;
    }
    const std::vector<rt_dmaterial> mats = to_dmaterials(d, s);
    ball_fast_media(d, mats, s);
    const std::vector<rt_dtexture> texs = to_dtextures(d, s);
    const std::vector<rt_dinstance> insts = to_dinstances(d);
    const std::vector<rt_dmedium> media = to_dmedia(d);
    std::vector<float> ranvec(256 * 4, 0.0f);
    for (int i = 0; i < 256; i++) for (int k = 0; k < 3; k++) ranvec[4 * i + k] = d->perlin_ranvec[3 * i + k];
    const std::vector<int32_t> perm(d->perlin_perm, d->perlin_perm + 768);
    const std::vector<uint8_t> texels(d->image_data, d->image_data + (d->nimages > 0 ? d->image_bytes : 0));
    for (int v : perm) if (v < 0 || v > 255) return fail(RT_ERR_INVALID, "Perlin permutation entry out of range");

    if (bvh.width == 4) s.nodes = stage(s.image, bvh.nodes4);
    else if (bvh.width == 8) s.nodes = stage(s.image, bvh.nodes8);
    else if (bvh.width == RT_BVH_CW8) s.nodes = stage(s.image, bvh.nodes8q);
    else s.nodes = stage(s.image, bvh.nodes2);
    s.prims = stage(s.image, prims);
    s.bprims = stage(s.image, bprims);
    s.media = stage(s.image, media);
    s.mats = stage(s.image, mats);
    s.texs = stage(s.image, texs);
    s.insts = stage(s.image, insts);
    s.groups = stage(s.image, groups);
    s.ranvec = stage(s.image, ranvec);
    s.perm = stage(s.image, perm);
    s.texels = stage(s.image, texels);
    trace("device records");

    s.root = bvh.root;
    s.has_bvh = d->nprims > 0;
    s.nmedia = d->nmedia;
    s.deep_balls = dense_balls(d);
    s.surf_boxes.resize((size_t)d->nprims * 6);
    s.surf_spheres.resize((size_t)d->nprims * 5);
    for (int i = 0; i < d->nprims; i++) {
        const rt_prim &pr = d->prims[i];
        prim_bounds(pr, d->instances, d->time0, d->time1, &s.surf_boxes[(size_t)i * 6], &s.surf_boxes[(size_t)i * 6 + 3]);
        const bool plain = pr.kind == RT_PRIM_SPHERE && pr.instance < 0;
        for (int k = 0; k < 3; k++) s.surf_spheres[(size_t)i * 5 + k] = plain ? pr.p[k] : 0.0f;
        s.surf_spheres[(size_t)i * 5 + 3] = plain ? std::fabs(pr.p[3]) : -1.0f;
        s.surf_spheres[(size_t)i * 5 + 4] = pr.kind == RT_PRIM_SPHERE ? std::fabs(pr.p[3])
                                            : pr.kind == RT_PRIM_MOVING_SPHERE ? std::fabs(pr.p[8]) : 0.0f;
    }
    for (int i = 0; i < d->nmedia; i++) {
        const rt_medium &m = d->media[i];
        const rt_prim &bp = d->boundary_prims[m.boundary_first];
        s.media_plain = s.media_plain && m.boundary_count == 1 && bp.kind == RT_PRIM_SPHERE && bp.instance < 0;
    }
    s.bvh_depth = bvh.depth;
    s.nnodes = (int)bvh.node_count();
    s.bvh_width = bvh.width;
    s.nprims = d->nprims;
    s.ninstances = d->ninstances;
    s.ngroups = (int)groups.size();
    s.nprescan = s.scan ? 0 : (int)big.size();
    return RT_OK;
}

}  // namespace rtnw
