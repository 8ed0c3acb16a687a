// empty_pixels.cpp — which pixels of a render job are provably empty: no primary ray of the
// pixel can reach a surface primitive, so a sample of it is decided by the media alone
// (rt_megakernel.h refill finishes such samples at the work claim).
//
// The test, in double.  A primary ray of pixel (x, y) has the direction
// D = llc + cu hor + cv ver - org with cu in [x / nx, (x + 1) / nx], cv likewise (main.cpp:
// 305-306, camera.h:52-55 with a zero lens radius).  With M = [hor ver llc - org] and
// (a, b, g) = M^-1 (P - org), a point P = org + t D has g = t and (a / g, b / g) = (cu, cv): the
// pixel's rays fill the pyramid cu0 <= a / g <= cu1, cv0 <= b / g <= cv1, g >= 0, whose four side
// planes are a - cu0 g = 0 and so on.  The footprint is widened by one pixel on every side and by
// what an error of the direction moves (a / g, b / g).  That error is taken as 1e-4 of the
// direction's magnitude plus a bound of the float rounding in camera_finish's sum, whose terms
// are as large as the origin (final(): 600 against a direction of 10): four operations of at
// most half an ulp of twice the largest camera component each, 8 x 2^-24 of it, doubled.  (1e-4
// of the origin's magnitude instead would widen final()'s footprint by ten pixels at 500 x 500
// and leave 0.56 of the oracle's empty pixels flagged.)  A primitive is out of the pyramid when all 8 corners
// of its padded box (prim_bounds, the BVH's own premise: an accepted hit lies inside it) lie
// outside one side plane, or all have g <= 0 (behind the origin).  A plain sphere is also
// tested itself, by its centre's distance from each side plane: its box's corners reach far
// outside its silhouette.  A sphere's radius is widened first by what float cancellation in
// its discriminant (sphere.h:28-31: b^2 - a c with |oc| >> R) can add to it.
//
// The four planes of a pixel are two of its column and two of its row, so a primitive's
// pixels are the product of the columns and the rows it is not out of: each primitive marks
// that set in a byte map of the job's bounding rectangle, as intervals where all corners
// lie in front of the camera (nearly always), column by column otherwise.  What is left
// unmarked is empty.  That is the per-pixel test of every primitive, without its cost.
#include "empty_pixels.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace rtnw {

namespace {

struct CamBasis {
    double org[3];
    double inv[3][3];   // rows of M^-1: (a, b, g) = inv (P - org)
    double eu, ev;      // the footprint's widening in cu and cv beyond the one pixel
};

bool cam_basis(const rt_camera_desc *cam, CamBasis *cb) {
    double H[3], V[3], W[3], mag = 0, dmag = 0;
    for (int k = 0; k < 3; k++) {
        cb->org[k] = cam->origin[k];
        H[k] = cam->horizontal[k];
        V[k] = cam->vertical[k];
        W[k] = (double)cam->lower_left_corner[k] - cb->org[k];
        dmag = std::max(dmag, std::fabs(W[k]) + 2 * std::fabs(H[k]) + 2 * std::fabs(V[k]));   // cu, cv in [-1, 2]
        for (double v : {cb->org[k], H[k], V[k], (double)cam->lower_left_corner[k]}) {
            if (!std::isfinite(v)) return false;
            mag = std::max(mag, std::fabs(v));
        }
    }
    // M = [H V W] (columns); M^-1 = adj(M) / det, rows: V x W, W x H, H x V
    auto cross = [](const double a[3], const double b[3], double c[3]) {
        c[0] = a[1] * b[2] - a[2] * b[1];
        c[1] = a[2] * b[0] - a[0] * b[2];
        c[2] = a[0] * b[1] - a[1] * b[0];
    };
    double r0[3], r1[3], r2[3];
    cross(V, W, r0);
    cross(W, H, r1);
    cross(H, V, r2);
    const double det = H[0] * r0[0] + H[1] * r0[1] + H[2] * r0[2];
    auto norm = [](const double a[3]) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); };
    if (!(std::fabs(det) > 1e-9 * norm(H) * norm(V) * norm(W)) || !std::isfinite(det)) return false;
    for (int k = 0; k < 3; k++) {
        cb->inv[0][k] = r0[k] / det;
        cb->inv[1][k] = r1[k] / det;
        cb->inv[2][k] = r2[k] / det;
    }
    // a direction off by delta (every component) moves (a, b, g) / t by at most the rows' 1-norms
    // times delta: cu by (|row a| + 2 |row g|) delta for cu in [-1, 2], while |row g| delta << 1
    const double delta = 1e-4 * dmag + 16 * 0x1p-24 * mag;
    auto n1 = [&](int r) { return std::fabs(cb->inv[r][0]) + std::fabs(cb->inv[r][1]) + std::fabs(cb->inv[r][2]); };
    if (!(n1(2) * delta < 0.01)) return false;
    cb->eu = 1.02 * (n1(0) + 2 * n1(2)) * delta;
    cb->ev = 1.02 * (n1(1) + 2 * n1(2)) * delta;
    return std::isfinite(cb->eu) && std::isfinite(cb->ev);
}

void to_cam(const CamBasis &cb, const double p[3], double out[3]) {
    const double q[3] = {p[0] - cb.org[0], p[1] - cb.org[1], p[2] - cb.org[2]};
    for (int r = 0; r < 3; r++) out[r] = cb.inv[r][0] * q[0] + cb.inv[r][1] * q[1] + cb.inv[r][2] * q[2];
}

// One axis of the footprint: index i of n (a column x, or a row counted from the bottom) spans
// [lo(i), hi(i)] of cu (cv), widened.
struct Axis {
    int n;
    double e;
    double lo(int i) const { return (double)(i - 1) / n - e; }
    double hi(int i) const { return (double)(i + 2) / n + e; }
};

// The indices in [i0, i1] whose two planes the primitive is not out of: ok[i - i0] = 1.
// a[c], g[c]: the corners' coordinate along the axis and their depth.  With a sphere
// (sr >= 0: sa, sg its centre's, na / ng the plane-function gradients' parts: the plane
// a - u g = 0 has the gradient row_a - u row_g) the centre's distance decides as well.
struct SphereAxis {
    double a, g, r;          // centre's (a, g), padded radius; r < 0: no sphere
    double raa, rag, rgg;    // row_a . row_a, row_a . row_g, row_g . row_g
};
// Returns false when no index is covered, else *first and *last: the range written (ok is not
// touched outside it).
bool axis_cover(const Axis &ax, const double a[8], const double g[8], const SphereAxis &sp, int i0, int i1, uint8_t *ok,
                int *first, int *last) {
    bool front = true;
    for (int c = 0; c < 8; c++) front = front && g[c] > 0;
    int lo_i = i0, hi_i = i1;
    if (front) {
        // all corners in front: out below when lo(i) > max a / g, out above when hi(i) < min a / g
        double umin = a[0] / g[0], umax = umin;
        for (int c = 1; c < 8; c++) {
            const double u = a[c] / g[c];
            umin = std::min(umin, u);
            umax = std::max(umax, u);
        }
        // hi(i) >= umin  <=>  i >= (umin - e) n - 2;  lo(i) <= umax  <=>  i <= (umax + e) n + 1
        const double fl = std::floor((umin - ax.e) * ax.n - 2) - 1, fh = std::ceil((umax + ax.e) * ax.n + 1) + 1;
        if (fl > (double)i1 || fh < (double)i0) return false;
        lo_i = std::max(i0, fl < (double)i0 ? i0 : (int)fl);
        hi_i = std::min(i1, fh > (double)i1 ? i1 : (int)fh);
    }
    for (int i = lo_i; i <= hi_i; i++) {
        const double ul = ax.lo(i), uh = ax.hi(i);
        bool below = true, above = true;   // all corners outside the lower / the upper plane
        for (int c = 0; c < 8; c++) {
            below = below && (a[c] - ul * g[c] < 0);
            above = above && (a[c] - uh * g[c] > 0);
        }
        bool out = below || above;
        if (!out && sp.r >= 0) {
            // the centre's signed distance from the plane a - u g = 0 is (a - u g) / |row_a - u row_g|
            const double fl = sp.a - ul * sp.g, fh = sp.a - uh * sp.g;
            const double nl = sp.raa - 2 * ul * sp.rag + ul * ul * sp.rgg, nh = sp.raa - 2 * uh * sp.rag + uh * uh * sp.rgg;
            out = (fl < 0 && fl * fl > sp.r * sp.r * nl) || (fh > 0 && fh * fh > sp.r * sp.r * nh);
        }
        ok[i - i0] = out ? 0 : 1;
    }
    // trim to the covered indices
    while (lo_i <= hi_i && !ok[lo_i - i0]) lo_i++;
    while (hi_i >= lo_i && !ok[hi_i - i0]) hi_i--;
    *first = lo_i;
    *last = hi_i;
    return lo_i <= hi_i;
}

}  // namespace

bool empty_fast_scene_ok(const SceneInfo &s, const rt_camera_desc *cam) {
    if (const char *e = std::getenv("RTNW_EMPTY_FAST"))
        if (std::atoi(e) == 0) return false;
    if (!(cam->lens_radius == 0.0f)) return false;
    for (int k = 0; k < 3; k++)
        if (cam->origin[k] == 0.0f && std::signbit(cam->origin[k])) return false;
    // (only the width-2 media variant carries refill's code, rt_megakernel.h kEmptyFast: the scenes
    // with no instance chain, (u, v)-reading material, checker texture or pre-scanned primitive)
    if (!s.media_plain || s.ninstances > 0 || s.has_uv || s.has_checker || s.nprescan > 0 || s.bvh_width != 2) return false;
    CamBasis cb;
    return cam_basis(cam, &cb);
}

bool empty_fast_render_ok(float t_min, int chunk, int flags, bool tile_job) {
    return tile_job && chunk == 1 && t_min >= 0.0f && !(flags & RT_FLAG_RIGHT_FOLD);
}

bool empty_pixel_bits(const SceneInfo &s, const rt_camera_desc *cam, int nx, int ny, const uint32_t *xy, size_t n,
                      std::vector<uint32_t> *bits, size_t *nflagged) {
    bits->assign((n + 31) / 32, 0u);
    *nflagged = 0;
    CamBasis cb;
    if (n == 0 || nx < 1 || ny < 1 || !cam_basis(cam, &cb)) return false;
    // the job's bounding rectangle (image coordinates), and its byte map: 1 = some primitive may be hit
    int x0 = 0xFFFF, x1 = 0, y0 = 0xFFFF, y1 = 0;
    for (size_t k = 0; k < n; k++) {
        const int x = (int)(xy[k] & 0xFFFFu), y = (int)(xy[k] >> 16);
        x0 = std::min(x0, x); x1 = std::max(x1, x);
        y0 = std::min(y0, y); y1 = std::max(y1, y);
    }
    if (x1 >= nx || y1 >= ny) return false;
    const size_t w = (size_t)(x1 - x0 + 1), h = (size_t)(y1 - y0 + 1);
    if (w * h > 4 * n + (1u << 20)) return false;   // pixels far apart in a huge frame: no map
    std::vector<uint8_t> hit(w * h, 0), colok(w), rowok(h);
    const Axis axu{nx, cb.eu}, axv{ny, cb.ev};
    // rows count from the bottom: image row y is j = ny - 1 - y
    const int j0 = ny - 1 - y1, j1 = ny - 1 - y0;
    auto dot3 = [](const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    const size_t nprims = s.surf_boxes.size() / 6;
    for (size_t p = 0; p < nprims; p++) {
        const float *B = &s.surf_boxes[p * 6];
        const float *S = &s.surf_spheres[p * 5];
        // a sphere's radius grows by what cancellation in its discriminant can add: the float
        // error of b^2 - a c is a few ulp of a |oc|^2, which shifts R^2 by that much
        double fuzz = 0;
        if (S[4] > 0) {
            double far2 = 0;
            for (int k = 0; k < 3; k++) {
                const double d = std::max(std::fabs(B[k] - cb.org[k]), std::fabs(B[3 + k] - cb.org[k]));
                far2 += d * d;
            }
            fuzz = 16 * 6e-8 * far2 / std::max((double)S[4], 1e-30);
        }
        if (!std::isfinite(fuzz)) fuzz = 1e300;
        double a[8], b[8], g[8];
        bool behind = true, finite = true;
        for (int c = 0; c < 8; c++) {
            const double P[3] = {(c & 1) ? (double)B[3] + fuzz : (double)B[0] - fuzz, (c & 2) ? (double)B[4] + fuzz : (double)B[1] - fuzz,
                                 (c & 4) ? (double)B[5] + fuzz : (double)B[2] - fuzz};
            double q[3];
            to_cam(cb, P, q);
            a[c] = q[0]; b[c] = q[1]; g[c] = q[2];
            behind = behind && g[c] <= 0;
            finite = finite && std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2]);
        }
        if (!finite) {   // a box the map cannot place: every pixel may hit it
            std::fill(hit.begin(), hit.end(), (uint8_t)1);
            break;
        }
        if (behind) continue;
        SphereAxis su{0, 0, -1, 0, 0, 0}, sv = su;
        if (S[3] >= 0) {
            const double C[3] = {S[0], S[1], S[2]};
            double q[3];
            to_cam(cb, C, q);
            const double cmax = std::max(std::fabs(C[0]), std::max(std::fabs(C[1]), std::fabs(C[2])));
            const double r = (double)S[3] * (1 + 1e-4) + 1e-3 + 1e-4 * cmax + fuzz;
            su = SphereAxis{q[0], q[2], r, dot3(cb.inv[0], cb.inv[0]), dot3(cb.inv[0], cb.inv[2]), dot3(cb.inv[2], cb.inv[2])};
            sv = SphereAxis{q[1], q[2], r, dot3(cb.inv[1], cb.inv[1]), dot3(cb.inv[1], cb.inv[2]), dot3(cb.inv[2], cb.inv[2])};
            if (!std::isfinite(r) || !std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2])) su.r = sv.r = -1;
        }
        int ca, cz, ra, rz;
        if (!axis_cover(axu, a, g, su, x0, x1, colok.data(), &ca, &cz)) continue;
        if (!axis_cover(axv, b, g, sv, j0, j1, rowok.data(), &ra, &rz)) continue;
        // the columns it covers (one run with all corners in front), marked in every row it covers
        const size_t c0 = (size_t)(ca - x0), c1 = (size_t)(cz - x0) + 1;
        size_t ones = 0;
        for (size_t xx = c0; xx < c1; xx++) ones += colok[xx];
        const bool run = ones == c1 - c0 && c1 - c0 >= 32;
        for (int j = ra; j <= rz; j++) {
            if (!rowok[(size_t)(j - j0)]) continue;
            uint8_t *row = &hit[(size_t)(j1 - j) * w];   // row j from the bottom is image row y0 + (j1 - j)
            if (run) std::memset(row + c0, 1, c1 - c0);
            else for (size_t xx = c0; xx < c1; xx++) row[xx] |= colok[xx];
        }
    }
    size_t cnt = 0;
    for (size_t k = 0; k < n; k++) {
        const size_t x = (xy[k] & 0xFFFFu) - (size_t)x0, y = (xy[k] >> 16) - (size_t)y0;
        if (!hit[y * w + x]) {
            (*bits)[k >> 5] |= 1u << (k & 31);
            cnt++;
        }
    }
    *nflagged = cnt;
    return true;
}

}  // namespace rtnw

extern "C" long rt_scene_desc_empty_pixels(const rt_scene_desc *d, const rt_camera_desc *cam, int nx, int ny, int x0, int y0,
                                           int w, int h, float t_min, int chunk, int flags, uint8_t *flags_out, int *on) {
    if (!cam || !flags_out || w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || nx > 65535 || ny > 65535 || w > nx - x0 || h > ny - y0)
        return rt_internal_fail(RT_ERR_INVALID, "rt_scene_desc_empty_pixels: bad argument");
    if (int rc = rtnw::validate_desc(d)) return rc;
    rtnw::LoweredScene low;
    if (int rc = rtnw::lower_scene(d, &low)) return rc;
    std::memset(flags_out, 0, (size_t)w * h);
    if (on) *on = rtnw::empty_fast_scene_ok(low, cam) && rtnw::empty_fast_render_ok(t_min, chunk > 0 ? chunk : 1, flags, true);
    std::vector<uint32_t> xy((size_t)w * h), bits;
    for (int yy = 0; yy < h; yy++)
        for (int xx = 0; xx < w; xx++) xy[(size_t)yy * w + xx] = (uint32_t)(x0 + xx) | ((uint32_t)(y0 + yy) << 16);
    size_t nflagged = 0;
    if (!rtnw::empty_pixel_bits(low, cam, nx, ny, xy.data(), xy.size(), &bits, &nflagged)) return 0;
    for (size_t k = 0; k < xy.size(); k++) flags_out[k] = (bits[k >> 5] >> (k & 31)) & 1u;
    return (long)nflagged;
}
