"""The frame history for background and edge pixels, the CPU side: the exact statement of the rule,
the ABI's struct and entry points, and the argument checks of rt_temporal_cover /
rt_temporal_cover_dev (made before any HIP call, so they answer without a GPU).

The rule is rt_temporal_clamped's (tests/test_temporal_clamp_spec.py, whose `_clamp` this file
calls) with two more classes of pixels under unequal cameras, stated here in numpy float32
(DESIGN.md §7k): tests/test_gpu_temporal_cover.py imports `temporal_cover_ref` and compares the
GPU's result with it bit for bit.  The operations are those of tests/test_temporal_spec.py, in
the order written; rt_temporal.hip's cover kernel performs the same sequence without contraction.
With the settings background, edges (0 / 1) and sigma_coverage besides rt_temporal_clamped's, for
a pixel p with coverage c, guide normal N and guide depth Z (means over samples in which a miss
contributes 0):

    no history (first frame):   rt_temporal's rule;  clipped = 0, source = 0
    cameras bytewise equal:     rt_temporal's rule;  clipped = 0, source = use ? 8 : 0
    otherwise:
        surf = c == 1 or (edges and c >= 0.5)
        back = not surf and background and (c == 0 or (edges and c < 0.5))
        neither: use = false
        e as in rt_temporal
        surf:  n = N / c (per component);  z = Z / c;  k = z / sqrt(dot(e, e));  d = (o + e*k) - o'
        back:  d = e                                              # a point at infinity
        dw, tau, r, s', t', fx, fy, z' = sqrt(dot(d, d)), the four taps and their weights: rt_temporal's
        a tap q with coverage c_q, guide normal N_q, guide depth Z_q counts when
            w > 0 and q is inside the image and len_h[q] > 0          # as in rt_temporal
            and |c - c_q| <= sigma_coverage
            and, surf:  (c_q == 1 or (edges and c_q >= 0.5)) and dot(n, N_q / c_q) >= cos_normal
                        and |z' - z_q| <= sigma_depth * min(z', z_q) + 1e-6f  with  z_q = Z_q / c_q
                 back:  c_q == 0 or (edges and c_q < 0.5)
        W, C, m, nmin, n_h, use, c_h, mu_h: rt_temporal's
        source = use ? ((surf ? 1 : 2) | ((c != 0 and c != 1) ? 4 : 0)) : 0
        radius >= 1: rt_temporal_clamped's step on every pixel with `use`, whatever its class
    the blend is rt_temporal's

A Jacobi pass: every value read is an input; taps outside the image do not exist.
"""
import ctypes
import math
import re

import numpy as np
import pytest

import oracle as O
import rtnw
from test_temporal_clamp_spec import GAMMA, _clamp, temporal_clamped_ref
from test_temporal_spec import (DEV_WITHOUT_GPU, HAVE_DEVICE, RT_ERR_HIP, RT_ERR_INVALID, SETTINGS, THREADS, _camera, _dot,
                                _good, _struct_fields, bits, plane_guides, temporal_ref, two_camera_case, view,
                                without_moments)

F = np.float32
SRC_NONE, SRC_SURFACE, SRC_BACKGROUND, SRC_EDGE, SRC_SAME = 0, 1, 2, 4, 8


# ------------------------------------------------------------------ the rule, in numpy
def temporal_cover_ref(cur, cam, hist=None, prev_cam=None, *, background, edges, sigma_coverage, radius, gamma, frame_spp,
                       max_history, cos_normal, sigma_depth, debug=None):
    """rt_temporal_cover on host arrays, bit for bit: (colour, moments' or None, len, clipped,
    source).  The arguments are temporal_clamped_ref's and the three settings.  `debug`: a dict
    that receives `use`, `surf`, `back` and per pixel the number of taps that counted (`taps`) and
    that failed the coverage distance alone (`far`)."""
    cf = np.ascontiguousarray(cur["color"], F)
    ny, nx, _ = cf.shape
    g = rtnw.pack_guides(cur["features"])
    S = None if cur.get("moments") is None else np.asarray(cur["moments"], F)
    n_f, r = int(frame_spp), int(radius)
    use = np.zeros((ny, nx), bool)
    nh = np.zeros((ny, nx), np.int64)
    ch = np.zeros((ny, nx, 3), F)
    mu = np.zeros((ny, nx, 2), F)
    clipped = np.zeros((ny, nx), np.int32)
    source = np.zeros((ny, nx), np.int32)
    dbg = {}
    if hist is not None:
        hc, hg = np.asarray(hist["color"], F), rtnw.pack_guides(hist["features"])
        hl = np.asarray(hist["len"], np.int32)
        hm = None if S is None else np.asarray(hist["moments"], F)
        with np.errstate(all="ignore"):
            if bytes(cam.desc) == bytes(prev_cam.desc):
                nh = np.minimum(hl, max_history).astype(np.int64)
                use = nh > 0
                ch = hc
                if S is not None:
                    mu = hm / hl.astype(F)[..., None]
                source = np.where(use, SRC_SAME, SRC_NONE).astype(np.int32)
            else:
                use, nh, ch, mu, source = _reproject_cover(nx, ny, g, _camera(cam), hc, hg, hm, hl, _camera(prev_cam),
                                                           max_history, cos_normal, sigma_depth, bool(background), bool(edges),
                                                           F(sigma_coverage), dbg)
                if r >= 1:
                    ch, mu, clipped = _clamp(cf, use, ch, mu, S is not None, r, F(gamma), {})
    with np.errstate(all="ignore"):
        n = np.where(use, nh + n_f, n_f).astype(np.int32)
        fn, nf = n.astype(F), F(n_f)
        a = nf / fn
        out = np.where(use[..., None], ch + (cf - ch) * a[..., None], cf)
        mom = None
        if S is not None:
            mom = np.where(use[..., None], (mu + (S / nf - mu) * a[..., None]) * fn[..., None], S)
            assert mom.dtype == F
    assert out.dtype == F and clipped.dtype == np.int32 and source.dtype == np.int32
    if debug is not None:
        debug.update(dbg, use=use)
    return out, mom, n, clipped, source


def _reproject_cover(nx, ny, g, c, hc, hg, hm, hl, pc, max_history, cos_normal, sigma_depth, background, edges, sigma_cov, dbg):
    cov, z = g[..., 3], g[..., 7] / g[..., 3]
    n_p = [g[..., 4] / cov, g[..., 5] / cov, g[..., 6] / cov]
    surf = (cov == F(1)) | (edges & (cov >= F(0.5)))
    back = ~surf & background & ((cov == F(0)) | (edges & (cov < F(0.5))))
    X, Y = np.arange(nx), np.arange(ny)[:, None]
    s = (X.astype(F) + F(0.5)) / F(nx)
    t = ((ny - 1 - Y).astype(F) + F(0.5)) / F(ny)
    e = [((c["lower_left_corner"][i] + s * c["horizontal"][i]) + t * c["vertical"][i]) - c["origin"][i] for i in range(3)]
    k = z / np.sqrt(_dot(e, e))
    d = [np.where(surf, (c["origin"][i] + e[i] * k) - pc["origin"][i], e[i] + np.zeros((ny, nx), F)) for i in range(3)]
    dw = _dot(d, pc["w"])
    a = [pc["lower_left_corner"][i] - pc["origin"][i] for i in range(3)]
    tau = _dot(a, pc["w"]) / dw
    r = [d[i] * tau - a[i] for i in range(3)]
    sp = _dot(r, pc["horizontal"]) / _dot(pc["horizontal"], pc["horizontal"])
    tq = _dot(r, pc["vertical"]) / _dot(pc["vertical"], pc["vertical"])
    fx = sp * F(nx) - F(0.5)
    fy = F(ny - 1) - (tq * F(ny) - F(0.5))
    zp = np.sqrt(_dot(d, d))
    active = (surf | back) & (dw < F(0))
    bx, by = np.floor(fx), np.floor(fy)
    wx1, wy1 = fx - bx, fy - by
    wx, wy = [F(1) - wx1, wx1], [F(1) - wy1, wy1]
    W = np.zeros((ny, nx), F)
    C = np.zeros((ny, nx, 3), F)
    m = np.zeros((ny, nx, 2), F)
    nmin = np.full((ny, nx), 0x7FFFFFFF, np.int64)
    taps, far = np.zeros((ny, nx), np.int32), np.zeros((ny, nx), np.int32)
    for j in range(2):
        for i in range(2):
            qxf, qyf = bx + F(i), by + F(j)
            w = wx[i] * wy[j]
            assert w.dtype == qxf.dtype == zp.dtype == dw.dtype == F
            inn = active & (w > F(0)) & (qxf >= F(0)) & (qxf < F(nx)) & (qyf >= F(0)) & (qyf < F(ny))
            qx, qy = np.where(inn, qxf, F(0)).astype(np.int64), np.where(inn, qyf, F(0)).astype(np.int64)
            inn = inn & (qx < nx) & (qy < ny)
            qx, qy = np.where(inn, qx, 0), np.where(inn, qy, 0)   # any in-image cell: `inn` masks it
            lq, Gq = hl[qy, qx], hg[qy, qx]
            cq = Gq[..., 3]
            dn = _dot(n_p, [Gq[..., 4] / cq, Gq[..., 5] / cq, Gq[..., 6] / cq])
            zq = Gq[..., 7] / cq
            assert dn.dtype == zq.dtype == F
            t_cov = np.abs(cov - cq) <= sigma_cov
            ok_s = ((cq == F(1)) | (edges & (cq >= F(0.5)))) & (dn >= F(cos_normal)) & \
                   (np.abs(zp - zq) <= F(sigma_depth) * np.minimum(zp, zq) + F(1e-6))
            ok_b = (cq == F(0)) | (edges & (cq < F(0.5)))
            cls = np.where(surf, ok_s, ok_b)
            ok = inn & (lq > 0) & t_cov & cls
            W = np.where(ok, W + w, W)
            C = np.where(ok[..., None], C + w[..., None] * hc[qy, qx], C)
            if hm is not None:
                m = np.where(ok[..., None], m + w[..., None] * (hm[qy, qx] / lq.astype(F)[..., None]), m)
            nmin = np.where(ok, np.minimum(nmin, lq), nmin)
            taps += ok
            far += inn & (lq > 0) & cls & ~t_cov
    assert W.dtype == C.dtype == m.dtype == F
    nh = np.minimum(nmin, max_history)
    use = (W > F(0)) & (nh > 0)
    edge = (cov != F(0)) & (cov != F(1))
    source = np.where(use, np.where(surf, SRC_SURFACE, SRC_BACKGROUND) | np.where(edge, SRC_EDGE, 0), SRC_NONE).astype(np.int32)
    dbg.update(surf=surf, back=back, taps=taps, far=far, fx=fx, fy=fy)
    return use, nh, C / W[..., None], m / W[..., None], source


# ------------------------------------------------------------------ the case both test files share
COVER = dict(background=1, edges=1, sigma_coverage=0.25)
PLAIN = dict(background=0, edges=0, sigma_coverage=0.25)
_cover_cases = {}


def cover_case(nx, ny):
    """(cur, cam, hist, prev_cam), made once and left unchanged: two_camera_case's cameras, colours,
    moments and lens; the guides plane_guides' of each camera; then the top ceil(ny / 3) rows of
    both frames made misses (albedo 1, coverage 0, normal 0, depth 0); then 20 % of the covered
    pixels of either frame given a coverage drawn from {0.25, 0.5, 0.75}, their normal and depth
    multiplied by it (the guides' mean over samples of which that share hit)."""
    if (nx, ny) not in _cover_cases:
        cur0, cam, hist0, prev_cam = two_camera_case(nx, ny)
        rng = np.random.default_rng(1000 * nx + ny)
        top = math.ceil(ny / 3)

        def guides(c):
            gd = plane_guides(c, nx, ny)
            gd[:top] = np.array([1, 1, 1, 0, 0, 0, 0, 0], F)
            part = (gd[..., 3] == F(1)) & (rng.random((ny, nx)) < 0.2)
            share = rng.choice(np.array([0.25, 0.5, 0.75], F), (ny, nx))
            scale = np.where(part, share, F(1)).astype(F)
            gd[..., 3:8] = np.where((gd[..., 3] == F(1))[..., None], gd[..., 3:8] * scale[..., None], gd[..., 3:8])
            gd.setflags(write=False)
            return gd
        hist, cur = dict(hist0, features=guides(prev_cam)), dict(cur0, features=guides(cam))
        _cover_cases[(nx, ny)] = (cur, cam, hist, prev_cam)
    return _cover_cases[(nx, ny)]


# the sizes of tests/test_gpu_temporal_clamp.py (restated: importing that file would mark this one `gpu`)
SIZES = [(1, 1), (1, 9), (9, 1), (3, 2), (64, 4), (65, 5), (67, 9), (130, 9), (33, 40)]


@pytest.mark.parametrize("nx,ny", [s for s in SIZES if s[0] * s[1] >= 256])
def test_the_cover_case_meets_every_source_value(nx, ny):
    """What tests/test_gpu_temporal_cover.py compares on the GPU, at background 1, edges 1,
    sigma_coverage 0.25, reports each of the source values 0, 1, 2, 5 and 6 on at least 3 pixels."""
    cur, cam, hist, prev_cam = cover_case(nx, ny)
    dbg = {}
    out, mom, ln, clipped, source = temporal_cover_ref(cur, cam, hist, prev_cam, radius=0, gamma=GAMMA, debug=dbg, **COVER,
                                                       **SETTINGS)
    assert np.isfinite(out).all() and np.isfinite(mom).all()
    counts = {v: int((source == v).sum()) for v in (0, 1, 2, 5, 6)}
    print(f"{nx}x{ny}: pixels per source value {counts}; pixels with a tap too far in coverage {int((dbg['far'] > 0).sum())}")
    assert sum(counts.values()) == nx * ny
    assert all(v >= 3 for v in counts.values()), counts
    assert (dbg["far"] > 0).any()
    assert np.array_equal(source != 0, ln != SETTINGS["frame_spp"]) and not clipped.any()


# ------------------------------------------------------------------ the contracts
def same(a, b):
    return (a is None and b is None) or np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("sigma", [0.0, 0.25, 1e30])
@pytest.mark.parametrize("radius", [0, 2])
@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no-moments"])
@pytest.mark.parametrize("case", ["planes", "cover"])
@pytest.mark.parametrize("nx,ny", [(130, 9), (33, 40)])
def test_zeroed_settings_are_the_clamped_rule_bit_for_bit(nx, ny, case, moments, radius, sigma):
    cur, cam, hist, prev_cam = (two_camera_case if case == "planes" else cover_case)(nx, ny)
    if not moments:
        cur, hist = without_moments(cur), without_moments(hist)
    kw = dict(SETTINGS, radius=radius, gamma=GAMMA)
    want = temporal_clamped_ref(cur, cam, hist, prev_cam, **kw)
    got = temporal_cover_ref(cur, cam, hist, prev_cam, background=0, edges=0, sigma_coverage=sigma, **kw)
    assert same(got[0], want[0]) and same(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[3], want[3]) and (radius == 0 or got[3].any())
    took = got[2] != SETTINGS["frame_spp"]
    assert took.any() and not took.all()
    assert np.array_equal(got[4], np.where(took, SRC_SURFACE, SRC_NONE))


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no-moments"])
def test_a_first_frame_and_equal_cameras_are_the_unclamped_rule(moments):
    nx, ny = 33, 40
    cur, cam, hist, _ = cover_case(nx, ny)
    if not moments:
        cur, hist = without_moments(cur), without_moments(hist)
    same_cam = view(nx, ny, (0.45, 0.55, -5.9), (0.35, 0.3, 0.0))
    assert same_cam is not cam and bytes(same_cam.desc) == bytes(cam.desc)
    kw = dict(SETTINGS, radius=3, gamma=0.0, **COVER)
    want = temporal_ref(cur, cam, **SETTINGS)
    got = temporal_cover_ref(cur, cam, **kw)
    assert same(got[0], want[0]) and same(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert not got[3].any() and not got[4].any()
    want = temporal_ref(cur, cam, hist, same_cam, **SETTINGS)
    got = temporal_cover_ref(cur, cam, hist, same_cam, **kw)
    assert same(got[0], want[0]) and same(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert not got[3].any()
    took = np.minimum(hist["len"], SETTINGS["max_history"]) > 0
    assert took.any() and not took.all() and np.array_equal(got[4], np.where(took, SRC_SAME, SRC_NONE))
    assert np.array_equal(took, got[2] != SETTINGS["frame_spp"])


@pytest.mark.parametrize("background,edges", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("case", ["planes", "cover"])
@pytest.mark.parametrize("nx,ny", [(130, 9), (33, 40)])
def test_the_settings_only_add_pixels_with_history(nx, ny, case, background, edges):
    """A pixel with a history under rt_temporal keeps one: coverage 1 against coverage 1 passes
    every new test.  Where no new tap joined, the pixel is rt_temporal's bit for bit."""
    cur, cam, hist, prev_cam = (two_camera_case if case == "planes" else cover_case)(nx, ny)
    _, _, base_len = temporal_ref(cur, cam, hist, prev_cam, **SETTINGS)
    base = base_len != SETTINGS["frame_spp"]
    for sigma in (0.0, 0.25, 1.0):
        out, mom, ln, _, source = temporal_cover_ref(cur, cam, hist, prev_cam, background=background, edges=edges,
                                                     sigma_coverage=sigma, radius=0, gamma=GAMMA, **SETTINGS)
        took = ln != SETTINGS["frame_spp"]
        assert (took | ~base).all() and np.array_equal(took, source != 0)
        assert (source[base] == SRC_SURFACE).all()
        if case == "cover" and sigma >= 0.25:   # a partly covered pixel beside fully covered ones
            assert took.sum() > base.sum()
        if not background:
            assert not (source & SRC_BACKGROUND).any()
        if not edges:
            assert not (source & SRC_EDGE).any()


# ------------------------------------------------------------------ properties of the rule
def _misses(nx, ny):
    g = np.zeros((ny, nx, 8), F)
    g[..., 0:3] = 1
    return g


def test_a_rotating_camera_reprojects_the_background_by_direction():
    """Two cameras of equal origin that differ by a rotation, on all-miss frames with a constant
    history colour: every pixel whose direction lands inside the previous view blends with that
    constant, the others are the frame; without `background` nothing takes a history."""
    nx, ny = 40, 24
    prev_cam, cam = view(nx, ny, (0.0, 0.5, -6.0), (0.0, 0.3, 0.0)), view(nx, ny, (0.0, 0.5, -6.0), (2.0, 0.3, 0.0))
    assert list(cam.desc.origin) == list(prev_cam.desc.origin) and bytes(cam.desc) != bytes(prev_cam.desc)
    rng = np.random.default_rng(3)
    const = np.array([0.25, 0.5, 1.5], F)
    cur = dict(color=(rng.random((ny, nx, 3)) * 2).astype(F), features=_misses(nx, ny), moments=None)
    hist = dict(color=np.broadcast_to(const, (ny, nx, 3)).copy(), features=_misses(nx, ny), moments=None,
                len=np.full((ny, nx), 12, np.int32))
    dbg = {}
    out, _, ln, clipped, source = temporal_cover_ref(cur, cam, hist, prev_cam, background=1, edges=0, sigma_coverage=0.0,
                                                     radius=0, gamma=GAMMA, debug=dbg, **SETTINGS)
    # inside the previous view: the sample point lies at least a pixel from the history's border
    inside = (dbg["fx"] >= 0) & (dbg["fx"] <= nx - 1) & (dbg["fy"] >= 0) & (dbg["fy"] <= ny - 1)
    outside = (dbg["fx"] < -1) | (dbg["fx"] > nx) | (dbg["fy"] < -1) | (dbg["fy"] > ny)
    assert inside.sum() * 4 >= nx * ny and outside.sum() * 8 >= nx * ny
    assert (source[inside] == SRC_BACKGROUND).all() and (ln[inside] == 16).all()
    assert (source[outside] == SRC_NONE).all() and np.array_equal(bits(out[outside]), bits(cur["color"][outside]))
    took = source != 0
    # the taps' weights sum to W and every tap holds the constant: C / W is the constant but for roundings
    hcol = (out[took] - cur["color"][took] * (F(4) / F(16))) / (F(1) - F(4) / F(16))
    assert np.abs(hcol - const).max() <= 1e-5
    out, _, ln, _, source = temporal_cover_ref(cur, cam, hist, prev_cam, background=0, edges=1, sigma_coverage=1.0, radius=0,
                                               gamma=GAMMA, **SETTINGS)
    assert not source.any() and np.array_equal(bits(out), bits(cur["color"])) and (ln == 4).all()


def _wall_pair(nx=8, ny=8):
    """The exact cameras of test_temporal_spec half a pixel apart before a wall: two taps of weight 1/2."""
    from test_temporal_spec import exact_camera
    wall = [((0.0, 0.0, -1.0), (0.0, 0.0, 8.0), -1e9, 1e9, 1e9, (0.5, 0.5, 0.5))]
    prev_cam, cam = exact_camera(0.0), exact_camera(1.0)
    rng = np.random.default_rng(9)
    cur = dict(color=(rng.random((ny, nx, 3)) * 2).astype(F), features=plane_guides(cam, nx, ny, wall), moments=None)
    hist = dict(color=(rng.random((ny, nx, 3)) * 2).astype(F), features=plane_guides(prev_cam, nx, ny, wall), moments=None,
                len=np.full((ny, nx), 8, np.int32))
    return cur, cam, hist, prev_cam


def _with_coverage(fr, y, x, c):
    g = fr["features"].copy()
    g[y, x, 3:8] = g[y, x, 3:8] * F(c)
    return dict(fr, features=g)


def test_coverage_of_exactly_a_half_is_a_surface_pixel():
    cur, cam, hist, prev_cam = _wall_pair()
    cur = _with_coverage(cur, 3, 2, 0.5)
    kw = dict(radius=0, gamma=GAMMA, **SETTINGS)
    want, _, want_len = temporal_ref(_wall_pair()[0], cam, hist, prev_cam, **SETTINGS)
    out, _, ln, _, source = temporal_cover_ref(cur, cam, hist, prev_cam, background=1, edges=1, sigma_coverage=0.5, **kw)
    assert source[3, 2] == (SRC_SURFACE | SRC_EDGE) and ln[3, 2] == 12
    # normal * 0.5 / 0.5 and depth * 0.5 / 0.5 are exact: the pixel is the fully covered one's bit for bit
    assert np.array_equal(bits(out), bits(want)) and np.array_equal(ln, want_len)
    # just under a half it is background, and its taps, all surface, are not of its class
    cur = _with_coverage(_wall_pair()[0], 3, 2, np.nextafter(F(0.5), F(0)))
    out, _, ln, _, source = temporal_cover_ref(cur, cam, hist, prev_cam, background=1, edges=1, sigma_coverage=1.0, **kw)
    assert source[3, 2] == SRC_NONE and ln[3, 2] == 4 and np.array_equal(bits(out[3, 2]), bits(cur["color"][3, 2]))
    # without `edges` a half-covered pixel has no class
    cur = _with_coverage(_wall_pair()[0], 3, 2, 0.5)
    out, _, ln, _, source = temporal_cover_ref(cur, cam, hist, prev_cam, background=1, edges=0, sigma_coverage=1.0, **kw)
    assert source[3, 2] == SRC_NONE and ln[3, 2] == 4


def test_a_tap_just_too_far_in_coverage_is_rejected():
    cur, cam, hist, prev_cam = _wall_pair()
    hist = _with_coverage(hist, 3, 4, 0.75)     # pixels (3, 3) and (3, 4) of the frame straddle it
    kw = dict(background=1, edges=1, radius=0, gamma=GAMMA, **SETTINGS)
    dbg = {}
    out, _, ln, _, source = temporal_cover_ref(cur, cam, hist, prev_cam, sigma_coverage=0.25, debug=dbg, **kw)
    assert (dbg["taps"][:, :7] == 2).all() and not dbg["far"].any()       # |1 - 0.75| <= 0.25: it counts
    below = float(np.nextafter(F(0.25), F(0)))
    out, _, ln, _, source = temporal_cover_ref(cur, cam, hist, prev_cam, sigma_coverage=below, debug=dbg, **kw)
    for x, other in ((3, 3), (4, 5)):           # the other tap alone
        assert dbg["taps"][3, x] == 1 and dbg["far"][3, x] == 1 and ln[3, x] == 12 and source[3, x] == SRC_SURFACE
        h = (F(0.5) * hist["color"][3, other]) / F(0.5)
        assert np.array_equal(bits(out[3, x]), bits(h + (cur["color"][3, x] - h) * (F(4) / F(12))))
    assert (dbg["taps"] == 2).sum() == 8 * 7 - 2


@pytest.mark.parametrize("nx,ny", [(130, 9), (33, 40)])
def test_edges_without_background_leave_the_lesser_part_alone(nx, ny):
    cur, cam, hist, prev_cam = cover_case(nx, ny)
    out, mom, ln, _, source = temporal_cover_ref(cur, cam, hist, prev_cam, background=0, edges=1, sigma_coverage=1.0, radius=0,
                                                 gamma=GAMMA, **SETTINGS)
    cov = cur["features"][..., 3]
    low = cov < F(0.5)
    assert (cov == F(0.25)).any() and (source[low] == SRC_NONE).all() and (ln[low] == 4).all()
    assert np.array_equal(bits(out[low]), bits(cur["color"][low])) and np.array_equal(bits(mom[low]), bits(cur["moments"][low]))
    assert (source[(cov >= F(0.5)) & (cov < F(1))] == (SRC_SURFACE | SRC_EDGE)).any()
    assert set(np.unique(source)) == {SRC_NONE, SRC_SURFACE, SRC_SURFACE | SRC_EDGE}


@pytest.mark.parametrize("nx,ny", [(130, 9), (33, 40)])
def test_the_clamp_runs_on_every_class(nx, ny):
    cur, cam, hist, prev_cam = cover_case(nx, ny)
    kw = dict(COVER, **SETTINGS)
    free = temporal_cover_ref(cur, cam, hist, prev_cam, radius=0, gamma=GAMMA, **kw)
    out, mom, ln, clipped, source = temporal_cover_ref(cur, cam, hist, prev_cam, radius=2, gamma=GAMMA, **kw)
    assert np.array_equal(source, free[4]) and np.array_equal(ln, free[2])
    for v in (SRC_SURFACE, SRC_BACKGROUND, SRC_SURFACE | SRC_EDGE):
        assert (clipped[source == v] != 0).any() and (clipped[source == v] == 0).any(), v
    assert not clipped[source == 0].any()
    keep = clipped == 0
    assert np.array_equal(bits(out[keep]), bits(free[0][keep])) and np.array_equal(bits(mom[keep]), bits(free[1][keep]))


# ------------------------------------------------------------------ the ABI
def test_the_cover_struct_and_entry_points_match_the_header():
    want = _struct_fields("rt_temporal_cover_params")
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    got = list(rtnw.RtTemporalCoverParams._fields_)
    assert [n for n, _ in got] == [re.sub(r"\[.*\]", "", n) for n, _ in want] == ["background", "edges", "sigma_coverage", "pad"]
    for (n, t), (wn, wt) in zip(got, want):
        size = re.search(r"\[(\d+)\]", wn)
        assert t == (ctype[wt] * int(size.group(1)) if size else ctype[wt]), n
    assert ctypes.sizeof(rtnw.RtTemporalCoverParams) == 32
    L = rtnw.lib()
    for name in ("rt_temporal_cover", "rt_temporal_cover_dev", "rt_launch_temporal_cover"):
        assert hasattr(L, name), name
    assert {"rt_temporal_cover", "rt_temporal_cover_dev"} <= set(rtnw.header_symbols())
    assert L.rt_temporal_cover.argtypes is not None and L.rt_temporal_cover_dev.argtypes is not None
    vp = rtnw.temporal_cover_params(1, 1, 0.5)
    assert vp.background == 1 and vp.edges == 1 and vp.sigma_coverage == 0.5 and list(vp.pad) == [0] * 5
    d, D = rtnw.temporal_cover_params(), rtnw.TEMPORAL_COVER_DEFAULTS
    assert d.background == D["background"] and d.edges == D["edges"] and d.sigma_coverage == F(D["sigma_coverage"])
    assert hasattr(rtnw, "temporal_cover")
    header = open(rtnw.HEADER).read()
    for name, value in (("NONE", 0), ("SURFACE", 1), ("BACKGROUND", 2), ("EDGE", 4), ("SAME", 8)):
        assert re.search(r"RT_TEMPORAL_SRC_%s = %d\b" % (name, value), header), name
        assert getattr(rtnw, "RT_TEMPORAL_SRC_" + name) == value
    # the two older structs are as they were
    assert ctypes.sizeof(rtnw.RtTemporalParams) == 32 and ctypes.sizeof(rtnw.RtTemporalClampParams) == 32


# ------------------------------------------------------------------ argument checks, no GPU
def _call(tp, cp, vp, *, nx=4, ny=3, null=None, moments="both", out_moments=True, history=True, alias=None, dev=False,
          clipped=True, source=True):
    """rt_temporal_cover / rt_temporal_cover_dev on small host buffers (never read when a check
    fails; the device form's pointers are never read on the host at all)."""
    L = rtnw.lib()
    h, w = min(max(ny, 1), 8), min(max(nx, 1), 8)   # an oversized image fails the size check: nothing is read
    mk = lambda c: np.zeros((h, w, c), np.float32)
    buf = {"cur.color": mk(3), "cur.guides": mk(8), "cur.moments": mk(2), "hist.color": mk(3), "hist.guides": mk(8),
           "hist.moments": mk(2), "hist.len": np.ones((h, w), np.int32), "out.color": mk(3), "out.moments": mk(2),
           "out.len": np.zeros((h, w), np.int32), "clipped": np.zeros((h, w), np.int32), "source": np.zeros((h, w), np.int32)}
    ptr = {k: (None if k == null else v.ctypes.data) for k, v in buf.items()}
    if moments in ("none", "hist"):
        ptr["cur.moments"] = None
    if moments in ("none", "cur"):
        ptr["hist.moments"] = None
    if not out_moments:
        ptr["out.moments"] = None
    if alias:
        ptr[alias[0]] = ptr[alias[1]]
    cur = rtnw.RtTemporalFrame(ptr["cur.color"], ptr["cur.guides"], ptr["cur.moments"], None)
    hist = rtnw.RtTemporalFrame(ptr["hist.color"], ptr["hist.guides"], ptr["hist.moments"], ptr["hist.len"])
    out = rtnw.RtTemporalFrame(ptr["out.color"], None, ptr["out.moments"], ptr["out.len"])
    cam = rtnw.Camera.preset("cornell", w, h)
    prev = rtnw.Camera.preset("final_alt", w, h)
    ref = lambda name, v: None if null == name else ctypes.byref(v)
    args = (0, nx, ny, ref("cur", cur), ref("cam", cam.desc), ref("hist", hist) if history else None,
            ref("prev_cam", prev.desc) if history else None, ref("tp", tp), ref("cp", cp), ref("vp", vp), ref("out", out),
            ptr["clipped"] if clipped else None, ptr["source"] if source else None)
    rc = L.rt_temporal_cover_dev(*args, None) if dev else L.rt_temporal_cover(*args, None)
    return rc, L.rt_last_error().decode()


def _clamp_params(radius=2, gamma=GAMMA, pad=None):
    cp = rtnw.RtTemporalClampParams(radius, gamma)
    if pad is not None:
        cp.pad[pad] = 1
    return cp


def _cover_params(background=1, edges=1, sigma_coverage=0.25, pad=None):
    vp = rtnw.RtTemporalCoverParams(background, edges, sigma_coverage)
    if pad is not None:
        vp.pad[pad] = 1
    return vp


@pytest.mark.parametrize("dev", [False, DEV_WITHOUT_GPU])
def test_valid_arguments_reach_the_device_check(dev):
    for vp, cp, kw in ((_cover_params(), _clamp_params(), {}), (_cover_params(0, 0, 0.0), _clamp_params(radius=0), {}),
                       (_cover_params(1, 0), _clamp_params(radius=3), {}), (_cover_params(0, 1, 1e30), _clamp_params(), {}),
                       (_cover_params(), _clamp_params(), dict(clipped=False)),
                       (_cover_params(), _clamp_params(), dict(source=False)),
                       (_cover_params(), _clamp_params(), dict(clipped=False, source=False)),
                       (_cover_params(), _clamp_params(), dict(history=False)),
                       (_cover_params(), _clamp_params(), dict(moments="none", out_moments=False)),
                       (_cover_params(), _clamp_params(), dict(alias=("out.moments", "cur.moments")))):
        rc, msg = _call(_good(), cp, vp, dev=dev, **kw)
        assert rc != RT_ERR_INVALID, (rc, msg)
        if HAVE_DEVICE:   # the host form stages its host buffers itself: a legal call
            assert rc == rtnw.RT_OK, (rc, msg)
        else:             # nothing about the arguments
            assert rc == RT_ERR_HIP and "hipSetDevice" in msg, (rc, msg)


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("null", ["cur", "cam", "prev_cam", "tp", "cp", "vp", "out", "cur.color", "cur.guides", "hist.color",
                                  "hist.guides", "hist.len", "out.color", "out.len"])
def test_null_arguments_are_invalid(null, dev):
    rc, msg = _call(_good(), _clamp_params(), _cover_params(), null=null, dev=dev)
    assert rc == RT_ERR_INVALID and "null argument" in msg and "(" + null.replace(".", "->") in msg, msg
    assert ("rt_temporal_cover_dev:" if dev else "rt_temporal_cover:") in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("field,value", [("background", -1), ("background", 2), ("edges", 2), ("edges", 1 << 30),
                                         ("sigma_coverage", -0.5), ("sigma_coverage", float("nan")),
                                         ("sigma_coverage", float("inf")), ("sigma_coverage", float("-inf")),
                                         ("pad", 0), ("pad", 4)])
def test_bad_cover_parameters_are_invalid(field, value, dev):
    rc, msg = _call(_good(), _clamp_params(), _cover_params(**{field: value}), dev=dev)
    assert rc == RT_ERR_INVALID and field in msg, msg
    if field == "pad":
        assert "cover's" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("field,value", [("radius", -1), ("radius", 4), ("radius", 1 << 30), ("gamma", -0.5),
                                         ("gamma", float("nan")), ("gamma", float("inf")), ("gamma", float("-inf")),
                                         ("pad", 0), ("pad", 5)])
def test_bad_clamp_parameters_are_invalid(field, value, dev):
    rc, msg = _call(_good(), _clamp_params(**{field: value}), _cover_params(), dev=dev)
    assert rc == RT_ERR_INVALID and field in msg, msg
    if field == "pad":
        assert "clamp's" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("field,value", [
    ("max_history", -1), ("max_history", (1 << 23) + 1), ("cos_normal", -1.5), ("cos_normal", 1.01),
    ("cos_normal", float("nan")), ("sigma_depth", -1.0), ("sigma_depth", float("nan")), ("frame_spp", 0),
    ("frame_spp", 65536), ("pad", 0), ("pad", 3),
])
def test_the_unclamped_rules_bad_parameters_are_invalid(field, value, dev):
    rc, msg = _call(_good(**{field: value}), _clamp_params(), _cover_params(), dev=dev)
    assert rc == RT_ERR_INVALID and field in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("nx,ny", [(0, 3), (4, 0), (-1, 3), (65536, 32768), (1 << 30, 2)])
def test_empty_and_oversized_images_are_invalid(nx, ny, dev):
    rc, msg = _call(_good(), _clamp_params(), _cover_params(), nx=nx, ny=ny, dev=dev)
    assert rc == RT_ERR_INVALID and "nx and ny" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("moments,out_moments,word", [("cur", True, "hist->moments"), ("hist", False, "cur->moments"),
                                                      ("none", True, "out->moments")])
def test_moments_given_inconsistently_are_invalid(moments, out_moments, word, dev):
    rc, msg = _call(_good(), _clamp_params(), _cover_params(), moments=moments, out_moments=out_moments, dev=dev)
    assert rc == RT_ERR_INVALID and word in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("a,b", [("out.color", "cur.color"), ("out.color", "hist.color"), ("out.moments", "hist.moments"),
                                 ("out.len", "hist.len")])
def test_in_place_is_invalid(a, b, dev):
    rc, msg = _call(_good(), _clamp_params(), _cover_params(), alias=(a, b), dev=dev)
    assert rc == RT_ERR_INVALID and a.replace(".", "->") in msg and b.replace(".", "->") in msg, msg


FRAME_ARRAYS = ["cur.color", "cur.guides", "cur.moments", "hist.color", "hist.guides", "hist.moments", "hist.len", "out.color",
                "out.moments", "out.len"]


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("other", FRAME_ARRAYS)
def test_a_mask_that_is_one_of_the_frames_arrays_is_invalid(other, dev):
    rc, msg = _call(_good(), _clamp_params(), _cover_params(), alias=("clipped", other), dev=dev)
    assert rc == RT_ERR_INVALID and "clipped" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("other", FRAME_ARRAYS + ["clipped"])
def test_a_source_that_is_the_mask_or_one_of_the_frames_arrays_is_invalid(other, dev):
    rc, msg = _call(_good(), _clamp_params(), _cover_params(), alias=("source", other), dev=dev)
    assert rc == RT_ERR_INVALID and "source" in msg, msg
    # a first frame too
    if not other.startswith("hist."):
        rc, msg = _call(_good(), _clamp_params(), _cover_params(), alias=("source", other), history=False, dev=dev)
        assert rc == RT_ERR_INVALID and "source" in msg, msg


# ------------------------------------------------------------------ on the oracle's random_scene
NX = NY = 48
SPP, SEED = 4, 31
_rendered = {}


def oracle_random_pair():
    """Two frames of the oracle's random_scene 48 x 48 at 4 spp (kernel statement, samples 0..3 and
    4..7) under the sky, from two cameras a step apart, with their first-hit guides
    (test_temporal_spec.oracle_cornell_pair's recipe); computed once."""
    if not _rendered:
        depth = O.SCENE_DEFAULTS["random_scene"]["max_depth"]
        desc = rtnw.SceneDesc.builtin("random_scene")
        aspect = float(F(NX) / F(NY))
        cams = [rtnw.Camera(lf, (0, 0, 0), (0, 1, 0), 20.0, aspect, 0.1, 10.0) for lf in ((13, 2, 3), (13.0, 2.1, 3.25))]
        frames = []
        for k, cam in enumerate(cams):
            spec = O.desc_spec(NX, NY, SPP, max_depth=depth, background="sky", seed=SEED, chunk=1, threads=THREADS,
                               sample_offset=k * SPP)
            color, _ = O.render_desc(desc, cam, spec)
            f = O.feature_means(O.first_hits_desc(desc, cam, spec))
            for v in (color, *f.values()):
                v.setflags(write=False)
            frames.append(dict(color=color, features=f, moments=None))
        _rendered.update(cams=cams, frames=frames)
    return _rendered["cams"], _rendered["frames"]


def test_on_the_oracles_random_scene_the_sky_and_the_outlines_take_a_history():
    cams, frames = oracle_random_pair()
    kw = dict(frame_spp=SPP, max_history=32, cos_normal=0.9, sigma_depth=0.1)
    c0, _, l0 = temporal_ref(frames[0], cams[0], **kw)
    hist = dict(frames[0], color=c0, len=l0)
    _, _, base_len = temporal_ref(frames[1], cams[1], hist, cams[0], **kw)
    out, none, ln, clipped, source = temporal_cover_ref(frames[1], cams[1], hist, cams[0], radius=0, gamma=GAMMA, **COVER, **kw)
    assert none is None and np.isfinite(out).all() and not clipped.any()
    base, took = base_len != SPP, ln != SPP
    cov = rtnw.pack_guides(frames[1]["features"])[..., 3]
    counts = {int(v): int((source == v).sum()) for v in np.unique(source)}
    print(f"random_scene {NX}x{NY}, two cameras a step apart: {base.mean():.3f} of the pixels take history under rt_temporal, "
          f"{took.mean():.3f} under cover; pixels per source value {counts}; coverage 0 on {(cov == 0).mean():.3f}, "
          f"partial on {((cov > 0) & (cov < 1)).mean():.3f}")
    assert (took | ~base).all() and took.sum() > base.sum()            # a strict superset
    assert (cov == 0).any() and np.isin(source[cov == 0], (SRC_BACKGROUND, SRC_NONE)).all()
    assert (source[cov == 0] == SRC_BACKGROUND).any()
    assert np.array_equal(took, source != 0)
    keep = ~took
    assert np.array_equal(bits(out[keep]), bits(frames[1]["color"][keep]))
