"""The reprojected frame history, the CPU side: the exact statement of the rule, the ABI's structs
and entry points, the argument checks of rt_temporal / rt_temporal_dev (made before any HIP call,
so they answer without a GPU), the rule on analytic planes seen by two cameras, and on the
oracle's cornell_box.

The rule is stated here in numpy float32, not in the product:
tests/test_gpu_temporal.py imports `temporal_ref` and compares the GPU's result with it bit for
bit.  Every operation is an add, subtract, multiply, IEEE divide, sqrt, floor, max, min, abs or
comparison on float32 values, in the order written; rt_temporal.hip performs the same sequence
without contraction.  dot(a, b) = (a0*b0 + a1*b1) + a2*b2.  For pixel p = (x, y), row 0 on top,
with n_f = frame_spp, the frame's colour c_f and moments (S1, S2), its guides (coverage cov_p,
normal n_p, depth z_p), the current camera (origin o, lower_left_corner llc, horizontal hor,
vertical ver) and the previous one (o', llc', hor', ver', w'):

    no history (first frame):      use = false
    cameras bytewise equal:        n_h = min(len_h[p], max_history);  use = n_h > 0
                                   c_h = color_h[p];  mu_h = M_h[p] / float(len_h[p])
    otherwise, when cov_p == 1:
        s = (float(x) + 0.5f) / float(nx);   t = (float(ny - 1 - y) + 0.5f) / float(ny)
        e = ((llc + s*hor) + t*ver) - o                       # per component
        k = z_p / sqrt(dot(e, e));   d = (o + e*k) - o'
        dw = dot(d, w');   only when dw < 0:                  # in front of the previous camera
        a = llc' - o';   tau = dot(a, w') / dw;   r = d*tau - a
        s' = dot(r, hor') / dot(hor', hor');   t' = dot(r, ver') / dot(ver', ver')
        fx = s'*float(nx) - 0.5f;   fy = float(ny - 1) - (t'*float(ny) - 0.5f);   z' = sqrt(dot(d, d))
        bx = floor(fx), by = floor(fy);  wx1 = fx - bx, wx0 = 1.0f - wx1;  wy1 = fy - by, wy0 = 1.0f - wy1
        W = 0, C = 0, m = 0, nmin = INT_MAX
        for j = 0, 1 (outer), i = 0, 1 (inner):  q = (bx + float(i), by + float(j)),  w = wx_i * wy_j
            counts = w > 0 and 0 <= q.x < float(nx) and 0 <= q.y < float(ny)      # NaN fails
                     and int(q.x) < nx and int(q.y) < ny and len_h[q] > 0 and cov_h[q] == 1
                     and dot(n_p, n_q) >= cos_normal
                     and |z' - z_q| <= sigma_depth * min(z', z_q) + 1e-6f
            if counts: W = W + w;  C = C + w*color_h[q];  m = m + w*(M_h[q] / float(len_h[q]))
                       nmin = min(nmin, len_h[q])
        n_h = min(nmin, max_history);  use = W > 0 and n_h > 0;  c_h = C / W;  mu_h = m / W
    use:      n = n_h + n_f;  a = float(n_f) / float(n)
              out = c_h + (c_f - c_h)*a;  M' = (mu_h + (S / float(n_f) - mu_h)*a) * float(n);  len' = n
    not use:  out = c_f, M' = S, len' = n_f                   # the frame bit for bit

A Jacobi pass: every value read is an input; taps outside the image do not exist.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import oracle as O
import rtnw
from conftest import ROOT

RT_ERR_INVALID = -1
RT_ERR_HIP = -2
F = np.float32
THREADS = min(16, os.cpu_count() or 1)


# ------------------------------------------------------------------ the rule, in numpy
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _camera(cam):
    """The fields the rule reads, float32 scalars per component."""
    d = cam.desc
    return {k: [F(v) for v in getattr(d, k)] for k in ("origin", "lower_left_corner", "horizontal", "vertical", "w")}


def temporal_ref(cur, cam, hist=None, prev_cam=None, *, frame_spp, max_history, cos_normal, sigma_depth, debug=None):
    """rt_temporal on host arrays, bit for bit: (colour, moments' or None, len).  `cur`: dict of
    color [ny, nx, 3], features (Scene.render_features' dict or packed guides [ny, nx, 8]) and
    moments [ny, nx, 2] or None; `hist`: None, or such a dict with len [ny, nx] int32 besides;
    the cameras are rtnw.Camera.  `debug`: a dict that receives per-pixel counts of the taps (with
    a positive weight, of reprojected pixels) that counted, lay outside, met len 0, and failed
    the coverage, the normal or the depth test alone."""
    cf = np.ascontiguousarray(cur["color"], F)
    ny, nx, _ = cf.shape
    g = rtnw.pack_guides(cur["features"])
    S = None if cur.get("moments") is None else np.asarray(cur["moments"], F)
    n_f = int(frame_spp)
    use = np.zeros((ny, nx), bool)
    nh = np.zeros((ny, nx), np.int64)
    ch = np.zeros((ny, nx, 3), F)
    mu = np.zeros((ny, nx, 2), F)
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
            else:
                use, nh, ch, mu = _reproject(nx, ny, g, _camera(cam), hc, hg, hm, hl, _camera(prev_cam), max_history,
                                             cos_normal, sigma_depth, debug)
    with np.errstate(all="ignore"):
        n = np.where(use, nh + n_f, n_f).astype(np.int32)
        fn, nf = n.astype(F), F(n_f)
        a = nf / fn
        out = np.where(use[..., None], ch + (cf - ch) * a[..., None], cf)
        mom = None
        if S is not None:
            mom = np.where(use[..., None], (mu + (S / nf - mu) * a[..., None]) * fn[..., None], S)
            assert mom.dtype == F
    assert out.dtype == F
    return out, mom, n


def _reproject(nx, ny, g, c, hc, hg, hm, hl, pc, max_history, cos_normal, sigma_depth, debug):
    cov, n_p, z = g[..., 3], [g[..., 4], g[..., 5], g[..., 6]], g[..., 7]
    X, Y = np.arange(nx), np.arange(ny)[:, None]
    s = (X.astype(F) + F(0.5)) / F(nx)
    t = ((ny - 1 - Y).astype(F) + F(0.5)) / F(ny)
    e = [((c["lower_left_corner"][i] + s * c["horizontal"][i]) + t * c["vertical"][i]) - c["origin"][i] for i in range(3)]
    k = z / np.sqrt(_dot(e, e))
    d = [(c["origin"][i] + e[i] * k) - pc["origin"][i] for i in range(3)]
    dw = _dot(d, pc["w"])
    a = [pc["lower_left_corner"][i] - pc["origin"][i] for i in range(3)]
    tau = _dot(a, pc["w"]) / dw
    r = [d[i] * tau - a[i] for i in range(3)]
    sp = _dot(r, pc["horizontal"]) / _dot(pc["horizontal"], pc["horizontal"])
    tq = _dot(r, pc["vertical"]) / _dot(pc["vertical"], pc["vertical"])
    fx = sp * F(nx) - F(0.5)
    fy = F(ny - 1) - (tq * F(ny) - F(0.5))
    zp = np.sqrt(_dot(d, d))
    active = (cov == F(1)) & (dw < F(0))
    bx, by = np.floor(fx), np.floor(fy)
    wx1, wy1 = fx - bx, fy - by
    wx, wy = [F(1) - wx1, wx1], [F(1) - wy1, wy1]
    W = np.zeros((ny, nx), F)
    C = np.zeros((ny, nx, 3), F)
    m = np.zeros((ny, nx, 2), F)
    nmin = np.full((ny, nx), 0x7FFFFFFF, np.int64)
    dbg = {k_: np.zeros((ny, nx), np.int32) for k_ in ("taps", "outside", "len0", "coverage", "normal", "depth")}
    for j in range(2):
        for i in range(2):
            qxf, qyf = bx + F(i), by + F(j)
            w = wx[i] * wy[j]
            assert w.dtype == qxf.dtype == zp.dtype == F
            cand = active & (w > F(0))
            inn = cand & (qxf >= F(0)) & (qxf < F(nx)) & (qyf >= F(0)) & (qyf < F(ny))
            qx, qy = np.where(inn, qxf, F(0)).astype(np.int64), np.where(inn, qyf, F(0)).astype(np.int64)
            inn = inn & (qx < nx) & (qy < ny)
            qx, qy = np.where(inn, qx, 0), np.where(inn, qy, 0)   # any in-image cell: `inn` masks it
            lq, Gq = hl[qy, qx], hg[qy, qx]
            dn = _dot(n_p, [Gq[..., 4], Gq[..., 5], Gq[..., 6]])
            t_len, t_cov, t_n = lq > 0, Gq[..., 3] == F(1), dn >= F(cos_normal)
            t_z = np.abs(zp - Gq[..., 7]) <= F(sigma_depth) * np.minimum(zp, Gq[..., 7]) + F(1e-6)
            ok = inn & t_len & t_cov & t_n & t_z
            W = np.where(ok, W + w, W)
            C = np.where(ok[..., None], C + w[..., None] * hc[qy, qx], C)
            if hm is not None:
                m = np.where(ok[..., None], m + w[..., None] * (hm[qy, qx] / lq.astype(F)[..., None]), m)
            nmin = np.where(ok, np.minimum(nmin, lq), nmin)
            dbg["taps"] += ok
            dbg["outside"] += cand & ~inn
            dbg["len0"] += inn & ~t_len
            dbg["coverage"] += inn & t_len & ~t_cov
            dbg["normal"] += inn & t_len & t_cov & ~t_n & t_z
            dbg["depth"] += inn & t_len & t_cov & t_n & ~t_z
    assert W.dtype == C.dtype == m.dtype == F
    if debug is not None:
        debug.update(dbg, fx=fx, fy=fy, active=active)
    nh = np.minimum(nmin, max_history)
    use = (W > F(0)) & (nh > 0)
    return use, nh, C / W[..., None], m / W[..., None]


SETTINGS = dict(max_history=24, cos_normal=0.9, sigma_depth=0.1, frame_spp=4)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ analytic planes under a camera
# (normal, a point of the plane, lowest x, highest x, highest y, albedo): a back wall, a panel in front of its
# left part (a depth step of a fifth at x = -0.3) and a panel hinged on the wall at x = 1.5 (the
# depth is continuous there, the normals' dot product is 0.8)
PLANES = [((0.0, 0.0, -1.0), (0.0, 0.0, 4.0), -1e9, 1e9, 2.5, (0.7, 0.7, 0.7)),
          ((0.0, 0.0, -1.0), (0.0, 0.0, 2.0), -1e9, -0.3, 2.5, (0.8, 0.3, 0.2)),
          ((-0.6, 0.0, -0.8), (1.5, 0.0, 4.0), 1.5, 1e9, 2.5, (0.2, 0.4, 0.8))]


def plane_guides(cam, nx, ny, planes=PLANES):
    """The packed guides [ny, nx, 8] a pinhole render of the planes would give, analytically (in
    double, rounded once): the nearest plane a pixel centre's ray meets; a miss is albedo 1,
    coverage 0, normal 0, depth 0, as rt_render_features writes it."""
    d = cam.desc
    o, llc, hor, ver = (np.array(list(getattr(d, k)), np.float64) for k in ("origin", "lower_left_corner", "horizontal", "vertical"))
    s = (np.arange(nx) + 0.5) / nx
    t = ((ny - 1 - np.arange(ny)) + 0.5) / ny
    e = llc + s[None, :, None] * hor + t[:, None, None] * ver - o
    best = np.full((ny, nx), np.inf)
    g = np.zeros((ny, nx, 8), np.float64)
    g[..., 0:3] = 1.0
    for n, p0, xlo, xhi, yhi, alb in planes:
        n, p0 = np.array(n), np.array(p0)
        den = e @ n
        with np.errstate(all="ignore"):
            tt = ((p0 - o) @ n) / den
        P = o + e * tt[..., None]
        hit = (den < 0) & (tt > 0) & (P[..., 0] >= xlo) & (P[..., 0] <= xhi) & (P[..., 1] <= yhi) & (tt < best)
        best = np.where(hit, tt, best)
        g[hit, 0:3], g[hit, 3], g[hit, 4:7] = alb, 1.0, n
        g[..., 7] = np.where(hit, tt * np.sqrt((e * e).sum(-1)), g[..., 7])
    return g.astype(F)


def view(nx, ny, lookfrom, lookat):
    """A pinhole camera whose wider half-angle is about 36 degrees whatever the aspect."""
    aspect = float(F(nx) / F(ny))
    vfov = 40.0 if aspect <= 2 else math.degrees(2 * math.atan(math.tan(math.radians(20.0)) * 2 / aspect))
    return rtnw.Camera(lookfrom, lookat, (0, 1, 0), vfov, aspect, 0.0, 1.0)


_cases = {}


def two_camera_case(nx, ny):
    """The synthetic two-camera case of the GPU tests, made once and left unchanged: (cur, cam,
    hist, prev_cam).  The planes above seen from two nearby cameras; a seeded random frame and
    history with moments; the history's len in 1..40 (the cap of SETTINGS is 24) with a block and
    a sprinkle of zeros; a few pixels of either frame partly covered."""
    if (nx, ny) not in _cases:
        rng = np.random.default_rng(1000 * nx + ny)
        prev_cam = view(nx, ny, (0.0, 0.5, -6.0), (0.0, 0.3, 0.0))
        cam = view(nx, ny, (0.45, 0.55, -5.9), (0.35, 0.3, 0.0))

        def frame(c):
            gd = plane_guides(c, nx, ny)
            part = rng.random((ny, nx)) < 0.03
            gd[..., 3] = np.where(part, F(0.75), gd[..., 3])
            ln = rng.integers(1, 41, (ny, nx)).astype(np.int32)
            col = (rng.random((ny, nx, 3)) * 2).astype(F)
            mean = (rng.random((ny, nx)) * 3).astype(F)
            mom = np.stack([mean * ln, (mean * mean + F(0.5)) * ln], -1).astype(F)
            return dict(color=col, features=gd, moments=mom, len=ln)
        hist, cur = frame(prev_cam), frame(cam)
        hist["len"][rng.random((ny, nx)) < 0.02] = 0
        hist["len"][ny // 2:ny // 2 + max(1, ny // 5), nx // 3:nx // 3 + max(1, nx // 8)] = 0
        cur["moments"] = (cur["moments"] / cur["len"].astype(F)[..., None] * F(SETTINGS["frame_spp"])).astype(F)
        del cur["len"]
        for fr in (hist, cur):
            for v in fr.values():
                v.setflags(write=False)
        _cases[(nx, ny)] = (cur, cam, hist, prev_cam)
    return _cases[(nx, ny)]


def without_moments(fr):
    return None if fr is None else {**fr, "moments": None}


# ------------------------------------------------------------------ properties of the rule
def flat(nx, ny, seed, cam):
    """A frame on the planes with seeded colour and moments."""
    rng = np.random.default_rng(seed)
    mean = (rng.random((ny, nx)) * 3).astype(F)
    return dict(color=(rng.random((ny, nx, 3)) * 2).astype(F), features=plane_guides(cam, nx, ny),
                moments=np.stack([mean * F(4), mean * mean * F(4) + F(1)], -1).astype(F))


def test_a_first_frame_copies_the_frame_bit_for_bit():
    cur, cam, _, _ = two_camera_case(33, 40)
    for fr in (cur, without_moments(cur)):
        out, mom, ln = temporal_ref(fr, cam, **SETTINGS)
        assert np.array_equal(bits(out), bits(cur["color"])) and (ln == SETTINGS["frame_spp"]).all()
        assert mom is None if fr["moments"] is None else np.array_equal(bits(mom), bits(cur["moments"]))


def test_equal_cameras_map_every_pixel_to_itself_and_len_stops_at_the_cap():
    nx, ny = 17, 11
    cam, same_cam = view(nx, ny, (0, 0.5, -6), (0, 0.3, 0)), view(nx, ny, (0, 0.5, -6), (0, 0.3, 0))
    fr = flat(nx, ny, 3, cam)
    kw = {**SETTINGS, "max_history": 10}
    hist, lens = None, []
    for _ in range(6):
        out, mom, ln = temporal_ref(fr, cam, hist, same_cam, **kw)
        lens.append(int(ln[0, 0]))
        assert (ln == ln[0, 0]).all()     # misses and partly covered pixels accumulate too: no tests
        # K equal frames keep the value, but for the blend's roundings
        assert np.abs(out - fr["color"]).max() <= 4 * 2.0 ** -24 * 2
        assert np.abs(mom - fr["moments"] / F(4) * ln[..., None].astype(F)).max() <= 1e-5 * np.abs(mom).max()
        hist = dict(color=out, features=fr["features"], moments=mom, len=ln)
    assert lens == [4, 8, 12, 14, 14, 14]    # n_h = min(len, 10): a running mean, then an exponential one
    # one blend, written out
    h = dict(color=fr["color"][::-1].copy(), features=fr["features"], moments=fr["moments"][::-1].copy(),
             len=np.full((ny, nx), 8, np.int32))
    out, mom, ln = temporal_ref(fr, cam, h, same_cam, **SETTINGS)
    a = F(4) / F(12)
    assert (ln == 12).all() and np.array_equal(bits(out), bits(h["color"] + (fr["color"] - h["color"]) * a))
    mu = h["moments"] / F(8)
    assert np.array_equal(bits(mom), bits((mu + (fr["moments"] / F(4) - mu) * a) * F(12)))
    # max_history 0: no history at all
    out, mom, ln = temporal_ref(fr, cam, h, same_cam, **{**SETTINGS, "max_history": 0})
    assert np.array_equal(bits(out), bits(fr["color"])) and np.array_equal(bits(mom), bits(fr["moments"])) and (ln == 4).all()


def exact_camera(x):
    """A pinhole camera at (x, 0, -8) looking down +z whose image plane (4 x 4 at z = -4) and 8 x 8
    pixels make every step of the reprojection of the plane z = 8 exact in float32: a pixel is 2
    units wide on that plane."""
    cam = rtnw.Camera((x, 0, -8), (x, 0, 0), (0, 1, 0), 90.0, 1.0, 0.0, 1.0)
    d = cam.desc
    d.origin[:] = (x, 0, -8)
    d.lower_left_corner[:] = (x - 2, -2, -4)
    d.horizontal[:] = (4, 0, 0)
    d.vertical[:] = (0, 4, 0)
    d.u[:], d.v[:], d.w[:] = (1, 0, 0), (0, 1, 0), (0, 0, -1)
    return cam


def test_a_sideways_shift_by_whole_pixels_lands_on_single_taps():
    nx = ny = 8
    wall = [((0.0, 0.0, -1.0), (0.0, 0.0, 8.0), -1e9, 1e9, 1e9, (0.5, 0.5, 0.5))]
    prev_cam, cam = exact_camera(0.0), exact_camera(4.0)      # two pixels to the right
    rng = np.random.default_rng(5)
    cur = dict(color=(rng.random((ny, nx, 3)) * 2).astype(F), features=plane_guides(cam, nx, ny, wall),
               moments=(rng.random((ny, nx, 2)) * 8).astype(F))
    hist = dict(color=(rng.random((ny, nx, 3)) * 2).astype(F), features=plane_guides(prev_cam, nx, ny, wall),
                moments=(rng.random((ny, nx, 2)) * 30).astype(F), len=rng.integers(1, 20, (ny, nx)).astype(np.int32))
    dbg = {}
    out, mom, ln = temporal_ref(cur, cam, hist, prev_cam, debug=dbg, **SETTINGS)
    assert np.array_equal(dbg["fx"], np.broadcast_to(np.arange(nx, dtype=F) + 2, (ny, nx)))
    assert np.array_equal(dbg["fy"], np.broadcast_to(np.arange(ny, dtype=F)[:, None], (ny, nx)))
    assert (dbg["taps"][:, :nx - 2] == 1).all() and (dbg["taps"][:, nx - 2:] == 0).all()
    # the last two columns look past the history's edge: the frame; the others blend with the one pixel
    assert np.array_equal(bits(out[:, nx - 2:]), bits(cur["color"][:, nx - 2:])) and (ln[:, nx - 2:] == 4).all()
    hl = hist["len"][:, 2:]
    assert np.array_equal(ln[:, :nx - 2], hl + 4)             # no neighbour's len leaks in through a zero weight
    a = (F(4) / (hl + 4).astype(F))[..., None]
    hcol = hist["color"][:, 2:]
    assert np.array_equal(bits(out[:, :nx - 2]), bits(hcol + (cur["color"][:, :nx - 2] - hcol) * a))
    mu = hist["moments"][:, 2:] / hl.astype(F)[..., None]
    want = (mu + (cur["moments"][:, :nx - 2] / F(4) - mu) * a) * (hl + 4).astype(F)[..., None]
    assert np.array_equal(bits(mom[:, :nx - 2]), bits(want))


def test_a_depth_step_leaves_the_uncovered_strip_to_the_frame():
    nx, ny = 96, 8
    prev_cam, cam = view(nx, ny, (0, 0.5, -6), (0, 0.5, 0)), view(nx, ny, (1.8, 0.5, -6), (1.8, 0.5, 0))
    planes = PLANES[:2]
    cur = flat(nx, ny, 7, cam)
    cur["features"] = plane_guides(cam, nx, ny, planes)
    hist = dict(flat(nx, ny, 8, prev_cam), len=np.full((ny, nx), 8, np.int32))
    hist["features"] = plane_guides(prev_cam, nx, ny, planes)
    dbg = {}
    out, mom, ln = temporal_ref(cur, cam, hist, prev_cam, debug=dbg, **SETTINGS)
    # moving right uncovers wall that the front panel hid: wall pixels whose taps all show the panel
    strip = (ln == 4) & (dbg["taps"] == 0) & (dbg["depth"] > 0)
    assert strip.any(axis=1).all() and 1 <= strip.sum(1).min() and strip.sum(1).max() <= 12, strip.sum(1)
    z = cur["features"][..., 7]
    assert (z[strip] > 9).all()                               # they are wall (depth 10), not panel (8)
    assert np.array_equal(bits(out[strip]), bits(cur["color"][strip]))
    assert np.array_equal(bits(mom[strip]), bits(cur["moments"][strip]))
    assert (ln[~strip & (dbg["taps"] == 4)] == 12).all() and (dbg["taps"] == 4).mean() > 0.6


def test_a_tap_with_len_zero_is_rejected():
    nx, ny = 8, 8
    wall = [((0.0, 0.0, -1.0), (0.0, 0.0, 8.0), -1e9, 1e9, 1e9, (0.5, 0.5, 0.5))]
    prev_cam, cam = exact_camera(0.0), exact_camera(1.0)      # half a pixel: two taps of weight 1/2
    rng = np.random.default_rng(9)
    cur = dict(color=(rng.random((ny, nx, 3)) * 2).astype(F), features=plane_guides(cam, nx, ny, wall), moments=None)
    hist = dict(color=(rng.random((ny, nx, 3)) * 2).astype(F), features=plane_guides(prev_cam, nx, ny, wall), moments=None,
                len=np.full((ny, nx), 8, np.int32))
    hist["len"][3, 4] = 0
    dbg = {}
    out, _, ln = temporal_ref(cur, cam, hist, prev_cam, debug=dbg, **SETTINGS)
    assert (dbg["taps"][:, :nx - 1] == 2).sum() == ny * (nx - 1) - 2
    for x, other in ((3, 3), (4, 5)):                         # the two pixels that straddle it take the other tap alone
        assert dbg["taps"][3, x] == 1 and dbg["len0"][3, x] == 1 and ln[3, x] == 12
        h = (F(0.5) * hist["color"][3, other]) / F(0.5)
        assert np.array_equal(bits(out[3, x]), bits(h + (cur["color"][3, x] - h) * (F(4) / F(12))))
    hist["len"][...] = 0
    out, _, ln = temporal_ref(cur, cam, hist, prev_cam, **SETTINGS)
    assert np.array_equal(bits(out), bits(cur["color"])) and (ln == 4).all()


def test_a_previous_camera_facing_away_gives_no_history():
    nx, ny = 33, 40
    cur, cam, hist, _ = two_camera_case(nx, ny)
    away = view(nx, ny, (0.0, 0.5, -6.0), (0.0, 0.3, -12.0))
    dbg = {}
    out, mom, ln = temporal_ref(cur, cam, hist, away, debug=dbg, **SETTINGS)
    assert not dbg["active"].any()
    assert np.array_equal(bits(out), bits(cur["color"])) and np.array_equal(bits(mom), bits(cur["moments"]))
    assert (ln == 4).all()


@pytest.mark.parametrize("nx,ny", [(130, 9), (33, 40)])
def test_the_two_camera_case_is_not_vacuous(nx, ny):
    """What tests/test_gpu_temporal.py compares on the GPU exercises every way a tap can fail."""
    cur, cam, hist, prev_cam = two_camera_case(nx, ny)
    dbg = {}
    out, mom, ln = temporal_ref(cur, cam, hist, prev_cam, debug=dbg, **SETTINGS)
    assert np.isfinite(out).all() and np.isfinite(mom).all()
    taps = dbg["taps"]
    counts = {k: int((dbg[k] > 0).sum()) for k in ("outside", "len0", "coverage", "normal", "depth")}
    print(f"{nx}x{ny}: taps per pixel {np.bincount(taps.ravel(), minlength=5).tolist()}, pixels with a tap that {counts}")
    assert (taps == 4).sum() * 4 >= nx * ny
    assert ((taps >= 1) & (taps <= 3)).any()
    assert all(v >= 1 for v in counts.values()), counts
    assert (ln == 4).any() and (ln == 4 + 24).any() and ((ln > 4) & (ln < 28)).any()   # none, capped, uncapped
    out2, none, ln2 = temporal_ref(without_moments(cur), cam, without_moments(hist), prev_cam, **SETTINGS)
    assert none is None and np.array_equal(bits(out), bits(out2)) and np.array_equal(ln, ln2)


# ------------------------------------------------------------------ the ABI
def _struct_fields(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            typ, names = decl.strip().rsplit(None, 1) if "*" in decl else decl.strip().split(None, 1)
            out += [(n.strip().lstrip("*"), typ.strip()) for n in names.split(",")]
    return out


def test_ctypes_structs_have_the_headers_layout():
    want = _struct_fields("rt_temporal_params")
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    got = [(n, t) for n, t in rtnw.RtTemporalParams._fields_]
    assert [n for n, _ in got] == [re.sub(r"\[.*\]", "", n) for n, _ in want]
    for (n, t), (wn, wt) in zip(got, want):
        size = re.search(r"\[(\d+)\]", wn)
        assert t == (ctype[wt] * int(size.group(1)) if size else ctype[wt]), n
    assert ctypes.sizeof(rtnw.RtTemporalParams) == 32
    frame = _struct_fields("rt_temporal_frame")
    assert [n for n, _ in frame] == [n for n, _ in rtnw.RtTemporalFrame._fields_] == ["color", "guides", "moments", "len"]
    assert ctypes.sizeof(rtnw.RtTemporalFrame) == 4 * ctypes.sizeof(ctypes.c_void_p)
    tp = rtnw.temporal_params(4)
    assert tp.frame_spp == 4 and tp.max_history == rtnw.TEMPORAL_DEFAULTS["max_history"] and list(tp.pad) == [0, 0, 0, 0]


def test_library_exports_the_temporal_entry_points():
    L = rtnw.lib()
    for name in ("rt_temporal", "rt_temporal_dev", "rt_launch_temporal"):
        assert hasattr(L, name), name
    assert {"rt_temporal", "rt_temporal_dev"} <= set(rtnw.header_symbols())
    assert L.rt_temporal.argtypes is not None and L.rt_temporal_dev.argtypes is not None
    assert hasattr(rtnw, "temporal") and hasattr(rtnw, "temporal_params")


# ------------------------------------------------------------------ argument checks, no GPU
def _call(tp, *, nx=4, ny=3, null=None, moments="both", out_moments=True, history=True, alias=None, dev=False):
    """rt_temporal / rt_temporal_dev on small host buffers (never read when a check fails; the
    device form's pointers are never read on the host at all)."""
    L = rtnw.lib()
    h, w = max(ny, 1), max(nx, 1)
    mk = lambda c: np.zeros((h, w, c), np.float32)
    buf = {"cur.color": mk(3), "cur.guides": mk(8), "cur.moments": mk(2), "hist.color": mk(3), "hist.guides": mk(8),
           "hist.moments": mk(2), "hist.len": np.ones((h, w), np.int32), "out.color": mk(3), "out.moments": mk(2),
           "out.len": np.zeros((h, w), np.int32)}
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
            ref("prev_cam", prev.desc) if history else None, ref("tp", tp), ref("out", out))
    rc = L.rt_temporal_dev(*args, None) if dev else L.rt_temporal(*args, None)
    return rc, L.rt_last_error().decode()


def _good(**kw):
    v = {**SETTINGS, **kw}
    pad = v.pop("pad", None)
    tp = rtnw.temporal_params(**v)
    if pad is not None:
        tp.pad[pad] = 1
    return tp


HAVE_DEVICE = rtnw.device_count() > 0
# rt_temporal_dev launches a kernel on the pointers it is given: with a device present, arguments
# that pass its checks must come with device memory (tests/test_gpu_temporal.py does that)
DEV_WITHOUT_GPU = pytest.param(True, marks=pytest.mark.skipif(HAVE_DEVICE, reason="a GPU is present"))


@pytest.mark.parametrize("dev", [False, DEV_WITHOUT_GPU])
def test_valid_arguments_reach_the_device_check(dev):
    inf = float("inf")
    for tp, kw in ((_good(), {}), (_good(max_history=0), {}), (_good(max_history=1 << 23), {}), (_good(cos_normal=-1.0), {}),
                   (_good(cos_normal=1.0), {}), (_good(sigma_depth=0.0), {}), (_good(sigma_depth=inf), {}),
                   (_good(frame_spp=1), {}), (_good(frame_spp=65535), {}), (_good(), dict(history=False)),
                   (_good(), dict(moments="none", out_moments=False)), (_good(), dict(out_moments=False)),
                   (_good(), dict(history=False, moments="cur")), (_good(), dict(alias=("out.moments", "cur.moments")))):
        rc, msg = _call(tp, dev=dev, **kw)
        assert rc != RT_ERR_INVALID, (rc, msg)
        if HAVE_DEVICE:   # rt_temporal stages its host buffers itself: a legal call
            assert rc == rtnw.RT_OK, (rc, msg)
        else:             # nothing about the arguments
            assert rc == RT_ERR_HIP and "hipSetDevice" in msg, (rc, msg)


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("null", ["cur", "cam", "prev_cam", "tp", "out", "cur.color", "cur.guides", "hist.color",
                                  "hist.guides", "hist.len", "out.color", "out.len"])
def test_null_arguments_are_invalid(null, dev):
    rc, msg = _call(_good(), null=null, dev=dev)
    assert rc == RT_ERR_INVALID and "null argument" in msg and null.replace(".", "->") in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("field,value", [
    ("max_history", -1), ("max_history", (1 << 23) + 1), ("cos_normal", -1.5), ("cos_normal", 1.01),
    ("cos_normal", float("nan")), ("sigma_depth", -1.0), ("sigma_depth", float("nan")), ("frame_spp", 0),
    ("frame_spp", -4), ("frame_spp", 65536), ("pad", 0), ("pad", 3),
])
def test_bad_parameters_are_invalid(field, value, dev):
    rc, msg = _call(_good(**{field: value}), dev=dev)
    assert rc == RT_ERR_INVALID and field in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("nx,ny", [(0, 3), (4, 0), (-1, 3), (4, -2), (65536, 32768), (1 << 30, 2)])
def test_empty_and_oversized_images_are_invalid(nx, ny, dev):
    L = rtnw.lib()
    one = np.zeros(16, np.float32).ctypes.data      # never read: the size check comes first
    tp, cam = _good(), rtnw.Camera.preset("cornell", 4, 4)
    cur = rtnw.RtTemporalFrame(one, one, None, None)
    out = rtnw.RtTemporalFrame(one + 4, None, None, one + 8)
    args = (0, nx, ny, ctypes.byref(cur), ctypes.byref(cam.desc), None, None, ctypes.byref(tp), ctypes.byref(out), None)
    rc = L.rt_temporal_dev(*args) if dev else L.rt_temporal(*args)
    msg = L.rt_last_error().decode()
    assert rc == RT_ERR_INVALID and "nx and ny" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("moments,out_moments,word", [("cur", True, "hist->moments"), ("hist", False, "cur->moments"),
                                                      ("none", True, "out->moments")])
def test_moments_given_inconsistently_are_invalid(moments, out_moments, word, dev):
    rc, msg = _call(_good(), moments=moments, out_moments=out_moments, dev=dev)
    assert rc == RT_ERR_INVALID and word in msg, msg
    if moments == "none":   # a first frame too
        rc, msg = _call(_good(), moments=moments, out_moments=True, history=False, dev=dev)
        assert rc == RT_ERR_INVALID and word in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("a,b", [("out.color", "cur.color"), ("out.color", "hist.color"), ("out.moments", "hist.moments"),
                                 ("out.len", "hist.len")])
def test_in_place_is_invalid(a, b, dev):
    rc, msg = _call(_good(), alias=(a, b), dev=dev)
    assert rc == RT_ERR_INVALID and a.replace(".", "->") in msg and b.replace(".", "->") in msg, msg


# ------------------------------------------------------------------ on the oracle's cornell_box
NX = NY = 48
SPP, SEED = 4, 31
_rendered = {}


def oracle_cornell_pair():
    """Two frames of the oracle's cornell_box 48 x 48 at 4 spp (kernel statement, samples 0..3 and
    4..7) from two cameras a step apart, with their first-hit guides; computed once."""
    if not _rendered:
        _, _, depth = rtnw.SCENE_DEFAULTS["cornell_box"]
        desc = rtnw.SceneDesc.builtin("cornell_box")
        aspect = float(F(NX) / F(NY))
        cams = [rtnw.Camera(lf, (278, 278, 0), (0, 1, 0), 40.0, aspect, 0.0, 10.0) for lf in ((228, 278, -800), (268, 288, -800))]
        frames = []
        for k, cam in enumerate(cams):
            spec = O.desc_spec(NX, NY, SPP, max_depth=depth, background="black", seed=SEED, chunk=1, threads=THREADS,
                               sample_offset=k * SPP)
            color, _ = O.render_desc(desc, cam, spec)
            f = O.feature_means(O.first_hits_desc(desc, cam, spec))
            for v in (color, *f.values()):
                v.setflags(write=False)
            frames.append(dict(color=color, features=f, moments=None))
        _rendered.update(cams=cams, frames=frames)
    return _rendered["cams"], _rendered["frames"]


def test_the_rule_on_the_oracles_cornell_box_accumulates_most_pixels():
    cams, frames = oracle_cornell_pair()
    kw = dict(frame_spp=SPP, max_history=32, cos_normal=0.9, sigma_depth=0.1)
    c0, _, l0 = temporal_ref(frames[0], cams[0], **kw)
    assert np.array_equal(bits(c0), bits(frames[0]["color"])) and (l0 == SPP).all()
    dbg = {}
    c1, none, l1 = temporal_ref(frames[1], cams[1], dict(frames[0], color=c0, len=l0), cams[0], debug=dbg, **kw)
    assert none is None and np.isfinite(c1).all()
    share = float((l1 == 2 * SPP).mean())
    print(f"cornell_box {NX}x{NY}, two cameras a step apart: {share:.3f} of the pixels take history; taps per pixel "
          f"{np.bincount(dbg['taps'].ravel(), minlength=5).tolist()}")
    assert set(np.unique(l1)) == {SPP, 2 * SPP} and share > 0.5
    keep = l1 == SPP
    assert np.array_equal(bits(c1[keep]), bits(frames[1]["color"][keep]))
