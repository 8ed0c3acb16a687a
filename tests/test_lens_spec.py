"""Lens renders (rt_lens_rays, rt_render_lens) without a GPU: the interface in the
header and in rtnw.py, the argument checks (all made before any HIP call, in the header's order),
the batch planner (job_plan.cpp plan_lens, through tests/native/lens_plan_check.cpp) and the numpy
float32 statements the GPU tests (tests/test_gpu_lens.py) hold the library to:

  lens_records   the rt_path_ray (and rt_ray) records of every (pixel, sample) of a rectangle for
                 the four camera models, from oracle.counter_draws and the host libm's sinf, with
                 the operation order the device follows;
  lens_reduce    the renders' summation rule: float32 sums in sample order from 0, one add per
                 sample, times float(1.0 / spp); the moments of y = (r + g) + b; the guides from
                 the samples' rt_hit records.

The statement itself is held here to test_radiance_spec.camera_records (and through it to the
oracle) for the perspective model, and to the geometry of the other three.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import rtnw
from test_radiance_spec import camera_records
from test_trace_spec import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(os.path.abspath(rtnw.__file__))
RT_ERR_INVALID = -1
RAYS_ENTRIES = ("rt_lens_rays", "rt_lens_rays_dev")
RENDER_ENTRIES = ("rt_render_lens", "rt_render_lens_dev")
ENTRIES = RAYS_ENTRIES + RENDER_ENTRIES
MODELS = {"perspective": rtnw.RT_LENS_PERSPECTIVE, "orthographic": rtnw.RT_LENS_ORTHOGRAPHIC,
          "fisheye": rtnw.RT_LENS_FISHEYE, "equirect": rtnw.RT_LENS_EQUIRECT}

F = np.float32
PI, TWO_PI, HALF_PI = F(np.pi), F(2.0 * np.pi), F(np.pi / 2.0)     # float(pi), float(2 pi), float(pi / 2)
FOV_UNIT = F(np.pi / 360.0)

_libm = ctypes.CDLL("libm.so.6")
_libm.sinf.restype = ctypes.c_float
_libm.sinf.argtypes = [ctypes.c_float]


def sinf(x):
    """The host libm's sinf of a float32 (the device restates glibc 2.35's bit for bit)."""
    assert isinstance(x, np.float32)
    return F(_libm.sinf(float(x)))


# ------------------------------------------------------------------ the statement of the models
def _vec(v):
    return np.array(list(v), F)


def lens_sample(cam, lens, nx, ny, x, j, sample, seed):
    """(origin [3], dir [3], time, skip) float32 of sample `sample` of the pixel (x, j), j counted
    from the bottom row as main.cpp:300 counts it; the stream is that of pixel key j * nx + x."""
    d = cam.desc
    org, hor, ver, llc, cu, cv, cw = (_vec(v) for v in (d.origin, d.horizontal, d.vertical, d.lower_left_corner, d.u, d.v, d.w))
    t0, span = F(d.time0), F(d.time1) - F(d.time0)
    ndraw = 35
    while True:
        draws = O.counter_draws(seed, j * nx + x, sample, ndraw)
        s = F(x + draws[0]) / F(nx)              # main.cpp:305-306
        t = F(j + draws[1]) / F(ny)
        at = 2
        if lens.model == rtnw.RT_LENS_PERSPECTIVE:
            while at + 2 < ndraw:                # camera.h:6-12: do ... while (dot(p, p) >= 1.0)
                px, py = F(2.0) * F(draws[at]) - F(1), F(2.0) * F(draws[at + 1]) - F(1)
                at += 2
                if (px * px + py * py) + F(0) * F(0) < F(1):
                    break
            else:
                ndraw *= 2
                continue
        break
    time = F(np.float64(t0) + (draws[at] if span != 0 else 0.0) * np.float64(span))   # camera.h:54
    skip = at + 1
    if lens.model == rtnw.RT_LENS_PERSPECTIVE:
        rdx, rdy = F(d.lens_radius) * px, F(d.lens_radius) * py
        offset = cu * rdx + cv * rdy
        return org + offset, (((llc + s * hor) + t * ver) - org) - offset, time, skip
    if lens.model == rtnw.RT_LENS_ORTHOGRAPHIC:
        return (org + (s - F(0.5)) * hor) + (t - F(0.5)) * ver, -cw, time, skip
    if lens.model == rtnw.RT_LENS_FISHEYE:
        fx, fy = F(2.0) * s - F(1), F(2.0) * t - F(1)
        r = np.sqrt(fx * fx + fy * fy)
        theta = r * (F(lens.fov_deg) * FOV_UNIT)
        st, ct = sinf(theta), sinf(HALF_PI - theta)
        if r > F(1):
            return org, np.zeros(3, F), time, skip
        if r == F(0):
            return org, -cw, time, skip
        return org, (((st * fx) / r) * cu + ((st * fy) / r) * cv) - ct * cw, time, skip
    assert lens.model == rtnw.RT_LENS_EQUIRECT
    sp, se = sinf(TWO_PI * (s - F(0.5))), sinf(PI * (t - F(0.5)))
    ce, cp = sinf(PI * (F(1) - t)), sinf(TWO_PI * (F(0.75) - s))
    return org, ((ce * sp) * cu + se * cv) - (ce * cp) * cw, time, skip


def lens_records(cam, lens, nx, ny, spp, seed, rect=None, sample_offset=0, t_min=0.001):
    """(records [spp, h, w] PATH_RAY_DTYPE, trace records [spp, h, w] RAY_DTYPE) of the rectangle
    rect = (x0, y0, w, h) (None: the frame), samples [sample_offset, sample_offset + spp):
    sample-major, row 0 the top row, what rt_lens_rays must write byte for byte."""
    x0, y0, w, h = rect or (0, 0, nx, ny)
    rec = np.zeros((spp, h, w), rtnw.PATH_RAY_DTYPE)
    tr = np.zeros((spp, h, w), rtnw.RAY_DTYPE)
    for k in range(spp):
        for row in range(h):
            j = ny - 1 - (y0 + row)
            for col in range(w):
                x = x0 + col
                o, d, time, skip = lens_sample(cam, lens, nx, ny, x, j, sample_offset + k, seed)
                assert o.dtype == F and d.dtype == F and time.dtype == F
                r = rec[k, row, col]
                r["origin"], r["dir"], r["time"], r["skip"] = o, d, time, skip
                r["pixel"], r["sample"] = j * nx + x, sample_offset + k
                q = tr[k, row, col]
                q["origin"], q["dir"], q["time"], q["t_min"], q["t_max"] = o, d, time, F(t_min), F(np.inf)
    return rec, tr


def lens_reduce(rgb, hits=None):
    """The renders' summation rule on rgb [n, h, w, 3] float32 (the samples' rt_radiance rgb in
    sample order): (image [h, w, 3], moments [h, w, 2], guides [h, w, 8] or None).  hits: a dict
    of [n, h, w(, 3)] arrays as Scene.trace_rays returns them, reshaped."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == F and rgb.ndim == 4
    n, h, w, _ = rgb.shape
    k = F(1.0 / float(F(n)))                      # vec3.h:134-141, as rt_resolve
    acc, mom = np.zeros((h, w, 3), F), np.zeros((h, w, 2), F)
    for s in range(n):                            # col += temp, main.cpp:311: one add per sample
        acc = acc + rgb[s]
        y = (rgb[s, ..., 0] + rgb[s, ..., 1]) + rgb[s, ..., 2]
        mom[..., 0] = mom[..., 0] + y
        mom[..., 1] = mom[..., 1] + y * y
    guides = None
    if hits is not None:
        guides = np.zeros((h, w, 8), F)
        for s in range(n):
            guides[..., 0:3] = guides[..., 0:3] + hits["albedo"][s]
            guides[..., 3] = guides[..., 3] + (hits["prim"][s] >= 0).astype(F)
            guides[..., 4:7] = guides[..., 4:7] + hits["normal"][s]
            guides[..., 7] = guides[..., 7] + hits["depth"][s]
        guides = guides * k
    img = acc * k
    assert img.dtype == F and mom.dtype == F
    return img, mom, guides


def view(aperture=0.2, t0=0.25, t1=0.75, nx=16, ny=12):
    """A tilted camera with a lens and an open shutter."""
    aspect = float(F(nx) / F(ny))
    return rtnw.Camera((3.5, 1.2, -6.0), (0.3, 0.7, 0.2), (0.1, 1, 0), 55.0, aspect, aperture, 6.5, t0, t1)


# ------------------------------------------------------------------ the interface
def test_header_declares_the_entry_points_and_records():
    text = open(rtnw.HEADER).read()
    syms = rtnw.header_symbols()
    for name in ENTRIES:
        assert name in syms, name
    for word in ("typedef struct rt_lens_params", "RTNW_LENS_BATCH", "DESIGN.md §7i", "Perspective identity", "Composition",
                 "Independence", "NO RAY"):
        assert word in text, word
    for name, value in MODELS.items():
        assert re.search(r"RT_LENS_%s\s*=\s*%d\b" % (name.upper(), value), text), name


def test_rtnw_mirrors_the_struct():
    assert ctypes.sizeof(rtnw.RtLensParams) == 32
    assert [(n, getattr(rtnw.RtLensParams, n).offset) for n, _ in rtnw.RtLensParams._fields_] == [("model", 0), ("fov_deg", 4),
                                                                                                 ("pad", 8)]
    lp = rtnw.lens_params(rtnw.RT_LENS_FISHEYE)
    assert (lp.model, lp.fov_deg, list(lp.pad)) == (2, 180.0, [0] * 6)
    assert rtnw.lens_params(rtnw.RT_LENS_EQUIRECT, 90).fov_deg == 90.0
    for m in ("render_lens", "render_lens_dev"):
        assert callable(getattr(rtnw.Scene, m))
    assert callable(rtnw.lens_rays) and callable(rtnw.lens_rays_dev)


def test_library_exports_the_entry_points():
    L = rtnw.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name


# ------------------------------------------------------------------ argument checks, no GPU
def _call(name, *, cam=True, lens=True, params=True, out=True, model=rtnw.RT_LENS_EQUIRECT, fov=180.0, pad=None,
          rect=(3, 2, 9, 7), **pkw):
    L = rtnw.lib()
    c = view()
    lp = rtnw.lens_params(model, fov)
    if pad is not None:
        lp.pad[pad] = 1
    kw = dict(max_depth=5, t_min=0.001, background=rtnw.RT_BG_SKY, seed=3, sample_offset=3)
    kw.update(pkw)
    nx, ny, spp = kw.pop("nx", 16), kw.pop("ny", 12), kw.pop("spp", 5)
    p = rtnw.RenderParams(nx, ny, spp, **kw)
    buf = np.full(9 * 7 * 5 * 48, 0xAB, np.uint8)     # room for the tile's records; must stay untouched
    head = [ctypes.byref(c.desc) if cam else None, ctypes.byref(lp) if lens else None, ctypes.byref(p) if params else None,
            *rect, buf.ctypes.data if out else None]
    if name in RAYS_ENTRIES:
        args = [0] + head + [None] + ([None] if name.endswith("_dev") else [])
    else:
        args = [None] + head + [None, None, None]      # a null scene
    rc = getattr(L, name)(*args)
    assert (buf == 0xAB).all()
    return rc, L.rt_last_error().decode()


def _invalid(name, word, **kw):
    rc, msg = _call(name, **kw)
    assert rc == RT_ERR_INVALID and name + ":" in msg and word in msg, (rc, msg, kw)


@pytest.mark.parametrize("name", ENTRIES)
def test_bad_arguments_are_invalid_in_the_headers_order(name):
    # each call is wrong in everything that follows too (a flag, a bad depth ...; the renders have
    # a null scene): the argument named is the first in the header's order
    later = dict(flags=rtnw.RT_FLAG_COUNT, max_depth=-1)
    _invalid(name, "null camera", cam=False, lens=False, params=False, out=False)
    _invalid(name, "null lens", lens=False, params=False, out=False)
    _invalid(name, "null parameters", params=False, out=False)
    _invalid(name, "null output", out=False, model=7, **later)
    for model in (-1, 4, 7):
        _invalid(name, "model", model=model, pad=0, **later)
    for k in range(6):
        _invalid(name, "pad", pad=k, model=rtnw.RT_LENS_FISHEYE, fov=0.0, **later)
    for fov in (np.nan, 0.0, -1.0, 360.5, np.inf):
        _invalid(name, "fov_deg", model=rtnw.RT_LENS_FISHEYE, fov=fov, nx=0, **later)
    for bad in (dict(nx=0), dict(ny=0), dict(nx=65536), dict(ny=65536)):
        _invalid(name, "nx and ny", spp=0, **bad, **later)
    _invalid(name, "spp", spp=0, rect=(0, 0, 17, 1), **later)
    _invalid(name, "sample_offset", sample_offset=2 ** 32 - 5, rect=(0, 0, 17, 1), **later)
    for rect in ((0, 0, 17, 1), (0, 0, 1, 13), (-1, 0, 2, 2), (0, -1, 2, 2), (8, 0, 9, 1), (0, 6, 1, 7), (0, 0, 0, 1), (0, 0, 1, 0)):
        _invalid(name, "rectangle", rect=rect, **later)
    for flag in (rtnw.RT_FLAG_COUNT, rtnw.RT_FLAG_PROFILE, rtnw.RT_FLAG_SUM_IN, rtnw.RT_FLAG_SUM_OUT, rtnw.RT_FLAG_RIGHT_FOLD,
                 32, -1):
        _invalid(name, "flag", flags=flag, max_depth=-1)
    _invalid(name, "max_depth", max_depth=-1, t_min=np.nan)
    for t in (np.nan, np.inf, -np.inf):
        _invalid(name, "t_min", t_min=t, background=2)
    for bg in (-1, 2):
        _invalid(name, "background", background=bg)


@pytest.mark.parametrize("name", RENDER_ENTRIES)
def test_a_null_scene_is_invalid_and_comes_last(name):
    _invalid(name, "null scene")
    # the fisheye's angle is not read under another model; its legal edge, a zero depth and a chunk pass
    _invalid(name, "null scene", fov=np.nan)
    _invalid(name, "null scene", model=rtnw.RT_LENS_FISHEYE, fov=360.0, max_depth=0, chunk=7)
    _invalid(name, "null scene", model=rtnw.RT_LENS_PERSPECTIVE, rect=(0, 0, 16, 12))


# ------------------------------------------------------------------ the statement itself
def test_perspective_reduces_to_the_radiance_specs_camera_records():
    nx, ny, spp, seed = 8, 5, 3, 11
    cam = view(nx=nx, ny=ny)
    rec, tr = lens_records(cam, rtnw.lens_params(rtnw.RT_LENS_PERSPECTIVE), nx, ny, spp, seed)
    want = camera_records(cam, nx, ny, spp, seed).reshape(ny, nx, spp).transpose(2, 0, 1)   # (row, col, sample) -> sample-major
    assert np.array_equal(np.ascontiguousarray(rec).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    assert rec["skip"].min() == 5 and rec["skip"].max() > 5 and (rec["skip"] % 2 == 1).all()
    for name in ("origin", "dir", "time"):
        assert np.array_equal(bits(tr[name]), bits(rec[name])), name
    assert (tr["t_min"] == F(0.001)).all() and np.isposinf(tr["t_max"]).all() and not tr["pad"].any()


def test_a_sample_offset_and_a_tile_select_the_frames_records():
    nx, ny, seed = 8, 5, 11
    cam = view(nx=nx, ny=ny)
    for name, model in MODELS.items():
        lens = rtnw.lens_params(model, 200.0)
        full, _ = lens_records(cam, lens, nx, ny, 4, seed)
        part, _ = lens_records(cam, lens, nx, ny, 2, seed, rect=(2, 1, 5, 3), sample_offset=1)
        assert np.array_equal(part, full[1:3, 1:4, 2:7]), name
        assert (part["sample"] == np.array([1, 2], np.uint32)[:, None, None]).all()
        assert part["pixel"][0, 0, 0] == (ny - 1 - 1) * nx + 2


def _frame(model, fov=180.0, nx=16, ny=12, spp=5, seed=7, **camkw):
    cam = view(nx=nx, ny=ny, **camkw)
    rec, _ = lens_records(cam, rtnw.lens_params(model, fov), nx, ny, spp, seed)
    return cam, rec


def _centre_draws(monkeypatch, d0, d1, d2=0.5):
    monkeypatch.setattr(O, "counter_draws", lambda seed, pixel, sample, n: np.array([d0, d1, d2] + [0.5] * (n - 3)))


@pytest.mark.parametrize("fov", [90.0, 180.0, 220.0, 360.0])
def test_fisheye_directions_are_unit_and_zero_exactly_outside_the_circle(fov):
    cam, rec = _frame(rtnw.RT_LENS_FISHEYE, fov)
    d = rec["dir"].astype(np.float64)
    norm = np.sqrt((d * d).sum(-1))
    s = (rec["pixel"] % 16 + 0.5) / 16                   # pixel centres: which pixels lie wholly inside or outside
    t = (rec["pixel"] // 16 + 0.5) / 12
    r_mid = np.hypot(2 * s - 1, 2 * t - 1)
    reach = np.hypot(1 / 16, 1 / 12)                     # a sample is within half a pixel of its centre, each way
    zero = norm == 0
    assert zero.any() and (~zero).any()
    assert zero[r_mid > 1 + reach].all() and not zero[r_mid < 1 - reach].any()
    assert np.abs(norm[~zero] - 1).max() < 1e-6
    assert (rec["skip"] == 3).all() and (bits(rec["origin"]) == bits(_vec(cam.desc.origin))).all()


def test_equirect_directions_are_unit_and_cover_the_sphere():
    cam, rec = _frame(rtnw.RT_LENS_EQUIRECT)
    d = rec["dir"].astype(np.float64)
    assert np.abs(np.sqrt((d * d).sum(-1)) - 1).max() < 1e-6
    cu, cv, cw = (_vec(v).astype(np.float64) for v in (cam.desc.u, cam.desc.v, cam.desc.w))
    up = d @ cv
    assert (up[:, 0] > 0.9).all() and (up[:, -1] < -0.9).all()      # the top row looks up
    assert ((d @ cw) > 0).any() and ((d @ cw) < 0).any() and ((d @ cu) > 0).any() and ((d @ cu) < 0).any()
    assert (rec["skip"] == 3).all() and (bits(rec["origin"]) == bits(_vec(cam.desc.origin))).all()
    assert ((rec["time"] >= 0.25) & (rec["time"] < 0.75)).all() and len(set(rec["time"].reshape(-1).tolist())) > 900


@pytest.mark.parametrize("name", ["orthographic", "fisheye", "equirect"])
def test_the_image_centre_looks_along_minus_w(name, monkeypatch):
    nx, ny = 16, 12
    cam = view(nx=nx, ny=ny)
    _centre_draws(monkeypatch, 0.0, 0.0)                 # pixel (8, 6) with no jitter: s = t = 0.5 exactly
    o, d, time, skip = lens_sample(cam, rtnw.lens_params(MODELS[name], 200.0), nx, ny, 8, 6, 0, 1)
    cw = _vec(cam.desc.w)
    assert np.abs(d.astype(np.float64) + cw).max() < 1e-6, (d, cw)
    assert skip == 3 and time == F(0.5)
    if name != "equirect":
        assert np.array_equal(bits(d), bits(-cw))        # r == 0: -w itself
    assert np.array_equal(bits(o), bits(_vec(cam.desc.origin)))


@pytest.mark.parametrize("fov", [60.0, 180.0, 270.0, 360.0])
def test_a_fisheye_ray_on_the_circle_lies_at_half_the_angle(fov, monkeypatch):
    nx, ny = 16, 12
    cam = view(nx=nx, ny=ny)
    cw = _vec(cam.desc.w).astype(np.float64)
    for x, j in ((0, 6), (8, 0), (8, 12), (16, 6)):       # s or t of 0 or 1 with the other at 0.5: r == 1
        _centre_draws(monkeypatch, 0.0, 0.0)
        _, d, _, _ = lens_sample(cam, rtnw.lens_params(rtnw.RT_LENS_FISHEYE, fov), nx, ny, x, j, 0, 1)
        d = d.astype(np.float64)
        angle = np.arctan2(np.linalg.norm(np.cross(d, -cw)), d @ -cw)
        assert abs(angle - np.radians(fov / 2)) < 1e-5, (fov, x, j, angle)


def test_equirect_columns_meet_at_the_seam(monkeypatch):
    nx, ny = 16, 12
    cam = view(nx=nx, ny=ny)
    lens = rtnw.lens_params(rtnw.RT_LENS_EQUIRECT)
    cw = _vec(cam.desc.w).astype(np.float64)
    for j, d1 in ((0, 0.3), (6, 0.0), (11, 0.9)):
        _centre_draws(monkeypatch, 1e-9, d1)
        _, left, _, _ = lens_sample(cam, lens, nx, ny, 0, j, 0, 1)          # s -> 0
        _centre_draws(monkeypatch, 1 - 1e-9, d1)
        _, right, _, _ = lens_sample(cam, lens, nx, ny, nx - 1, j, 0, 1)    # s -> 1
        assert np.abs(left.astype(np.float64) - right).max() < 1e-6, (j, left, right)
        if j == 6:
            assert np.abs(left - cw).max() < 1e-6                            # the seam looks backwards, along +w


def test_orthographic_rays_are_parallel_from_the_plane_through_the_origin():
    cam, rec = _frame(rtnw.RT_LENS_ORTHOGRAPHIC)
    cw = _vec(cam.desc.w)
    assert (bits(rec["dir"]) == bits(-cw)).all()
    off = rec["origin"].astype(np.float64) - _vec(cam.desc.origin)
    hor, ver = (_vec(v).astype(np.float64) for v in (cam.desc.horizontal, cam.desc.vertical))
    assert np.abs(off @ cw.astype(np.float64)).max() < 1e-5                  # in the plane through origin, normal w
    a, b = off @ hor / (hor @ hor), off @ ver / (ver @ ver)
    assert a.min() < -0.45 and a.max() > 0.45 and b.min() < -0.45 and b.max() > 0.45 and np.abs(a).max() <= 0.5 + 1e-6
    assert (rec["skip"] == 3).all()


def test_a_closed_shutter_consumes_its_draw_unused():
    cam, rec = _frame(rtnw.RT_LENS_EQUIRECT, spp=2, t0=0.4, t1=0.4)
    assert (rec["time"] == F(0.4)).all() and (rec["skip"] == 3).all()


# ------------------------------------------------------------------ the reduction rule
def test_lens_reduce_is_the_renders_rule():
    rng = np.random.default_rng(2)
    rgb = rng.uniform(0, 4, (5, 2, 3, 3)).astype(F)
    img, mom, guides = lens_reduce(rgb)
    assert guides is None
    acc = F(0)
    for s in range(5):
        acc = acc + rgb[s, 1, 2, 0]
    assert img[1, 2, 0] == acc * F(1.0 / 5)
    y =(rgb[..., 0] + rgb[..., 1]) + rgb[..., 2]
    m2 = F(0)
    for s in range(5):
        m2 = m2 + y[s, 0, 1] * y[s, 0, 1]
    assert mom[0, 1, 1] == m2
    hits = dict(prim=np.array([3, -1, -2, 0, 5], np.int32).reshape(5, 1, 1), depth=np.arange(5, dtype=F).reshape(5, 1, 1),
                normal=np.ones((5, 1, 1, 3), F), albedo=np.full((5, 1, 1, 3), 0.5, F))
    _, _, g = lens_reduce(rgb[:, :1, :1], hits)
    assert g.shape == (1, 1, 8) and g[0, 0, 3] == F(3) * F(1.0 / 5) and g[0, 0, 7] == F(10) * F(1.0 / 5)


# ------------------------------------------------------------------ the batch planner
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lens_plan") / "lens_plan_check")
    host = os.path.join(PKG, "csrc", "host")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
                          "-I", host, os.path.join(host, "job_plan.cpp"), os.path.join(ROOT, "tests", "native", "lens_plan_check.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def lens_plan(exe, npix, spp, knob=None):
    out = subprocess.run([exe, str(npix), str(spp)] + ([knob] if knob is not None else []), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    head = [int(v) for v in out[0].split()]
    return head, np.array([[int(v) for v in line.split()] for line in out[1:] if line], np.int64).reshape(-1, 4)


@pytest.mark.parametrize("npix, spp, knob, limit", [
    (63, 5, "1", 1), (63, 5, "10", 10), (63, 5, "62", 62), (63, 5, "63", 63), (63, 5, "100", 100), (63, 5, "189", 189),
    (63, 5, None, 2 ** 21), (63, 5, "0", 2 ** 21), (63, 5, "junk", 2 ** 21), (1, 1, "1", 1), (130, 2, "64", 64),
    (2 ** 21 + 5, 3, None, 2 ** 21), (2 ** 19, 16, None, 2 ** 21), (100, 3, str(2 ** 40), 2 ** 24)])
def test_every_pixel_and_sample_lands_in_exactly_one_batch(plan_exe, npix, spp, knob, limit):
    (got_limit, pix_per, smp_per, nblocks, nruns, nbatches, rays_per), b = lens_plan(plan_exe, npix, spp, knob)
    assert got_limit == limit and len(b) == nbatches == nblocks * nruns and rays_per == pix_per * smp_per
    seen = np.zeros((spp, npix), np.uint8)
    last = {}
    for p0, np_, s0, ns in b.tolist():
        assert np_ >= 1 and ns >= 1 and np_ * ns <= min(limit, rays_per) and np_ * ns < 2 ** 31
        seen[s0:s0 + ns, p0:p0 + np_] += 1
        assert last.get(p0, 0) == s0          # a block's runs come in sample order, without a gap
        last[p0] = s0 + ns
    assert (seen == 1).all()
    if limit >= npix * spp:
        assert nbatches == 1
