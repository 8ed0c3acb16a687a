"""Radiance queries (rt_radiance_rays) without a GPU: the interface in the header
and in rtnw.py, the argument checks (all made before any HIP call, in the header's order), and
the numpy float32 statement of the oracle's camera the GPU tests (tests/test_gpu_radiance.py)
make their rays with:

  lens_camera_rays    camera::get_ray (camera.h:41-56) for any aperture and shutter span, rebuilt
                      outside the oracle from oracle.counter_draws with the reference's operation
                      order, together with the number of draws each sample spent before color():
                      2 jitter draws, 2 per lens-disk candidate including the accepted one, 1
                      time draw.  That count is the `skip` of the ray-tracing identity.

It is held to oracle.first_hits_desc here, bit for bit, on a scene of two spheres seen through
a wide lens (which pins the accepted candidate, and with it skip), and to
test_trace_spec.camera_rays where the lens is a pinhole and the shutter is closed.
"""
import ctypes
import re

import numpy as np
import pytest

import gen_scenes as G
import oracle as O
import rtnw
from test_trace_spec import bits, camera_rays, first_hits_spheres, pinhole, sphere_list, two_spheres

RT_ERR_INVALID = -1
ENTRIES = ("rt_radiance_rays", "rt_radiance_rays_dev")


# ------------------------------------------------------------------ the camera statement
def lens_camera_rays(cam, nx, ny, spp, seed):
    """(origin [n, 3], dir [n, 3], time [n]) float32 and skip [n] uint32 of the oracle's camera
    samples, n = ny * nx * spp in oracle.first_hits_desc's order (row, column, sample); the
    sample of row `row`, column i has pixel key (ny - 1 - row) * nx + i."""
    d = cam.desc
    f = np.float32
    llc, hor, ver, org, cu, cv = (np.array(list(v), f) for v in (d.lower_left_corner, d.horizontal, d.vertical, d.origin,
                                                                 d.u, d.v))
    lens, t0, span = f(d.lens_radius), f(d.time0), f(d.time1) - f(d.time0)
    n = ny * nx * spp
    s_, t_ = np.zeros((n, 1), f), np.zeros((n, 1), f)
    px, py = np.zeros((n, 1), f), np.zeros((n, 1), f)
    time, skip = np.zeros(n, f), np.zeros(n, np.uint32)
    k = 0
    for row in range(ny):
        j = ny - 1 - row
        for i in range(nx):
            for s in range(spp):
                ndraw = 35
                while True:
                    draws = O.counter_draws(seed, j * nx + i, s, ndraw)
                    s_[k] = f(i + draws[0]) / f(nx)     # main.cpp:305-306
                    t_[k] = f(j + draws[1]) / f(ny)
                    at = 2
                    while at + 2 < ndraw:               # camera.h:6-12: do ... while (dot(p, p) >= 1.0)
                        x, y = f(2.0) * f(draws[at]) - f(1), f(2.0) * f(draws[at + 1]) - f(1)
                        at += 2
                        if (x * x + y * y) + f(0) * f(0) < f(1):
                            break
                    else:
                        ndraw *= 2
                        continue
                    px[k], py[k] = x, y
                    time[k] = f(np.float64(t0) + draws[at] * np.float64(span))   # camera.h:54
                    skip[k] = at + 1
                    break
                k += 1
    rdx, rdy = lens * px, lens * py                     # rd = lens_radius * random_in_unit_disk()
    offset = cu * rdx + cv * rdy                        # u * rd.x() + v * rd.y()
    origin = org + offset
    dirs = (((llc + s_ * hor) + t_ * ver) - org) - offset
    assert origin.dtype == f and dirs.dtype == f
    return origin, dirs, time, skip


def pixel_keys(nx, ny, spp):
    """(pixel [n], sample [n]) uint32 of lens_camera_rays' samples, in its order."""
    row, col, s = np.meshgrid(np.arange(ny), np.arange(nx), np.arange(spp), indexing="ij")
    return ((ny - 1 - row) * nx + col).reshape(-1).astype(np.uint32), s.reshape(-1).astype(np.uint32)


def camera_records(cam, nx, ny, spp, seed):
    """The rt_path_ray records ([n] rtnw.PATH_RAY_DTYPE) that restate every camera sample of the
    frame: the ray, its stream's key numbers and the draws spent before color()."""
    o, d, time, skip = lens_camera_rays(cam, nx, ny, spp, seed)
    pix, smp = pixel_keys(nx, ny, spp)
    return rtnw.pack_path_rays(o, d, time, pix, smp, skip)


# ------------------------------------------------------------------ the interface
def test_header_declares_the_entry_points_and_records():
    text = open(rtnw.HEADER).read()
    syms = rtnw.header_symbols()
    for name in ENTRIES:
        assert name in syms, name
    for word in ("typedef struct rt_path_ray", "typedef struct rt_radiance", "RTNW_RADIANCE_BATCH"):
        assert word in text, word
    m = re.search(r"#define\s+RT_RADIANCE_MAX_SKIP\s+(\d+)\b", text)
    assert m and int(m.group(1)) == rtnw.RT_RADIANCE_MAX_SKIP == 192
    assert re.search(r"#define\s+RT_ABI_VERSION\s+2\b", text)


def test_rtnw_mirrors_the_records():
    assert ctypes.sizeof(rtnw.RtPathRay) == rtnw.PATH_RAY_DTYPE.itemsize == 48
    assert ctypes.sizeof(rtnw.RtRadiance) == rtnw.RADIANCE_DTYPE.itemsize == 16
    for T, D in ((rtnw.RtPathRay, rtnw.PATH_RAY_DTYPE), (rtnw.RtRadiance, rtnw.RADIANCE_DTYPE)):
        assert [n for n, _ in T._fields_] == list(D.names)
        for name, _ in T._fields_:
            assert getattr(T, name).offset == D.fields[name][1], name
    offs = {n: rtnw.PATH_RAY_DTYPE.fields[n][1] for n in rtnw.PATH_RAY_DTYPE.names}
    assert offs == dict(origin=0, time=12, dir=16, skip=28, pixel=32, sample=36, pad=40)
    assert {n: rtnw.RADIANCE_DTYPE.fields[n][1] for n in rtnw.RADIANCE_DTYPE.names} == dict(rgb=0, status=12)
    for m in ("radiance_rays", "radiance_rays_dev"):
        assert callable(getattr(rtnw.Scene, m))


def test_pack_path_rays_fills_the_records():
    r = rtnw.pack_path_rays([[1, 2, 3], [4, 5, 6]], [0, 0, -1], time=0.25, pixel=[7, 2 ** 32 - 1], sample=9, skip=[5, 192])
    assert r.dtype == rtnw.PATH_RAY_DTYPE and r.shape == (2,)
    raw = r.view(np.uint32).reshape(2, 12)
    assert raw[:, :7].view(np.float32).tolist() == [[1, 2, 3, 0.25, 0, 0, -1], [4, 5, 6, 0.25, 0, 0, -1]]
    assert raw[:, 7:10].tolist() == [[5, 7, 9], [192, 2 ** 32 - 1, 9]] and not raw[:, 10:].any()


def test_library_exports_the_entry_points():
    L = rtnw.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name


# ------------------------------------------------------------------ argument checks, no GPU
def _call(name, *, scene=None, params=True, rays=True, out=True, n=4, **pkw):
    L = rtnw.lib()
    r = rtnw.pack_path_rays(np.zeros((4, 3)), (0, 0, 1))
    o = np.zeros(4, rtnw.RADIANCE_DTYPE)
    kw = dict(max_depth=5, t_min=0.001, background=rtnw.RT_BG_SKY, seed=3)
    kw.update(pkw)
    p = rtnw.RenderParams(0, 0, 0, **kw)    # nx, ny, spp are ignored: zeros are fine
    args = [scene, ctypes.byref(p) if params else None, r.ctypes.data if rays else None, n,
            o.ctypes.data if out else None, None]
    rc = getattr(L, name)(*args)
    return rc, L.rt_last_error().decode()


def _invalid(name, word, **kw):
    rc, msg = _call(name, **kw)
    assert rc == RT_ERR_INVALID and name + ":" in msg and word in msg, (rc, msg, kw)


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("n", [-1, 2 ** 31])
def test_ray_counts_outside_the_range_are_invalid(name, n):
    # the count comes first: everything else is wrong too
    _invalid(name, "n must be", n=n, params=False, rays=False, out=False)
    _invalid(name, "n must be", n=n)


@pytest.mark.parametrize("name", ENTRIES)
def test_no_rays_is_ok_even_without_a_scene(name):
    assert _call(name, n=0)[0] == rtnw.RT_OK
    assert _call(name, n=0, params=False, rays=False, out=False)[0] == rtnw.RT_OK
    assert _call(name, n=0, max_depth=-1, flags=rtnw.RT_FLAG_COUNT)[0] == rtnw.RT_OK


@pytest.mark.parametrize("name", ENTRIES)
def test_null_arguments_and_bad_parameters_are_invalid_before_the_scene(name):
    # every call has a null scene: the argument named is reported, not the scene
    _invalid(name, "null parameters", params=False)
    _invalid(name, "null rays", rays=False)
    _invalid(name, "null output", out=False)
    _invalid(name, "max_depth", max_depth=-1)
    for t in (np.nan, np.inf, -np.inf):
        _invalid(name, "t_min", t_min=t)
    for bg in (-1, 2):
        _invalid(name, "background", background=bg)
    for flag in (rtnw.RT_FLAG_COUNT, rtnw.RT_FLAG_PROFILE, rtnw.RT_FLAG_SUM_IN, rtnw.RT_FLAG_SUM_OUT,
                 rtnw.RT_FLAG_RIGHT_FOLD, 32, -1):
        _invalid(name, "flag", flags=flag)
    assert _call(name, max_depth=0)[1].find("null scene") >= 0   # max_depth 0 is legal


@pytest.mark.parametrize("name", ENTRIES)
def test_null_scene_is_invalid(name):
    _invalid(name, "null scene")


# ------------------------------------------------------------------ the statement against the oracle
def lens_case(**kw):
    return G.Case(name="radiance_two_spheres", make=two_spheres, seed=5, nx=32, ny=16, spp=4, lookfrom=(0.0, 1.5, 6.0),
                  lookat=(0.0, 0.5, 0.0), **kw)


def test_lens_camera_rays_and_the_sphere_statement_equal_the_oracle_bit_for_bit():
    case = lens_case(aperture=0.3)
    desc, cam = case.builder().desc(), case.camera()
    assert cam.desc.lens_radius == np.float32(0.15) and (cam.desc.time0, cam.desc.time1) == (0.0, 1.0)
    fh = O.first_hits_desc(desc, cam, O.desc_spec(case.nx, case.ny, case.spp, max_depth=4, background="sky", seed=case.seed))
    o, d, time, skip = lens_camera_rays(cam, case.nx, case.ny, case.spp, case.seed)
    assert len(d) == 2048 and ((time >= 0) & (time < 1)).all() and len(set(time.tolist())) > 2000
    # 5 draws with the first candidate accepted (pi / 4 of the samples), 2 more per rejected one
    assert skip.min() == 5 and (skip % 2 == 1).all() and skip.max() > 7 and skip.max() <= rtnw.RT_RADIANCE_MAX_SKIP
    assert 0.70 < float(np.mean(skip == 5)) < 0.86
    assert len({tuple(x) for x in o.tolist()}) > 2000     # every sample has its own lens point
    prim, t = first_hits_spheres(o, d, sphere_list(desc), 0.001, np.inf)
    depth = t * np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    share = float(np.mean(prim >= 0))
    print(f"hit share {share:.3f}; prims hit {sorted(set(prim.tolist()))}; skips {sorted(set(skip.tolist()))}")
    assert 0.05 < share < 0.95 and set(prim.tolist()) == {-1, 0, 1}
    assert np.array_equal(prim, fh["prim"].reshape(-1))
    assert np.array_equal(bits(depth), bits(fh["depth"].reshape(-1)))


def test_a_pinhole_with_a_closed_shutter_reduces_to_camera_rays():
    case = lens_case(aperture=0.0)
    cam = pinhole(case, 0.37)
    o, d, time, skip = lens_camera_rays(cam, case.nx, case.ny, case.spp, case.seed)
    o0, d0, time0 = camera_rays(cam, case.nx, case.ny, case.spp, case.seed)
    assert np.array_equal(bits(o), bits(o0)) and np.array_equal(bits(d), bits(d0)) and np.array_equal(bits(time), bits(time0))
    assert skip.min() == 5 and skip.max() > 5    # the disk is drawn even when the lens radius is 0


def test_pixel_keys_follow_the_order_of_the_rays():
    pix, smp = pixel_keys(3, 2, 2)
    assert pix.tolist() == [3, 3, 4, 4, 5, 5, 0, 0, 1, 1, 2, 2] and smp.tolist() == [0, 1] * 6
