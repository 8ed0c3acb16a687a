"""Ray queries (rt_trace_rays, rt_occluded) without a GPU: the interface in the
header and in rtnw.py, the argument checks (all made before any HIP call), and the numpy
float32 statements the GPU tests (tests/test_gpu_trace.py) hold the kernel to:

  camera_rays         the oracle's camera rays of a pinhole camera with a closed shutter, rebuilt
                      outside it: u = float32(i + draw0) / float32(nx), v likewise, and
                      dir = ((llc + u * hor) + v * ver) - origin, component-wise (camera.h:41-56
                      with lens_radius 0: the lens offset is zero);
  first_hits_spheres  sphere.h:25-52 over a list of spheres under hitable_list.h:20-32;
  expected_with_tmax  what a bounded query returns, from the unbounded result.

The first two are held to oracle.first_hits_desc here, bit for bit, on a scene of two spheres.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import gen_scenes as G
import oracle as O
import rtnw

RT_ERR_INVALID = -1
FLT_MAX = np.float32(np.finfo(np.float32).max)
ENTRIES = ("rt_trace_rays", "rt_trace_rays_dev", "rt_occluded", "rt_occluded_dev")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ the statements
def pinhole(case, T):
    """The case's view through a pinhole whose shutter is closed at time T."""
    aspect = float(np.float32(case.nx) / np.float32(case.ny))
    focus = float(np.linalg.norm(np.subtract(case.lookfrom, case.lookat)))
    return rtnw.Camera(case.lookfrom, case.lookat, (0, 1, 0), case.vfov, aspect, 0.0, focus, T, T)


def camera_rays(cam, nx, ny, spp, seed):
    """(origin [n, 3], dir [n, 3], time [n]) float32 of the oracle's camera samples, n = ny * nx * spp
    in oracle.first_hits_desc's order (row, column, sample), for a camera with lens_radius 0
    and time0 == time1."""
    d = cam.desc
    assert d.lens_radius == 0.0 and d.time0 == d.time1, "camera_rays states a pinhole with a closed shutter"
    f = np.float32
    llc, hor, ver, org = (np.array(list(v), f) for v in (d.lower_left_corner, d.horizontal, d.vertical, d.origin))
    u = np.zeros((ny, nx, spp), f)
    v = np.zeros((ny, nx, spp), f)
    for row in range(ny):
        j = ny - 1 - row
        for i in range(nx):
            for s in range(spp):
                d0, d1 = O.counter_draws(seed, j * nx + i, s, 2)
                u[row, i, s] = f(i + d0) / f(nx)     # (float)(i + draw) / (float)nx
                v[row, i, s] = f(j + d1) / f(ny)
    u, v = u.reshape(-1, 1), v.reshape(-1, 1)
    dirs = ((llc + u * hor) + v * ver) - org
    assert dirs.dtype == f
    n = len(dirs)
    return np.broadcast_to(org, (n, 3)).copy(), dirs, np.full(n, d.time0, f)


def first_hits_spheres(origin, dirs, spheres, t_min, t_max):
    """hitable_list::hit over `spheres` ([m, 4] float32: centre, radius; list order) for rays
    (origin, dirs [n, 3]; t_min, t_max scalars or [n]) in float32: (prim [n] int32, -1 a miss;
    t [n] float32, 0 on a miss).  A t_max at or above FLT_MAX is MAXFLOAT."""
    f = np.float32
    o, d = np.asarray(origin, f).reshape(-1, 3), np.asarray(dirs, f).reshape(-1, 3)
    n = len(d)
    t_min = np.broadcast_to(np.asarray(t_min, f), (n,))
    closest = np.minimum(np.broadcast_to(np.asarray(t_max, f), (n,)), FLT_MAX).astype(f)
    prim = np.full(n, -1, np.int32)

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    a = dot(d, d)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k, s in enumerate(np.asarray(spheres, f).reshape(-1, 4)):
            oc = o - s[:3]
            b = dot(oc, d)
            c = dot(oc, oc) - s[3] * s[3]
            disc = b * b - a * c
            root = np.sqrt(np.where(disc > 0, disc, f(0)))
            t1 = (-b - root) / a
            ok1 = (disc > 0) & (t1 < closest) & (t1 > t_min)            # sphere.h:33
            t2 = (-b + root) / a
            ok2 = (disc > 0) & ~ok1 & (t2 < closest) & (t2 > t_min)     # sphere.h:42
            t = np.where(ok1, t1, t2)
            take = ok1 | ok2
            closest = np.where(take, t, closest).astype(f)
            prim[take] = k
    return prim, np.where(prim >= 0, closest, f(0)).astype(f)


def expected_with_tmax(hit, t_max):
    """The result of a query bounded by t_max ([n]) from the unbounded result `hit` (a dict as
    Scene.trace_rays returns, plus `rect` [n] bool: the hit primitive is a rect): the hit itself
    where t < t_max, or t <= t_max on a rect (aarect.h:52), else a miss."""
    t_max = np.asarray(t_max, np.float32)
    keep = (hit["prim"] >= 0) & np.where(hit["rect"], hit["t"] <= t_max, hit["t"] < t_max)
    out = {}
    for k, miss in (("prim", -1), ("material", -1), ("t", 0), ("depth", 0), ("normal", 0), ("albedo", 1)):
        a = hit[k]
        out[k] = np.where(keep.reshape((-1,) + (1,) * (a.ndim - 1)), a, np.asarray(miss, a.dtype))
    return out


def sphere_list(desc):
    """[m, 4] float32 of a descriptor whose surfaces are all plain spheres without a chain."""
    c = desc.contents
    assert all(c.prims[i].kind == 0 and c.prims[i].instance < 0 for i in range(c.nprims))
    return np.array([[c.prims[i].p[k] for k in range(4)] for i in range(c.nprims)], np.float32)


# ------------------------------------------------------------------ the interface
def test_header_declares_the_entry_points_and_records():
    text = open(rtnw.HEADER).read()
    syms = rtnw.header_symbols()
    for name in ENTRIES:
        assert name in syms, name
    for word in ("typedef struct rt_ray", "typedef struct rt_hit", "RT_HIT_MISS", "RT_HIT_INVALID", "RTNW_TRACE_BATCH"):
        assert word in text, word
    assert re.search(r"#define\s+RT_ABI_VERSION\s+2\b", text)


def test_rtnw_mirrors_the_records():
    assert ctypes.sizeof(rtnw.RtRay) == ctypes.sizeof(rtnw.RtHit) == 48
    assert rtnw.RAY_DTYPE.itemsize == rtnw.HIT_DTYPE.itemsize == 48
    for T, D in ((rtnw.RtRay, rtnw.RAY_DTYPE), (rtnw.RtHit, rtnw.HIT_DTYPE)):
        for name, _ in T._fields_:
            assert getattr(T, name).offset == D.fields[name][1], name
    assert (rtnw.RT_HIT_MISS, rtnw.RT_HIT_INVALID) == (-1, -2)
    for m in ("trace_rays", "occluded", "trace_rays_dev", "occluded_dev"):
        assert callable(getattr(rtnw.Scene, m))


def test_pack_rays_fills_the_records():
    r = rtnw.pack_rays([[1, 2, 3], [4, 5, 6]], [0, 0, -1], t_min=0.5, t_max=[7, np.inf], time=0.25)
    assert r.dtype == rtnw.RAY_DTYPE and r.shape == (2,)
    raw = r.view(np.float32).reshape(2, 12)
    assert raw[:, :8].tolist() == [[1, 2, 3, 0.5, 0, 0, -1, 7], [4, 5, 6, 0.5, 0, 0, -1, np.inf]]
    assert raw[:, 8].tolist() == [0.25, 0.25] and not raw[:, 9:].any()


def test_library_exports_the_entry_points():
    L = rtnw.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name


# ------------------------------------------------------------------ argument checks, no GPU
def _call(name, *, scene=None, rays=True, out=True, n=4):
    L = rtnw.lib()
    r = rtnw.pack_rays(np.zeros((4, 3)), (0, 0, 1))
    o = np.zeros(4, rtnw.HIT_DTYPE)
    args = [scene, r.ctypes.data if rays else None, n, o.ctypes.data if out else None, None]
    rc = getattr(L, name)(*args)
    return rc, L.rt_last_error().decode()


@pytest.mark.parametrize("name", ENTRIES)
def test_null_rays_or_output_is_invalid(name):
    rc, msg = _call(name, rays=False)
    assert rc == RT_ERR_INVALID and name + ":" in msg and "null rays" in msg, (rc, msg)
    rc, msg = _call(name, out=False)
    assert rc == RT_ERR_INVALID and name + ":" in msg and "null output" in msg, (rc, msg)


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("n", [-1, 2 ** 31])
def test_ray_counts_outside_the_range_are_invalid(name, n):
    rc, msg = _call(name, n=n)
    assert rc == RT_ERR_INVALID and name + ":" in msg and "n must be" in msg, (rc, msg)


@pytest.mark.parametrize("name", ENTRIES)
def test_null_scene_is_invalid(name):
    rc, msg = _call(name)
    assert rc == RT_ERR_INVALID and name + ":" in msg and "null scene" in msg, (rc, msg)


@pytest.mark.parametrize("name", ENTRIES)
def test_no_rays_is_ok_even_without_a_scene(name):
    rc, _ = _call(name, n=0)
    assert rc == rtnw.RT_OK
    rc, _ = _call(name, n=0, rays=False, out=False)
    assert rc == rtnw.RT_OK


# ------------------------------------------------------------------ the statements against the oracle
def two_spheres(b):
    b.add(b.sphere((0, -100.5, -1), 100, b.lambert()), b.sphere((0.2, 0.6, 0), 0.9, b.lambert()))


def test_camera_rays_and_the_sphere_statement_equal_the_oracle_bit_for_bit():
    case = G.Case(name="trace_two_spheres", make=two_spheres, seed=5, nx=32, ny=16, spp=4, lookfrom=(0.0, 1.5, 6.0),
                  lookat=(0.0, 0.5, 0.0))
    desc, cam = case.builder().desc(), pinhole(case, 0.0)
    fh = O.first_hits_desc(desc, cam, O.desc_spec(case.nx, case.ny, case.spp, max_depth=4, background="sky", seed=case.seed))
    o, d, time = camera_rays(cam, case.nx, case.ny, case.spp, case.seed)
    assert len(d) == 2048 and (time == 0).all()
    prim, t = first_hits_spheres(o, d, sphere_list(desc), 0.001, np.inf)
    depth = t * np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    share = float(np.mean(prim >= 0))
    print(f"hit share {share:.3f}; prims hit {sorted(set(prim.tolist()))}")
    assert 0.05 < share < 0.95 and set(prim.tolist()) == {-1, 0, 1}
    assert np.array_equal(prim, fh["prim"].reshape(-1))
    assert np.array_equal(bits(depth), bits(fh["depth"].reshape(-1)))


def test_the_sphere_statement_bounds():
    """t_min and t_max are exclusive for a sphere; behind t_min the far root is the hit."""
    sph = np.array([[0, 0, -5, 1]], np.float32)
    o, d = np.zeros((1, 3), np.float32), np.array([[0, 0, -1]], np.float32)

    def one(*args):
        p, t = first_hits_spheres(o, d, *args)
        return int(p[0]), float(t[0])
    assert one(sph, 0.001, np.inf) == (0, 4.0)
    assert one(sph, 0.001, 4.0) == (-1, 0.0)                      # t < t_max
    assert one(sph, 0.001, np.nextafter(np.float32(4), np.float32(9))) == (0, 4.0)
    assert one(sph, 4.0, np.inf) == (0, 6.0)                      # t > t_min: the far root
    assert one(sph, 4.0, 6.0) == (-1, 0.0)
    assert one(sph, 6.0, np.inf) == (-1, 0.0)
    assert one(np.vstack([sph, sph]), 0.001, FLT_MAX) == (0, 4.0)   # the earlier of a tie


def test_expected_with_tmax_keeps_a_rect_at_its_own_t():
    hit = dict(prim=np.array([3, 4, -1, 5], np.int32), material=np.array([1, 2, -1, 0], np.int32),
               t=np.array([2, 2, 0, 2], np.float32), depth=np.array([4, 4, 0, 4], np.float32),
               normal=np.ones((4, 3), np.float32), albedo=np.full((4, 3), 0.5, np.float32),
               rect=np.array([False, True, False, False]))
    e = expected_with_tmax(hit, np.array([2, 2, 2, 3], np.float32))
    assert e["prim"].tolist() == [-1, 4, -1, 5] and e["material"].tolist() == [-1, 2, -1, 0]
    assert e["t"].tolist() == [0, 2, 0, 2] and e["depth"].tolist() == [0, 4, 0, 4]
    assert e["normal"][:, 0].tolist() == [0, 1, 0, 1] and e["albedo"][:, 0].tolist() == [1, 0.5, 1, 0.5]
