"""The ray, radiance and lens queries on the GPU held to the oracle on rays that no camera makes
(DESIGN.md §7l): the families of tests/free_rays.py (origins anywhere in and around the scene,
rays continued from a surface, grazing rays, per-ray bounds on both sides, scaled directions),
records whose key fields span the uint32 range with every edge of `skip`, hand-placed origins
inside glass, inside every medium and on every light, and lens views from inside the scene.
The oracle's entries (oracle.trace_rays_desc, oracle.radiance_rays_desc) are pinned to the
reference on the CPU by tests/test_free_rays_spec.py, which also holds every (case, family) to
the conditions that make it worth running.

The ray queries are compared bit for bit, every field, no tolerance and no exclusions
(tests/test_gpu_trace.py's convention).  Radiance is compared bit for bit on every record where
the host libm is the one the device restates (oracle.host_libm_pinned); elsewhere the exact
share is printed and test_gpu_generated.check's bar is applied to the batch laid out as an image
(that file's convention).  LIBM_WHY is printed either way.
"""
import ctypes

import numpy as np
import pytest

import free_rays as R
import oracle as O
import rtnw
from test_free_rays_spec import RADIANCE_CASES, RADIANCE_FAMILIES, THREADS, TRACE_CASES, families, path_families
from test_gpu_generated import BG, check
from test_gpu_parity import LIBM_PINNED, LIBM_WHY
from test_lens_spec import MODELS, lens_reduce

pytestmark = pytest.mark.gpu

FIELDS = ("prim", "material", "t", "depth", "normal", "albedo", "pad")
F = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


_scenes = {}


def scene_of(name):
    if name not in _scenes:
        _scenes[name] = rtnw.Scene(families(name)[1])
    return _scenes[name]


# ------------------------------------------------------------------ a. ray queries
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name", TRACE_CASES)
def test_trace_rays_equal_the_oracle_in_every_bit(name, family):
    c, desc, fam, hits = families(name)
    sc, rays, want = scene_of(name), fam[family], hits[family]
    got = sc.trace_rays(rays)
    differ = {f: int((bits(got[f]) != bits(want[f])).reshape(len(rays), -1).any(axis=1).sum()) for f in FIELDS}
    print(f"{name} {family}: {len(rays)} rays, hit share {float((want['prim'] >= 0).mean()):.3f}, differing records {differ}")
    for f in FIELDS:
        assert same(got[f], want[f]), (f, differ)
    occ = sc.occluded(rays)
    assert occ.dtype == np.uint8 and np.array_equal(occ, (want["prim"] >= 0).astype(np.uint8))


def test_the_device_forms_equal_the_oracle_too():
    L = rtnw.lib()
    name, family = "chains_long", "continued"
    c, desc, fam, hits = families(name)
    sc, rays, want = scene_of(name), fam[family], hits[family]
    n = len(rays)
    dev = ctypes.c_void_p()
    rtnw._check(L.rt_device_alloc(0, n * (48 + 48 + 1), ctypes.byref(dev)))
    try:
        d_rays, d_hits, d_occ = dev.value, dev.value + 48 * n, dev.value + 96 * n
        rtnw._check(L.rt_copy_to_device(ctypes.c_void_p(d_rays), rays.ctypes.data, rays.nbytes))
        sc.trace_rays_dev(d_rays, n, d_hits)
        sc.occluded_dev(d_rays, n, d_occ)
        got = np.zeros(n, rtnw.HIT_DTYPE)
        occ = np.zeros(n, np.uint8)
        rtnw._check(L.rt_copy_to_host(got.ctypes.data, ctypes.c_void_p(d_hits), got.nbytes))
        rtnw._check(L.rt_copy_to_host(occ.ctypes.data, ctypes.c_void_p(d_occ), n))
    finally:
        L.rt_device_free(dev)
    for f in FIELDS:
        assert same(got[f], want[f]), f
    assert np.array_equal(occ, (want["prim"] >= 0).astype(np.uint8))


# ------------------------------------------------------------------ b. radiance queries
def assert_radiance(what, got, want, shape):
    """Bits on every record where the host libm is pinned; else check()'s bar on the batch as an image."""
    assert got.dtype == rtnw.RADIANCE_DTYPE and (got["status"] == 0).all()
    exact = float((bits(got["rgb"]) == bits(want["rgb"])).all(axis=1).mean())
    print(f"{what}: {len(got)} records, bit-exact share {exact:.4f}, lit share {float((want['rgb'] > 0).any(axis=1).mean()):.3f}; "
          f"host libm pinned: {LIBM_PINNED} ({LIBM_WHY})")
    if LIBM_PINNED:
        assert same(got["rgb"], want["rgb"]), what
    else:
        check(what, got["rgb"].reshape(shape), want["rgb"].reshape(shape))


def query(name, rec, max_depth=None, background=None):
    """(the GPU's records, the oracle's) of a case's records in kernel order."""
    c, desc, _, _ = families(name)
    depth = c.max_depth if max_depth is None else max_depth
    bg = background or c.background
    p = rtnw.RenderParams(5, 3, 2, chunk=2, sample_offset=7, max_depth=depth, background=BG[bg], seed=c.seed)   # the frame is ignored
    return scene_of(name).radiance_rays(p, rec), O.radiance_rays_desc(desc, rec, max_depth=depth, background=bg, seed=c.seed,
                                                                      threads=THREADS)


@pytest.mark.parametrize("family", RADIANCE_FAMILIES)
@pytest.mark.parametrize("name", RADIANCE_CASES)
def test_radiance_rays_equal_the_oracle(name, family):
    rec = path_families(name)[family]
    got, want = query(name, rec)
    assert_radiance(f"{name} {family}", got, want, (32, 48, 3))
    assert (want["rgb"] > 0).any()


@pytest.mark.parametrize("name", RADIANCE_CASES)
def test_radiance_from_inside_glass_media_and_on_lights_equals_the_oracle(name):
    pf = path_families(name)
    rec, labels = pf["hand"], pf["hand_labels"]
    assert len(rec) > 0 and len(rec) % 16 == 0
    got, want = query(name, rec)
    assert_radiance(f"{name} hand-placed {sorted(set(labels.tolist()))}", got, want, (-1, 16, 3))


# black needs a light to see: textures_by_kind has the cases' only ones (it is black by default, so sky is its variant)
VARIANTS = [(50, "sky", "textures_by_kind"), (50, "black", "textures_by_kind"), (1, "sky", "boundaries_bvh"),
            (1, "black", "textures_by_kind"), (0, "sky", "chains_long"), (0, "black", "textures_by_kind")]


@pytest.mark.parametrize("max_depth,background,name", VARIANTS)
def test_radiance_depth_limits_and_backgrounds_equal_the_oracle(max_depth, background, name):
    rec = path_families(name)["continued"]
    got, want = query(name, rec, max_depth, background)
    assert_radiance(f"{name} continued, max_depth {max_depth}, {background}", got, want, (32, 48, 3))
    assert (want["rgb"] > 0).any()
    if max_depth == 0 and background == "black":    # nothing scatters: only a light seen directly is lit
        assert (want["rgb"] == 0).all(axis=1).mean() > 0.5


# ------------------------------------------------------------------ c. lens renders from inside the scene
LENS_CASES = ["scan65_mixed", "media9_bvh"]
LENSES = [("fisheye", 200.0), ("fisheye", 360.0), ("equirect", 0.0), ("orthographic", 0.0)]
NX, NY, SPP = 16, 8, 4


def inside_view():
    """A tilted camera with a lens and an open shutter among the scene's objects."""
    return rtnw.Camera((0.3, 1.0, 0.5), (-1.0, 0.8, -2.0), (0.1, 1, 0), 55.0, float(F(NX) / F(NY)), 0.1, 2.5, 0.0, 1.0)


@pytest.mark.parametrize("model,fov", LENSES, ids=[f"{m}{int(f) or ''}" for m, f in LENSES])
@pytest.mark.parametrize("name", LENS_CASES)
def test_a_lens_render_from_inside_is_its_records_through_the_oracle(name, model, fov):
    c, desc, _, _ = families(name)
    sc, cam, lens = scene_of(name), inside_view(), rtnw.lens_params(MODELS[model], fov or 180.0)
    depth = min(c.max_depth, 8)
    p = rtnw.RenderParams(NX, NY, SPP, chunk=1, seed=c.seed, sample_offset=2, max_depth=depth, background=BG[c.background])
    img, mom, gd = sc.render_lens(cam, p, lens, 0, 0, NX, NY, moments=True, guides=True)
    rec, tr = rtnw.lens_rays(cam, p, lens, 0, 0, NX, NY, trace=True)     # held to the numpy statement by test_gpu_lens.py
    rec, tr = rec.reshape(-1), tr.reshape(-1)
    valid = (rec["dir"] != 0).any(axis=1)                                # a fisheye sample outside the circle has no ray
    assert valid.any() and (not valid.all()) == (model == "fisheye")
    n = len(rec)
    rgb = np.zeros((n, 3), F)
    rgb[valid] = O.radiance_rays_desc(desc, rec[valid], max_depth=depth, background=c.background, seed=c.seed,
                                      threads=THREADS)["rgb"]
    h = O.trace_rays_desc(desc, tr[valid], THREADS)
    hits = dict(prim=np.full(n, rtnw.RT_HIT_INVALID, np.int32), depth=np.zeros(n, F), normal=np.zeros((n, 3), F),
                albedo=np.ones((n, 3), F))
    for k in hits:
        hits[k][valid] = h[k]
    hits = {k: v.reshape((SPP, NY, NX) + v.shape[1:]) for k, v in hits.items()}
    want, want_mom, want_gd = lens_reduce(rgb.reshape(SPP, NY, NX, 3), hits)
    exact = float((bits(img) == bits(want)).all(axis=-1).mean())
    print(f"{name} {model} {fov}: bit-exact pixels {exact:.4f}, coverage {float(want_gd[..., 3].mean()):.3f}, "
          f"rays {int(valid.sum())} of {n}; host libm pinned: {LIBM_PINNED} ({LIBM_WHY})")
    assert (want > 0).any() and 0.05 < want_gd[..., 3].mean() <= 1.0
    assert same(gd[..., 3:], want_gd[..., 3:])        # coverage, normal, depth: no libm in them
    if LIBM_PINNED:
        assert same(img, want) and same(mom, want_mom) and same(gd, want_gd)
    else:
        check(f"{name} {model} image", img, want)
        check(f"{name} {model} moments", mom, want_mom)
        check(f"{name} {model} guide albedo", gd[..., 0:3], want_gd[..., 0:3])
