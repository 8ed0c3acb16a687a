"""Lens renders on the GPU (rt_lens_rays, rt_render_lens and their _dev forms) held
to rt_hip.h's contracts: the records are tests/test_lens_spec.py's statement; with
RT_LENS_PERSPECTIVE the render is rt_render_tile(chunk = 1), its moments and its feature guides,
bit for bit; for every model it is the library's own records fed through the radiance and ray
queries and reduced by lens_reduce, bit for bit; and it depends neither on the batch size nor on
the tile split.  Where the statement needs a sine, bits are asserted on a host whose libm is the
one the device restates (oracle.host_libm_pinned); elsewhere the pin state is printed and origin
and direction are held to 1 ulp, the integer fields staying exact.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import gen_scenes as G
import oracle as O
import rtnw
from test_gpu_generated import BG
from test_lens_spec import MODELS, lens_records, lens_reduce, view

pytestmark = pytest.mark.gpu

LIBM_PINNED, LIBM_WHY = O.host_libm_pinned()
NX, NY, SPP, OFFSET, TILE = 16, 12, 5, 3, (3, 2, 9, 7)     # the tile's 63 * 5 rays are no multiple of 64
FRAMES = [(NX, NY, SPP, OFFSET), (1, 1, 1, 0), (65, 1, 2, 0)]   # ... the first and last lanes of a wave and of a block
IDENTITY = ["scan64_mixed", "scan65_mixed", "cloud1736", "media9_bvh"]
COMPOSE = ["scan64_mixed", "media9_bvh"]
RT_ERR_INVALID, RT_ERR_UNSUPPORTED = -1, -4
F = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def ulps(a, b):
    """The distance of two float32 arrays in units in the last place (+0 and -0 are 0 apart)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def lens_of(name, fov=200.0):
    return rtnw.lens_params(MODELS[name], fov)


def frame_params(nx=NX, ny=NY, spp=SPP, offset=OFFSET, seed=9, **kw):
    kw = dict(dict(max_depth=6, background=rtnw.RT_BG_SKY), **kw)
    return rtnw.RenderParams(nx, ny, spp, chunk=1, seed=seed, sample_offset=offset, **kw)


_statements = {}


def statement(name, nx, ny, spp, offset):
    """(camera, records, trace records) of a frame by the CPU statement, made once."""
    key = (name, nx, ny, spp, offset)
    if key not in _statements:
        cam = view(nx=nx, ny=ny)
        _statements[key] = (cam,) + lens_records(cam, lens_of(name), nx, ny, spp, 9, sample_offset=offset)
    return _statements[key]


def assert_records(name, got, want):
    """Bits where nothing but + - * / sqrt is involved or the host libm is pinned; else 1 ulp on
    origin and direction, every other field exact."""
    if name == "perspective" or LIBM_PINNED:
        assert same(got, want), name
        return
    print(f"{name}: host libm not pinned ({LIBM_WHY}): origin and direction held to 1 ulp")
    for field in got.dtype.names:
        if field in ("origin", "dir"):
            assert ulps(got[field], want[field]).max() <= 1, (name, field)
            assert np.array_equal(got[field] == 0, want[field] == 0), (name, field)    # a no-ray sample stays one
        else:
            assert same(got[field], want[field]), (name, field)


# ------------------------------------------------------------------ 1. the records
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "x".join(map(str, f[:3])))
@pytest.mark.parametrize("name", list(MODELS))
def test_records_equal_the_statement(name, frame):
    nx, ny, spp, offset = frame
    cam, want, want_tr = statement(name, nx, ny, spp, offset)
    p = frame_params(nx, ny, spp, offset)
    got, got_tr = rtnw.lens_rays(cam, p, lens_of(name), 0, 0, nx, ny, trace=True)
    assert got.shape == (spp, ny, nx) and got.dtype == rtnw.PATH_RAY_DTYPE and got_tr.dtype == rtnw.RAY_DTYPE
    assert_records(name, got, want)
    assert_records(name, got_tr, want_tr)
    # the trace records restate the library's own rays: t_min, +inf, the same time, nothing else
    for field in ("origin", "dir", "time"):
        assert same(got_tr[field], got[field]), field
    assert (got_tr["t_min"] == F(0.001)).all() and np.isposinf(got_tr["t_max"]).all() and not bits(got_tr["pad"]).any()
    assert not got["pad"].any()
    assert same(rtnw.lens_rays(cam, p, lens_of(name), 0, 0, nx, ny), got)     # without the trace records
    if name == "fisheye" and nx == NX:
        zero = (got["dir"] == 0).all(-1)
        assert zero.any() and not zero.all()


@pytest.mark.parametrize("name", list(MODELS))
def test_a_tile_is_the_crop_of_the_frames_records(name):
    cam, want, want_tr = statement(name, NX, NY, SPP, OFFSET)
    x0, y0, w, h = TILE
    got, got_tr = rtnw.lens_rays(cam, frame_params(), lens_of(name), x0, y0, w, h, trace=True)
    assert_records(name, got, np.ascontiguousarray(want[:, y0:y0 + h, x0:x0 + w]))
    assert_records(name, got_tr, np.ascontiguousarray(want_tr[:, y0:y0 + h, x0:x0 + w]))
    full = rtnw.lens_rays(cam, frame_params(), lens_of(name), 0, 0, NX, NY)
    assert same(got, full[:, y0:y0 + h, x0:x0 + w])


@pytest.mark.parametrize("name", list(MODELS))
def test_the_device_form_on_a_callers_stream_writes_the_same_records(name):
    import torch
    cam = view()
    x0, y0, w, h = TILE
    n = w * h * SPP
    want, want_tr = rtnw.lens_rays(cam, frame_params(), lens_of(name), x0, y0, w, h, trace=True)
    stream = torch.cuda.Stream()
    d_rays = torch.full((n * 48 + 48,), 0xAB, dtype=torch.uint8, device="cuda")     # one record of slack: stays untouched
    d_tr = torch.full((n * 48 + 48,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert d_rays.data_ptr() % 16 == 0 and d_tr.data_ptr() % 16 == 0
    rtnw.lens_rays_dev(cam, frame_params(), lens_of(name), x0, y0, w, h, d_rays.data_ptr(), d_tr.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    rays, tr = d_rays.cpu().numpy(), d_tr.cpu().numpy()
    assert same(rays[:n * 48].view(rtnw.PATH_RAY_DTYPE).reshape(SPP, h, w), want)
    assert same(tr[:n * 48].view(rtnw.RAY_DTYPE).reshape(SPP, h, w), want_tr)
    assert (rays[n * 48:] == 0xAB).all() and (tr[n * 48:] == 0xAB).all()


# ------------------------------------------------------------------ scenes, one object per case
_scenes = {}


def scene(name):
    """(case, scene, camera of the 16 x 12 frame) of a generated case, made once."""
    if name not in _scenes:
        c = G.BY_NAME[name]
        aspect = float(F(NX) / F(NY))
        focus = float(np.linalg.norm(np.subtract(c.lookfrom, c.lookat)))
        cam = rtnw.Camera(c.lookfrom, c.lookat, (0, 1, 0), c.vfov, aspect, c.aperture, focus, 0.0, 1.0)
        _scenes[name] = (c, rtnw.Scene(c.builder().desc()), cam)
    return _scenes[name]


def case_params(c, **kw):
    return frame_params(max_depth=min(c.max_depth, 8), background=BG[c.background], seed=c.seed, **kw)


# ------------------------------------------------------------------ 2. the perspective identity
def test_the_identity_scenes_cover_the_search_modes_and_the_features():
    modes, moving, media, chains = set(), False, False, False
    for name in IDENTITY:
        c, sc, cam = scene(name)
        _, st = sc.render_tile(cam, case_params(c, spp=1), 0, 0, NX, NY, stats=True)
        modes.add("scan" if st["scan_groups"] > 0 else ("lds" if st["lds_level"] >= 1 else "hbm"))
        d = sc.desc.contents
        kinds = {d.prims[i].kind for i in range(d.nprims)}
        moving |= 1 in kinds and cam.desc.lens_radius > 0 and cam.desc.time1 > cam.desc.time0     # RT_PRIM_MOVING_SPHERE
        media |= d.nmedia > 0
        chains |= any(d.prims[i].instance >= 0 for i in range(d.nprims))
    assert modes == {"scan", "lds", "hbm"} and moving and media and chains, (modes, moving, media, chains)


@pytest.mark.parametrize("name", IDENTITY)
def test_perspective_is_the_render_its_moments_and_its_guides(name):
    c, sc, cam = scene(name)
    lens = lens_of("perspective")
    p = case_params(c)
    img, mom, gd = sc.render_lens(cam, p, lens, 0, 0, NX, NY, moments=True, guides=True)
    ref = sc.render_tile(cam, p, 0, 0, NX, NY)
    ref2, ref_mom = sc.render_tile_moments(cam, p, 0, 0, NX, NY)
    ref_gd = rtnw.pack_guides(sc.render_features(cam, p, 0, 0, NX, NY))
    print(f"{name}: lit share {float((ref > 0).mean()):.3f}, coverage {float(ref_gd[..., 3].mean()):.3f}")
    assert (ref > 0).any() and same(ref, ref2)
    assert same(img, ref) and same(mom, ref_mom) and same(gd, ref_gd)
    assert same(sc.render_lens(cam, p, lens, 0, 0, NX, NY), ref)            # alone, the image is the same
    x0, y0, w, h = TILE
    t_img, t_mom, t_gd = sc.render_lens(cam, p, lens, x0, y0, w, h, moments=True, guides=True)
    assert same(t_img, sc.render_tile(cam, p, x0, y0, w, h))
    crop = (slice(y0, y0 + h), slice(x0, x0 + w))
    assert same(t_img, img[crop]) and same(t_mom, mom[crop]) and same(t_gd, gd[crop])


# ------------------------------------------------------------------ 3. composition
def compose(sc, cam, p, lens, rect):
    """lens_reduce of the library's own records through the radiance and the ray queries."""
    x0, y0, w, h = rect
    rec, tr = rtnw.lens_rays(cam, p, lens, x0, y0, w, h, trace=True)
    rad = sc.radiance_rays(p, rec.reshape(-1))
    hits = sc.trace_rays(tr.reshape(-1))
    hits = {k: v.reshape((p.spp, h, w) + v.shape[1:]) for k, v in hits.items()}
    return lens_reduce(rad["rgb"].reshape(p.spp, h, w, 3), hits), rad, hits


@pytest.mark.parametrize("name", COMPOSE)
@pytest.mark.parametrize("model", list(MODELS))
def test_the_render_is_its_records_through_the_queries_reduced_by_the_rule(model, name):
    c, sc, cam = scene(name)
    lens, p = lens_of(model), case_params(c)
    for rect in ((0, 0, NX, NY), TILE):
        (want, want_mom, want_gd), rad, hits = compose(sc, cam, p, lens, rect)
        img, mom, gd = sc.render_lens(cam, p, lens, *rect, moments=True, guides=True)
        assert same(img, want) and same(mom, want_mom) and same(gd, want_gd), (model, rect)
        invalid = rad["status"] == rtnw.RT_HIT_INVALID
        assert np.array_equal(invalid, hits["prim"].reshape(-1) == rtnw.RT_HIT_INVALID)
        if rect != TILE:                                      # (the tile lies inside the image circle)
            assert invalid.any() == (model == "fisheye")      # the samples outside the circle, and no others
    assert (img > 0).any()


# ------------------------------------------------------------------ 4. a scene that needs no oracle
EMISSION = np.array([0.25, 0.5, 1.0], F)


def inside_a_light(b):
    b.add(b.sphere((0.0, 0.0, 0.0), 50.0, b.light(b.const(*EMISSION.tolist()))))


@pytest.mark.parametrize("model", ["equirect", "fisheye", "orthographic"])
def test_inside_an_emissive_sphere_every_ray_returns_the_emission(model):
    n, spp = 16, 4
    cam = rtnw.Camera((1.0, 2.0, -3.0), (0.0, 1.0, 4.0), (0, 1, 0), 40.0, 1.0, 0.0, 5.0, 0.0, 0.0)
    lens = rtnw.lens_params(MODELS[model], 180.0)
    # the CPU statement picks the pixels: how many of each pixel's samples have a ray
    rec, _ = lens_records(cam, lens, n, n, spp, 4)
    count = (rec["dir"] != 0).any(-1).sum(0)
    if model == "fisheye":
        assert (count == spp).any() and (count == 0).any() and count[0, 0] == 0 and count[n // 2, n // 2] == spp
    else:
        assert (count == spp).all()
    sc = rtnw.Scene(G.Case(name="lens_inside_a_light", make=inside_a_light, seed=1).builder().desc())
    p = rtnw.RenderParams(n, n, spp, max_depth=5, background=rtnw.RT_BG_BLACK, chunk=1, seed=4)
    img, mom, gd = sc.render_lens(cam, p, lens, 0, 0, n, n, moments=True, guides=True)
    share = (count.astype(F) * F(0.25))[..., None]        # exact: quarters
    assert same(img, share * EMISSION)                    # the emission inside, exactly 0 outside, quarters on the rim
    assert same(gd[..., 3], share[..., 0]) and same(gd[..., 0:3], share * EMISSION + (F(1) - share))   # a miss's albedo is 1
    assert same(mom[..., 0], count.astype(F) * F(1.75))
    if model == "fisheye":
        assert not bits(img[0, 0]).any() and gd[0, 0, 3] == 0 and same(img[n // 2, n // 2], EMISSION)
    sc.close()


# ------------------------------------------------------------------ 5. independence
CHILD = """
import sys
sys.path[:0] = {paths!r}
import numpy as np
import gen_scenes as G, rtnw
import test_gpu_lens as T
c, sc, cam = T.scene({name!r})
try:
    img, mom, gd = sc.render_lens(cam, T.case_params(c), T.lens_of({model!r}), *{rect!r}, moments=True, guides=True)
    rays = rtnw.lens_rays(cam, T.case_params(c), T.lens_of({model!r}), *{rect!r})
    np.savez({out!r}, img=img, mom=mom, gd=gd, rays=rays.view(np.uint8))
except rtnw.RtError as e:
    np.savez({out!r}, code=np.array([e.code]))
    print(e)
"""


def run_child(tmp_path, name, model, rect, **env):
    out = str(tmp_path / "child.npz")
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here, os.path.dirname(rtnw.__file__), os.path.dirname(O.__file__)]
    res = subprocess.run([sys.executable, "-c", CHILD.format(paths=paths, name=name, model=model, rect=rect, out=out)],
                         check=True, env=dict(os.environ, **env), timeout=120, capture_output=True, text=True)
    return np.load(out), res.stdout


@pytest.mark.parametrize("batch", ["1", "100", "50"])     # one ray; no divisor of 960 or 192; below w * h = 192
def test_the_batch_size_does_not_show(tmp_path, batch):
    name, model, rect = "scan64_mixed", "fisheye", (0, 0, NX, NY)     # the frame: its corners have no rays
    c, sc, cam = scene(name)
    img, mom, gd = sc.render_lens(cam, case_params(c), lens_of(model), *rect, moments=True, guides=True)
    rays = rtnw.lens_rays(cam, case_params(c), lens_of(model), *rect)
    got, _ = run_child(tmp_path, name, model, rect, RTNW_LENS_BATCH=batch)
    assert same(got["img"], img) and same(got["mom"], mom) and same(got["gd"], gd)
    assert same(got["rays"], rays.view(np.uint8))
    assert (img > 0).any() and (gd[..., 3] > 0).any()


def test_the_device_render_on_a_callers_stream_gives_the_same_bytes():
    import torch
    c, sc, cam = scene("media9_bvh")
    p, lens = case_params(c), lens_of("equirect")
    x0, y0, w, h = TILE
    img, mom, gd = sc.render_lens(cam, p, lens, x0, y0, w, h, moments=True, guides=True)
    stream = torch.cuda.Stream()
    d_img = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda")
    d_mom = torch.full((h, w, 2), 7.0, dtype=torch.float32, device="cuda")
    d_gd = torch.full((h, w, 8), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert d_gd.data_ptr() % 16 == 0
    sc.render_lens_dev(cam, p, lens, x0, y0, w, h, d_img.data_ptr(), d_mom.data_ptr(), d_gd.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert same(d_img.cpu().numpy(), img) and same(d_mom.cpu().numpy(), mom) and same(d_gd.cpu().numpy(), gd)
    d_img.fill_(7.0)
    sc.render_lens_dev(cam, p, lens, x0, y0, w, h, d_img.data_ptr(), 0, 0, stream.cuda_stream)    # the image alone
    stream.synchronize()
    assert same(d_img.cpu().numpy(), img)


def test_two_seeds_give_different_images():
    c, sc, cam = scene("scan64_mixed")
    a = sc.render_lens(cam, case_params(c), lens_of("equirect"), 0, 0, NX, NY)
    b = sc.render_lens(cam, frame_params(max_depth=min(c.max_depth, 8), background=BG[c.background], seed=c.seed + 1),
                       lens_of("equirect"), 0, 0, NX, NY)
    assert (bits(a) != bits(b)).any(-1).mean() > 0.5
    assert same(a, sc.render_lens(cam, case_params(c), lens_of("equirect"), 0, 0, NX, NY))


def test_a_split_sample_range_recombines_by_the_rule():
    c, sc, cam = scene("scan64_mixed")
    lens = lens_of("equirect")
    whole = sc.render_lens(cam, case_params(c, offset=0, spp=5), lens, 0, 0, NX, NY, moments=True, guides=True)
    rgb, hits = [], []
    for offset, spp in ((0, 2), (2, 3)):
        _, rad, h = compose(sc, cam, case_params(c, offset=offset, spp=spp), lens, (0, 0, NX, NY))
        rgb.append(rad["rgb"].reshape(spp, NY, NX, 3))
        hits.append(h)
    both = {k: np.concatenate([h[k] for h in hits]) for k in hits[0]}
    want = lens_reduce(np.concatenate(rgb), both)
    for got, ref in zip(whole, want):
        assert same(got, ref)


# ------------------------------------------------------------------ 6. errors that need the scene
def test_a_shutter_outside_the_scenes_span_is_invalid_and_leaves_the_outputs_alone():
    c, sc, cam = scene("scan64_mixed")       # moving spheres over [0, 1]
    late = rtnw.Camera(c.lookfrom, c.lookat, (0, 1, 0), c.vfov, float(F(NX) / F(NY)), c.aperture, 9.0, 0.5, 1.5)
    p, lens = case_params(c), lens_of("equirect")
    out = [np.full((NY, NX, k), 7.0, F) for k in (3, 2, 8)]
    rc = rtnw.lib().rt_render_lens(sc.handle, ctypes.byref(late.desc), ctypes.byref(lens), ctypes.byref(p), 0, 0, NX, NY,
                                   out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, None)
    msg = rtnw.lib().rt_last_error().decode()
    assert rc == RT_ERR_INVALID and "rt_render_lens:" in msg and "shutter" in msg, (rc, msg)
    assert all((o == 7.0).all() for o in out)
    with pytest.raises(rtnw.RtError) as e:
        sc.render_lens_dev(late, p, lens, 0, 0, NX, NY, 16, 0, 0)     # never dereferenced: the check comes first
    assert e.value.code == RT_ERR_INVALID and "shutter" in str(e.value)
    # a scene without moving spheres does not mind
    c2, sc2, _ = scene("cloud1736")
    late2 = rtnw.Camera(c2.lookfrom, c2.lookat, (0, 1, 0), c2.vfov, float(F(NX) / F(NY)), c2.aperture, 9.0, 0.5, 1.5)
    assert (sc2.render_lens(late2, case_params(c2), lens, 0, 0, NX, NY) > 0).any()


def test_a_wide_bvh_is_unsupported(tmp_path):
    got, out = run_child(tmp_path, "cloud1736", "equirect", TILE, RTNW_BVH_WIDTH="4")
    assert got["code"].tolist() == [RT_ERR_UNSUPPORTED] and "2-wide BVH" in out, (got["code"], out)
