"""Ray queries on the GPU (rt_trace_rays, rt_occluded and their _dev forms)
against the oracle, bit for bit: the oracle's own camera rays of the generated scenes
(tests/gen_scenes.py), rebuilt outside it by test_trace_spec.camera_rays, must come back from
rt_trace_rays with oracle.first_hits_desc's primitive, depth, normal and albedo; bounded,
invalid and axis-parallel rays follow the statements of tests/test_trace_spec.py.  Every
comparison is of bits: there is no tolerance in this file."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import gen_scenes as G
import oracle as O
import rtnw
from test_gpu_parity import THREADS
from test_trace_spec import FLT_MAX, camera_rays, expected_with_tmax, first_hits_spheres, pinhole, sphere_list

pytestmark = pytest.mark.gpu

CASES = ["scan64_mixed", "scan65_mixed", "scan_five_kinds", "prescan8", "prescan9", "cell_near_inst_moving", "media9_bvh",
         "boundaries_bvh", "cloud1736", "quad4095", "progression200", "chains_short", "chains_long", "image_rects",
         "textures_by_kind"]
TIMES = [0.0, 0.37, 1.0]
FIELDS = ("prim", "material", "t", "depth", "normal", "albedo")
RT_ERR_UNSUPPORTED = -4


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


_scenes, _views = {}, {}


def scene_of(name):
    """(case, descriptor, scene), made once."""
    if name not in _scenes:
        c = G.BY_NAME[name]
        desc = c.builder().desc()
        _scenes[name] = (c, desc, rtnw.Scene(desc))
    return _scenes[name]


def view(name, T):
    """The case's pinhole view at time T, made once and left unchanged: the oracle's first hits,
    the rebuilt rays (t_min 0.001, t_max +inf), rt_trace_rays' result for them, and whether each
    hit primitive is a rect."""
    if (name, T) not in _views:
        c, desc, sc = scene_of(name)
        cam = pinhole(c, T)
        fh = O.first_hits_desc(desc, cam, O.desc_spec(c.nx, c.ny, c.spp, max_depth=c.max_depth, background=c.background,
                                                      seed=c.seed, threads=THREADS))
        o, d, time = camera_rays(cam, c.nx, c.ny, c.spp, c.seed)
        # asserted, not tolerated: a zero component would put rects outside the parity contract
        assert (d != 0).all(), "a rebuilt camera ray has a zero direction component: change the seed"
        rays = rtnw.pack_rays(o, d, 0.001, np.inf, time)
        hit = sc.trace_rays(rays)
        kinds = np.array([desc.contents.prims[i].kind for i in range(desc.contents.nprims)] + [-1], np.int32)
        hit["rect"] = kinds[hit["prim"]] >= 2
        _views[(name, T)] = (fh, rays, hit)
    return _views[(name, T)]


def check_occluded(sc, rays, hit):
    """3. rt_occluded is 1 exactly where rt_trace_rays reports a primitive."""
    occ = sc.occluded(rays)
    assert occ.dtype == np.uint8 and np.array_equal(occ, (hit["prim"] >= 0).astype(np.uint8))


# ------------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("T", TIMES)
@pytest.mark.parametrize("name", CASES)
def test_camera_rays_hit_what_the_oracle_hits(name, T):
    c, desc, sc = scene_of(name)
    fh, rays, hit = view(name, T)
    n = len(rays)
    share = float(np.mean(hit["prim"] >= 0))
    print(f"{name} T={T}: {n} rays, hit share {share:.3f}")
    assert 0.05 <= float(np.mean(fh["prim"] >= 0)) <= 0.95
    assert np.array_equal(hit["prim"], fh["prim"].reshape(-1))
    for k in ("depth", "normal", "albedo"):
        assert same(hit[k], fh[k].reshape(hit[k].shape)), k
    mats = np.array([desc.contents.prims[i].material for i in range(desc.contents.nprims)] + [-1], np.int32)
    assert np.array_equal(hit["material"], mats[hit["prim"]])
    d = rays["dir"]
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    assert length.dtype == np.float32 and same(hit["t"] * length, hit["depth"])
    assert not hit["pad"].any()
    check_occluded(sc, rays, hit)


def test_every_kind_and_the_chains_are_hit_and_moving_spheres_move():
    for name in ("scan64_mixed", "chains_short", "chains_long"):
        _, desc, _ = scene_of(name)
        p = desc.contents.prims
        hit = view(name, 0.0)[2]["prim"]
        got = sorted(set(hit[hit >= 0].tolist()))
        if name == "scan64_mixed":
            assert {p[i].kind for i in got} == {0, 1, 2, 3, 4}, name
        assert any(p[i].instance >= 0 for i in got), name
    a, b = view("scan64_mixed", 0.0)[2], view("scan64_mixed", 0.37)[2]
    assert not (same(a["prim"], b["prim"]) and same(a["depth"], b["depth"]))


# ------------------------------------------------------------------ 2. per-ray bounds
def bounds_of(t, k):
    """Six bounds around each t, dealt by ray index: t, the floats next to it, t / 2, 2 t, FLT_MAX."""
    f = np.float32
    table = np.stack([t, np.nextafter(t, f(0)), np.nextafter(t, f(np.inf)), f(0.5) * t, f(2) * t, np.full_like(t, FLT_MAX)])
    return table[k % 6, np.arange(len(t))].astype(f)


@pytest.mark.parametrize("name", CASES)
def test_per_ray_t_max(name):
    c, desc, sc = scene_of(name)
    _, rays, hit = view(name, 0.37)
    n = len(rays)
    k = np.arange(n)
    # the hits' own t; a miss gets a finite bound too
    tmax = bounds_of(np.where(hit["prim"] >= 0, hit["t"], np.float32(1)), k)
    r = rays.copy()
    r["t_max"] = tmax
    got, want = sc.trace_rays(r), expected_with_tmax(hit, tmax)
    for f in FIELDS:
        assert same(got[f], want[f]), f
    at_t = (hit["prim"] >= 0) & (k % 6 == 0)
    print(f"{name}: t_max == t on {int((at_t & hit['rect']).sum())} rects and {int((at_t & ~hit['rect']).sum())} spheres")
    assert (got["prim"][at_t & ~hit["rect"]] == -1).all() and (got["prim"][at_t & hit["rect"]] >= 0).all()
    check_occluded(sc, r, got)


def test_a_sphere_at_t_max_misses_and_a_rect_at_t_max_hits():
    """Both kinds occur with t_max == t: every hit of the batch bounded by its own t."""
    _, rays, hit = view("scan64_mixed", 0.0)
    sc = scene_of("scan64_mixed")[2]
    have = hit["prim"] >= 0
    r = rays.copy()
    r["t_max"] = np.where(have, hit["t"], np.float32(1))
    got = sc.trace_rays(r)
    rect, sph = have & hit["rect"], have & ~hit["rect"]
    assert rect.sum() > 10 and sph.sum() > 10
    assert (got["prim"][sph] == -1).all()
    assert np.array_equal(got["prim"][rect], hit["prim"][rect]) and same(got["t"][rect], hit["t"][rect])
    check_occluded(sc, r, got)


@pytest.mark.parametrize("name", ["cloud1736", "progression200"])
def test_per_ray_t_min_on_spheres(name):
    c, desc, sc = scene_of(name)
    _, rays, hit = view(name, 0.0)
    k = np.arange(len(rays))
    tmin = bounds_of(np.where(hit["prim"] >= 0, hit["t"], np.float32(1)), k)
    tmin[k % 6 == 5] = np.float32(-1.0)   # in place of FLT_MAX: a negative t_min, which admits what lies behind the origin
    r = rays.copy()
    r["t_min"] = tmin
    got = sc.trace_rays(r)
    prim, t = first_hits_spheres(r["origin"], r["dir"], sphere_list(desc), tmin, np.inf)
    print(f"{name}: {int((prim != hit['prim']).sum())} of {len(k)} results moved with t_min; hit share {np.mean(prim >= 0):.3f}")
    assert (prim != hit["prim"]).any() and (prim >= 0).any()
    assert np.array_equal(got["prim"], prim) and same(got["t"], t)
    check_occluded(sc, r, got)


# ------------------------------------------------------------------ 4. invalid rays
def test_invalid_rays_report_invalid_and_leave_the_others_alone():
    name = "scan64_mixed"   # moving spheres: the time span counts
    sc = scene_of(name)[2]
    _, rays, hit = view(name, 0.37)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    bad = []
    for field in ("origin", "dir"):
        for value in (nan, inf, -inf):
            for comp in range(3):
                bad.append((field, comp, value))
    for field in ("time", "t_min"):
        for value in (nan, inf, -inf):
            bad.append((field, None, value))
    bad += [("t_max", None, nan), ("dir", "all", np.float32(0)), ("time", None, np.float32(-0.5)),
            ("time", None, np.float32(1.5))]
    r = rays[:4 * len(bad)].copy()
    where = np.arange(len(bad)) * 4 + 1   # interleaved with valid rays
    for at, (field, comp, value) in zip(where, bad):
        if comp is None:
            r[field][at] = value
        elif comp == "all":
            r[field][at] = value
        else:
            r[field][at, comp] = value
    got, occ = sc.trace_rays(r), sc.occluded(r)
    invalid = np.zeros(len(r), bool)
    invalid[where] = True
    assert (got["prim"][invalid] == rtnw.RT_HIT_INVALID).all() and (occ[invalid] == 255).all()
    assert (got["material"][invalid] == -1).all() and not got["t"][invalid].any() and not got["depth"][invalid].any()
    assert not got["normal"][invalid].any() and (got["albedo"][invalid] == 1).all() and not got["pad"].any()
    alone = sc.trace_rays(r[~invalid])
    for f in FIELDS:
        assert same(got[f][~invalid], alone[f]) and same(got[f][~invalid], hit[f][:len(r)][~invalid]), f
    assert np.array_equal(occ[~invalid], (alone["prim"] >= 0).astype(np.uint8))
    # t_max = -inf and +inf are bounds, not errors; without moving spheres the time is ignored
    r2 = rays[:8].copy()
    r2["t_max"][::2] = -inf
    assert (sc.trace_rays(r2)["prim"][::2] == -1).all()
    sc3 = scene_of("cloud1736")[2]
    r3 = view("cloud1736", 0.0)[1][:64].copy()
    base = sc3.trace_rays(r3)
    r3["time"] = np.float32(7.0)
    moved = sc3.trace_rays(r3)
    for f in FIELDS:
        assert same(base[f], moved[f]), f


# ------------------------------------------------------------------ 5. axis-parallel rays on spheres
def test_axis_parallel_rays_on_spheres():
    c, desc, sc = scene_of("cloud1736")   # spheres only, the BVH in HBM
    sph = sphere_list(desc)
    f = np.float32
    axes = np.concatenate([np.eye(3, dtype=f), -np.eye(3, dtype=f)])
    rng = np.random.default_rng(11)
    centres = sph[rng.choice(len(sph), 24, replace=False), :3]
    origins, dirs = [], []
    for a in axes:
        for cen in centres:
            jitter = rng.uniform(-0.05, 0.05, 3).astype(f) * (a == 0)   # through the sphere, off its centre
            origins += [cen - f(9) * a + jitter, cen - f(0.6) * a + jitter]   # outside the cloud; inside it
            dirs += [a, a * f(3)]
        for o in ((0, 1, 0), (0, 0, 0), (1.5, 0, -2), (-3, 2.25, 0.5)):   # zero origin components too
            origins.append(np.array(o, f))
            dirs.append(a)
    rays = rtnw.pack_rays(np.array(origins, f), np.array(dirs, f), 0.001, np.inf, 0.0)
    assert ((rays["dir"] == 0).sum(axis=1) == 2).all()
    prim, t = first_hits_spheres(rays["origin"], rays["dir"], sph, 0.001, np.inf)
    share = float(np.mean(prim >= 0))
    print(f"axis-parallel: {len(rays)} rays, hit share {share:.3f}")
    assert 0.25 < share < 1.0 and (prim == -1).any()
    got = sc.trace_rays(rays)
    assert np.array_equal(got["prim"], prim) and same(got["t"], t)
    check_occluded(sc, rays, got)


# ------------------------------------------------------------------ 6. shapes and plumbing
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_any_number_of_rays(n):
    sc = scene_of("scan65_mixed")[2]
    _, rays, hit = view("scan65_mixed", 0.37)
    assert n <= len(rays)
    got = sc.trace_rays(rays[:n])
    for f in FIELDS + ("pad",):
        assert same(got[f], hit[f][:n]), f
    check_occluded(sc, rays[:n], got)


CHILD = """
import sys
sys.path[:0] = {paths!r}
import numpy as np
import gen_scenes as G, rtnw
from test_trace_spec import camera_rays, pinhole
c = G.BY_NAME[{name!r}]
sc = rtnw.Scene(c.builder().desc())
o, d, time = camera_rays(pinhole(c, 0.37), c.nx, c.ny, c.spp, c.seed)
rays = rtnw.pack_rays(o, d, 0.001, np.inf, time)
hit = sc.trace_rays(rays)
np.savez({out!r}, occluded=sc.occluded(rays), **hit)
"""


def test_small_batches_change_nothing(tmp_path):
    """RTNW_TRACE_BATCH=64 in a fresh process (24 full batches), then 100: the last batch short."""
    name = "scan65_mixed"
    _, rays, hit = view(name, 0.37)
    assert len(rays) > 64 and len(rays) % 64 == 0
    sc = scene_of(name)[2]
    out = str(tmp_path / "small.npz")
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here, os.path.dirname(rtnw.__file__), os.path.dirname(O.__file__)]
    env = dict(os.environ, RTNW_TRACE_BATCH="64")
    subprocess.run([sys.executable, "-c", CHILD.format(paths=paths, name=name, out=out)], check=True, env=env, timeout=120)
    small = np.load(out)
    for f in FIELDS + ("pad",):
        assert same(small[f], hit[f]), f
    assert np.array_equal(small["occluded"], sc.occluded(rays))
    # a batch size that does not divide the count, in this process (the knob is read per call)
    os.environ["RTNW_TRACE_BATCH"] = "100"
    try:
        odd = sc.trace_rays(rays)
        occ = sc.occluded(rays)
    finally:
        del os.environ["RTNW_TRACE_BATCH"]
    for f in FIELDS + ("pad",):
        assert same(odd[f], hit[f]), f
    assert np.array_equal(occ, small["occluded"])


def test_device_forms_equal_the_host_forms():
    L = rtnw.lib()
    sc = scene_of("prescan9")[2]
    _, rays, hit = view("prescan9", 0.37)
    n = len(rays)
    occ = sc.occluded(rays)
    dev = ctypes.c_void_p()
    rtnw._check(L.rt_device_alloc(0, n * (48 + 48 + 1), ctypes.byref(dev)))
    try:
        d_rays, d_hits, d_occ = dev.value, dev.value + 48 * n, dev.value + 96 * n
        rtnw._check(L.rt_copy_to_device(ctypes.c_void_p(d_rays), rays.ctypes.data, rays.nbytes))
        sc.trace_rays_dev(d_rays, n, d_hits)
        sc.occluded_dev(d_rays, n, d_occ)
        hits = np.zeros(n, rtnw.HIT_DTYPE)
        occ_dev = np.zeros(n, np.uint8)
        rtnw._check(L.rt_copy_to_host(hits.ctypes.data, ctypes.c_void_p(d_hits), hits.nbytes))
        rtnw._check(L.rt_copy_to_host(occ_dev.ctypes.data, ctypes.c_void_p(d_occ), n))
    finally:
        L.rt_device_free(dev)
    for f in FIELDS + ("pad",):
        assert same(hits[f], hit[f]), f
    assert np.array_equal(occ_dev, occ)


def test_an_empty_scene_reports_misses():
    sc = rtnw.Scene.builtin("edge_empty")
    rays = view("scan65_mixed", 0.37)[1][:130]
    got = sc.trace_rays(rays)
    assert (got["prim"] == -1).all() and (got["material"] == -1).all() and not got["t"].any() and not got["depth"].any()
    assert not got["normal"].any() and (got["albedo"] == 1).all() and not got["pad"].any()
    assert not sc.occluded(rays).any()
    sc.close()


def test_a_wide_bvh_is_unsupported(monkeypatch):
    monkeypatch.setenv("RTNW_BVH_WIDTH", "4")
    sc = rtnw.Scene(scene_of("cloud1736")[1])
    monkeypatch.delenv("RTNW_BVH_WIDTH")
    rays = view("cloud1736", 0.0)[1][:8]
    for call in (sc.trace_rays, sc.occluded):
        with pytest.raises(rtnw.RtError) as e:
            call(rays)
        assert e.value.code == RT_ERR_UNSUPPORTED and "2-wide BVH" in str(e.value)
    sc.close()
