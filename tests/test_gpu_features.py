"""The first-hit feature pass on the GPU (rt_render_features, rt_render_features_dev).

Three ties: the means are the float32 sums of the one-sample results (bitwise); coverage and a
light's albedo equal what the megakernel renders for the same samples with max_depth = 0
(bitwise: the two kernels build the same camera rays and find the same first hits); normals,
depths and albedos follow the float64 restatement of tests/test_features_spec.py within 8 x
the float32 restatement's own deviation from it.
"""
import ctypes

import numpy as np
import pytest

import rtnw
import test_features_spec as S
from test_gpu_parity import _scene

pytestmark = pytest.mark.gpu

SEED = 23
KEYS = ("albedo", "normal", "depth", "coverage")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def setup(scene, nx, ny, spp, **kw):
    cam_name, bg, depth = rtnw.SCENE_DEFAULTS[scene]
    p = rtnw.RenderParams(nx, ny, spp, max_depth=depth, background=bg, seed=SEED, chunk=1, **kw)
    return _scene(scene), rtnw.Camera.preset(cam_name, nx, ny), p


_single = {}


def single(scene, nx, ny, k):
    """Sample k's features of the full frame (spp = 1, sample_offset = k); computed once."""
    key = (scene, nx, ny, k)
    if key not in _single:
        sc, cam, p = setup(scene, nx, ny, 1, sample_offset=k)
        f = sc.render_features(cam, p, 0, 0, nx, ny)
        for v in f.values():
            v.setflags(write=False)
        _single[key] = f
    return _single[key]


def mean_f32(parts):
    """Sample-order float32 sum times float(1.0 / n), as rt_resolve normalises."""
    acc = np.zeros(parts[0].shape, np.float32)
    for v in parts:
        acc = acc + v
    return acc * np.float32(1.0 / np.float64(np.float32(len(parts))))


@pytest.mark.parametrize("scene", ["random_motion", "cornell_box", "final", "earth"])
def test_means_are_the_float32_sums(scene):
    nx, ny, n = 17, 9, 5
    sc, cam, p = setup(scene, nx, ny, n)
    full = sc.render_features(cam, p, 0, 0, nx, ny)
    for key in KEYS:
        want = mean_f32([single(scene, nx, ny, k)[key] for k in range(n)])
        assert same(full[key], want), (scene, key, float(np.abs(full[key] - want).max()))
    cov = full["coverage"]
    assert ((cov >= 0) & (cov <= 1)).all() and cov.max() > 0
    assert np.isfinite(full["albedo"]).all() and np.isfinite(full["normal"]).all() and np.isfinite(full["depth"]).all()
    # a sub-rectangle is the crop of the full frame
    x0, y0, w, h = 3, 2, 11, 5
    part = sc.render_features(cam, p, x0, y0, w, h)
    for key in KEYS:
        assert same(part[key], np.ascontiguousarray(full[key][y0:y0 + h, x0:x0 + w])), (scene, key)
    # the device entry point writes the same values, packed (albedo, coverage, normal, depth)
    L = rtnw.lib()
    dev = ctypes.c_void_p()
    packed = np.zeros((ny, nx, 8), np.float32)
    rtnw._check(L.rt_device_alloc(0, packed.nbytes, ctypes.byref(dev)))
    try:
        sc.render_features_dev(cam, p, 0, 0, nx, ny, dev.value)
        rtnw._check(L.rt_copy_to_host(packed.ctypes.data, dev, packed.nbytes))
    finally:
        L.rt_device_free(dev)
    assert same(packed[..., 0:3], full["albedo"]) and same(packed[..., 3], full["coverage"])
    assert same(packed[..., 4:7], full["normal"]) and same(packed[..., 7], full["depth"])


def test_any_output_may_be_null():
    nx, ny = 17, 9
    sc, cam, p = setup("cornell_box", nx, ny, 1)
    depth = np.zeros((ny, nx), np.float32)
    rtnw._check(rtnw.lib().rt_render_features(sc.handle, ctypes.byref(cam.desc), ctypes.byref(p), 0, 0, nx, ny, None, None,
                                              depth.ctypes.data, None))
    assert same(depth, single("cornell_box", nx, ny, 0)["depth"])


@pytest.mark.parametrize("scene", ["random_motion", "random_scene", "edge_single", "edge_degenerate", "edge_empty"])
def test_coverage_is_the_megakernels_first_hit(scene):
    """max_depth = 0 under the sky: a first hit on a non-emitter renders exactly 0, and the sky
    is never 0.  random_motion's view has a lens and an open shutter: jitter, lens and time
    draws all enter the tie.  edge_degenerate also holds a light (its xy_rect): a first hit on
    it renders what it emits, which is the feature albedo bit for bit, and never the sky's
    colour (the sky equals a miss's albedo (1, 1, 1) only straight down)."""
    nx, ny = 33, 17
    cam_name, _, _ = rtnw.SCENE_DEFAULTS[scene]
    sc, cam = _scene(scene), rtnw.Camera.preset(cam_name, nx, ny)
    hits = 0
    for k in range(8):
        p = rtnw.RenderParams(nx, ny, 1, max_depth=0, background=rtnw.RT_BG_SKY, seed=SEED, chunk=1, sample_offset=k)
        img = sc.render_tile(cam, p, 0, 0, nx, ny)
        f = sc.render_features(cam, p, 0, 0, nx, ny)
        cov = f["coverage"]
        assert set(np.unique(cov)) <= {0.0, 1.0}
        hit = (img == 0).all(-1)
        if scene == "edge_degenerate":
            lit = (bits(img) == bits(f["albedo"])).all(-1)
            assert (img[lit] == 2.0).all()     # the rect's (2, 2, 2)
            hit |= lit
        assert np.array_equal(cov == 1.0, hit), (scene, k, int(((cov == 1.0) != hit).sum()))
        hits += int(cov.sum())
    assert (hits == 0) == (scene == "edge_empty")


@pytest.mark.parametrize("scene", ["cornell_box", "simple_light"])
def test_a_lights_albedo_is_what_it_emits(scene):
    nx, ny = 33, 17
    cam_name, _, _ = rtnw.SCENE_DEFAULTS[scene]
    sc, cam = _scene(scene), rtnw.Camera.preset(cam_name, nx, ny)
    lit = 0
    for k in range(8):
        p = rtnw.RenderParams(nx, ny, 1, max_depth=0, background=rtnw.RT_BG_BLACK, seed=SEED, chunk=1, sample_offset=k)
        img = sc.render_tile(cam, p, 0, 0, nx, ny)
        f = sc.render_features(cam, p, 0, 0, nx, ny)
        on = (img != 0).any(-1)
        assert same(f["albedo"][on], img[on]) and (f["coverage"][on] == 1.0).all()
        lit += int(on.sum())
    assert lit > 0


@pytest.fixture(scope="module")
def draws():
    d = S.jitter_draws(S.NX, S.NY, S.OFFSETS, S.SEED)
    d.setflags(write=False)
    return d


@pytest.mark.parametrize("scene", ["edge_single", "random_scene"])
def test_first_hits_follow_the_float64_restatement(scene, draws):
    nx, ny = S.NX, S.NY
    sc, cam, desc = _scene(scene), S.pinhole_camera(scene, nx, ny), rtnw.SceneDesc.builtin(scene)
    r64, _, keep = S.compared(desc, cam, nx, ny, draws)
    assert 1.0 - keep.mean() <= S.MAX_UNDECIDED
    _, _, mat = S.spheres_of(desc)
    got = []
    for k in range(S.OFFSETS):
        p = rtnw.RenderParams(nx, ny, 1, t_min=0.001, seed=S.SEED, sample_offset=k)
        got.append(sc.render_features(cam, p, 0, 0, nx, ny))
    g = {key: np.stack([f[key] for f in got]) for key in KEYS}
    assert np.array_equal(g["coverage"][keep] == 1.0, r64["hit"][keep])
    h = keep & r64["hit"]
    dn = np.abs(g["normal"][h] - r64["normal"][h]).max()
    dz = np.abs(g["depth"][h] / r64["depth"][h] - 1).max()
    print(f"{scene}: {int(h.sum())} hits compared, normal deviation {dn:.3g} (bar {S.TOL_NORMAL:.3g}), "
          f"depth {dz:.3g} (bar {S.TOL_DEPTH:.3g})")
    assert dn <= S.TOL_NORMAL and dz <= S.TOL_DEPTH
    miss = keep & ~r64["hit"]
    assert (g["normal"][miss] == 0).all() and (g["depth"][miss] == 0).all() and (g["albedo"][miss] == 1).all()
    # the hit material's colour, bitwise: its one colour, or one of the checker's two
    for m in np.unique(mat[r64["prim"][h]]):
        sel = h & (mat[r64["prim"]] == m)
        cols = S.material_colours(desc, m)
        ok = np.zeros(int(sel.sum()), bool)
        for c in cols:
            ok |= (bits(g["albedo"][sel]) == bits(c)).all(-1)
        assert ok.all(), (scene, int(m))
        if len(cols) == 2 and sel.sum() > 50:
            assert all(((bits(g["albedo"][sel]) == bits(c)).all(-1)).any() for c in cols)   # both squares show
