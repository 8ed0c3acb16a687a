"""The first-hit feature pass, the CPU side: the new entry points, the argument checks of
rt_render_features / rt_render_features_dev (made before any HIP call, so they answer without
a GPU), and a numpy restatement of the first hit for scenes of spheres.

The restatement (`first_hits`) is what tests/test_gpu_features.py compares normals, depths and
albedos with.  It is written once for a dtype: the float64 run is the reference, the float32
run measures how far float32 arithmetic of the same formulas strays from it, which sets the
tolerance (TOL_* below).  Its camera has aperture 0 and a closed shutter at 0, so a sample's
ray is a function of its two jitter draws (oracle.counter_draws).
"""
import ctypes

import numpy as np
import pytest

import oracle as O
import rtnw

RT_ERR_INVALID = -1
RT_PRIM_SPHERE, RT_TEX_CONSTANT, RT_TEX_CHECKER = 0, 0, 1
RT_MAT_LAMBERTIAN, RT_MAT_METAL, RT_MAT_DIELECTRIC = 0, 1, 2

# The restated case: 32 x 16 pixels, spp = 1 at sample offsets 0..3, seed 23, the views below
NX, NY, OFFSETS, SEED = 32, 16, 4, 23
# Largest deviation of the float32 restatement from the float64 one over the compared samples of
# both scenes (test_restatement_tolerances recomputes them), and the bars, 8 x that:
#   normal, absolute per component: 5.34e-5 (edge_single, near the rim)             -> 4.3e-4
#   depth, relative:                4.99e-5 (random_scene: the ground's large sphere) -> 4.0e-4
DEV_NORMAL, DEV_DEPTH = 5.4e-5, 5.0e-5
TOL_NORMAL, TOL_DEPTH = 8 * DEV_NORMAL, 8 * DEV_DEPTH
MAX_UNDECIDED = 0.02


# Views of the restated scenes.  The grazing rule (discriminant below 1e-3 of b^2) leaves out
# every hit on a sphere whose squared radius is below 1e-3 of its squared distance: from the
# "random" preset's 13 units that is each of random_scene's small spheres, a tenth of the
# image.  random_scene is therefore looked at from close above the ground, where the rule
# leaves out under 1 % and the view still holds the ground's checker, a large sphere and
# several small ones; edge_single keeps the preset's view (its sky exercises the misses).
VIEWS = {
    "edge_single": dict(lookfrom=rtnw.CAMERA_PRESETS["random"]["lookfrom"], lookat=(0, 0, 0), vfov=20.0),
    "random_scene": dict(lookfrom=(-2, 1.6, 1.0), lookat=(-2, 0, 0.3), vfov=90.0),
}


def pinhole_camera(scene, nx, ny):
    """The scene's view with aperture 0 and the shutter closed at 0."""
    v = VIEWS[scene]
    aspect = float(np.float32(nx) / np.float32(ny))
    return rtnw.Camera(v["lookfrom"], v["lookat"], (0, 1, 0), v["vfov"], aspect, 0.0, 10.0, 0.0, 0.0)


def spheres_of(desc):
    """(centres [S, 3], radii [S], material index [S]) of a scene of spheres only."""
    c = desc.contents
    assert all(c.prims[i].kind == RT_PRIM_SPHERE and c.prims[i].instance < 0 for i in range(c.nprims))
    ctr = np.array([[c.prims[i].p[k] for k in range(3)] for i in range(c.nprims)], np.float64).reshape(-1, 3)
    rad = np.array([c.prims[i].p[3] for i in range(c.nprims)], np.float64)
    mat = np.array([c.prims[i].material for i in range(c.nprims)], np.int64)
    return ctr, rad, mat


def material_colours(desc, mat):
    """The colours a material can show: one for a constant texture, a metal or a dielectric,
    the two leaves for a checker of constants.  float32, as the descriptor holds them."""
    c = desc.contents
    m = c.materials[int(mat)]
    if m.kind == RT_MAT_METAL:
        return [np.array(list(m.albedo), np.float32)]
    if m.kind == RT_MAT_DIELECTRIC:
        return [np.ones(3, np.float32)]
    t = c.textures[m.texture]
    leaves = [t] if t.kind == RT_TEX_CONSTANT else [c.textures[t.even], c.textures[t.odd]]
    assert all(x.kind == RT_TEX_CONSTANT for x in leaves)
    return [np.array(list(x.color), np.float32) for x in leaves]


def jitter_draws(nx, ny, offsets, seed):
    """[offsets, ny, nx, 2]: the two jitter draws of every sample; image row y is j = ny-1-y."""
    u = np.zeros((offsets, ny, nx, 2), np.float64)
    for k in range(offsets):
        for y in range(ny):
            j = ny - 1 - y
            for x in range(nx):
                u[k, y, x] = O.counter_draws(seed, j * nx + x, k, 2)
    return u


def first_hits(desc, cam, nx, ny, draws, t_min, T):
    """First surface hit of every sample in arithmetic of dtype T (sphere.h:25-52 over the
    list): dict of hit [..] bool, prim [..], t, depth, normal [.., 3], undecided [..] bool."""
    ctr, rad, _ = spheres_of(desc)
    ctr, rad = ctr.astype(T), rad.astype(T)
    d = cam.desc
    org, llc, hor, ver = (np.array(list(v), T) for v in (d.origin, d.lower_left_corner, d.horizontal, d.vertical))
    K, H, W, _ = draws.shape
    X = np.arange(W, dtype=np.float64)[None, None, :]
    J = (ny - 1 - np.arange(H, dtype=np.float64))[None, :, None]
    cu = ((X + draws[..., 0]).astype(np.float32).astype(T) / T(nx))[..., None]
    cv = ((J + draws[..., 1]).astype(np.float32).astype(T) / T(ny))[..., None]
    dirs = ((llc + cu * hor) + cv * ver) - org                       # [K, H, W, 3]
    oc = org - ctr                                                   # [S, 3]
    a = (dirs * dirs).sum(-1)[..., None]                             # [K, H, W, 1]
    b = (dirs[..., None, 0] * oc[:, 0] + dirs[..., None, 1] * oc[:, 1]) + dirs[..., None, 2] * oc[:, 2]   # [K, H, W, S]
    cc = (oc * oc).sum(-1) - rad * rad                               # [S]
    disc = b * b - a * cc
    with np.errstate(all="ignore"):
        sq = np.sqrt(np.where(disc > 0, disc, 0))
        t1, t2 = (-b - sq) / a, (-b + sq) / a
    ok1 = (disc > 0) & (t1 > T(t_min))
    ok2 = (disc > 0) & ~ok1 & (t2 > T(t_min))
    t = np.where(ok1, t1, np.where(ok2, t2, np.inf))
    prim = t.argmin(-1)
    best = np.take_along_axis(t, prim[..., None], -1)[..., 0]
    hit = np.isfinite(best)
    # what the restatement cannot decide: a grazing hit (the winner's discriminant below 1e-3
    # of its b^2: t and the normal are ill-conditioned there), or a second candidate within
    # 1e-4 relative of the first.  (A sphere missed by a hair could flip to a hit only within
    # float32's rounding of the discriminant, ~1e-6 of b^2; `compared` drops the samples on
    # which the two precisions disagree.)
    with np.errstate(all="ignore"):
        dw = np.take_along_axis(disc, prim[..., None], -1)[..., 0]
        bw = np.take_along_axis(b, prim[..., None], -1)[..., 0]
        grazing = hit & (dw < 1e-3 * bw * bw)
        second = np.sort(t, -1)[..., 1] if t.shape[-1] > 1 else np.full(best.shape, np.inf)
        close = hit & (second <= best * (1 + 1e-4))
    p = org + best[..., None] * dirs
    with np.errstate(all="ignore"):
        normal = np.where(hit[..., None], (p - ctr[prim]) / rad[prim][..., None], 0)
        depth = np.where(hit, best * np.sqrt(a[..., 0]), 0)
    return dict(hit=hit, prim=prim, t=best, depth=depth, normal=normal, undecided=grazing | close)


def compared(desc, cam, nx, ny, draws, t_min=0.001):
    """The float64 restatement, the float32 one, and the samples both decide alike."""
    r64 = first_hits(desc, cam, nx, ny, draws, t_min, np.float64)
    r32 = first_hits(desc, cam, nx, ny, draws, t_min, np.float32)
    keep = ~r64["undecided"] & ~r32["undecided"] & (r64["hit"] == r32["hit"]) & (r64["prim"] == r32["prim"])
    return r64, r32, keep


@pytest.fixture(scope="module")
def draws():
    return jitter_draws(NX, NY, OFFSETS, SEED)


def test_restatement_tolerances(draws):
    """The chosen seed leaves at most 2 % of the samples undecided, and the recorded float32
    deviations (the tolerance's source) are what the restatement gives."""
    dev_n = dev_z = 0.0
    for scene in ("edge_single", "random_scene"):
        desc = rtnw.SceneDesc.builtin(scene)
        cam = pinhole_camera(scene, NX, NY)
        r64, r32, keep = compared(desc, cam, NX, NY, draws)
        assert 1.0 - keep.mean() <= MAX_UNDECIDED, (scene, 1.0 - keep.mean())
        h = keep & r64["hit"]
        assert h.sum() > 100, scene
        dev_n = max(dev_n, float(np.abs(r32["normal"][h] - r64["normal"][h]).max()))
        dev_z = max(dev_z, float(np.abs(r32["depth"][h] / r64["depth"][h] - 1).max()))
        print(f"{scene}: undecided {1.0 - keep.mean():.4f}, hits {int(h.sum())}, float32 deviation so far "
              f"normal {dev_n:.3g}, depth {dev_z:.3g}")
    assert dev_n <= DEV_NORMAL and dev_n >= DEV_NORMAL / 1.5, dev_n
    assert dev_z <= DEV_DEPTH and dev_z >= DEV_DEPTH / 1.5, dev_z


def test_library_exports_the_feature_entry_points():
    L = rtnw.lib()
    for name in ("rt_render_features", "rt_render_features_dev", "rt_launch_features", "rt_launch_features_resolve"):
        assert hasattr(L, name), name
    assert {"rt_render_features", "rt_render_features_dev"} <= set(rtnw.header_symbols())
    assert hasattr(rtnw.Scene, "render_features") and hasattr(rtnw.Scene, "render_features_dev")


# ------------------------------------------------------------------ argument checks, no GPU
def _features(params, *, cam=True, p=True, outs=(1, 1, 1, 1), rect=(0, 0, 4, 3), dev=False):
    """With a null scene: every argument check comes before any HIP call, the scene's last."""
    L = rtnw.lib()
    camd = rtnw.RtCameraDesc()
    bufs = [np.zeros((3, 4, c), np.float32) for c in (3, 3, 1, 1)]
    ptrs = [b.ctypes.data if use else None for b, use in zip(bufs, outs)]
    cp, pp = (ctypes.byref(camd) if cam else None), (ctypes.byref(params) if p else None)
    if dev:
        rc = L.rt_render_features_dev(None, cp, pp, *rect, next((q for q in ptrs if q), None), None)
    else:
        rc = L.rt_render_features(None, cp, pp, *rect, *ptrs)
    return rc, L.rt_last_error().decode()


def _good(**kw):
    return rtnw.RenderParams(4, 3, 5, seed=1, **kw)


@pytest.mark.parametrize("dev", [False, True])
def test_valid_arguments_reach_the_scene_check(dev):
    for params, kw in ((_good(), {}), (_good(flags=rtnw.RT_FLAG_RIGHT_FOLD, max_depth=0, chunk=7), {}),
                       (_good(sample_offset=9), dict(rect=(1, 1, 3, 2))), (_good(), dict(outs=(0, 0, 1, 0)))):
        rc, msg = _features(params, dev=dev, **kw)
        assert rc == RT_ERR_INVALID and "null scene" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("null", ["cam", "p"])
def test_null_arguments_are_invalid(null, dev):
    rc, msg = _features(_good(), dev=dev, **{null: False})
    assert rc == RT_ERR_INVALID and "null argument" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
def test_all_outputs_null_is_invalid(dev):
    rc, msg = _features(_good(), outs=(0, 0, 0, 0), dev=dev)
    assert rc == RT_ERR_INVALID and "null output" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("field,value,word", [("nx", 0, "nx"), ("ny", 0, "ny"), ("nx", -4, "nx"), ("ny", -1, "ny"),
                                              ("spp", 0, "spp"), ("spp", -2, "spp")])
def test_bad_sizes_are_invalid(field, value, word, dev):
    p = _good()
    setattr(p, field, value)
    rc, msg = _features(p, dev=dev)
    assert rc == RT_ERR_INVALID and word in msg and "null scene" not in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("rect", [(0, 0, 5, 3), (0, 0, 4, 4), (-1, 0, 2, 2), (2, 2, 3, 1), (0, 0, 0, 3), (0, 0, 4, -1)])
def test_rectangles_outside_the_image_are_invalid(rect, dev):
    rc, msg = _features(_good(), rect=rect, dev=dev)
    assert rc == RT_ERR_INVALID and "rectangle" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("flag", ["RT_FLAG_COUNT", "RT_FLAG_PROFILE", "RT_FLAG_SUM_IN", "RT_FLAG_SUM_OUT"])
def test_unsupported_flags_are_invalid(flag, dev):
    rc, msg = _features(_good(flags=getattr(rtnw, flag) | rtnw.RT_FLAG_RIGHT_FOLD), dev=dev)
    assert rc == RT_ERR_INVALID and flag in msg and "null scene" not in msg, msg
