"""RT_FLAG_RIGHT_FOLD on the GPU: the megakernel's right-fold variants (rt_megakernel.h kFold).

With the flag a sample's radiance is main.cpp:36's `emitted + attenuation*color(...)`
evaluated from the deepest hit outwards, the reference's own operation order, so the GPU
image is compared for EQUALITY with what the reference binary wrote
(tests/golden/ref_*.npy) — unconditionally: the goldens are files, and the device runs
its own restatement of glibc (csrc/hip/rt_libm.h).  Against the live oracle
(`media_after=True, forward=False`, the spec the variants implement; the oracle calls the
host's libm) the policy is test_gpu_parity.py's assert_exact.  tests/test_right_fold_spec.py
keeps on record that the default kernel order differs from six of the ten goldens, so the
first test here fails without the feature.
"""
import os

import numpy as np
import pytest

import oracle as O
import rtnw
from conftest import GOLDEN
from test_gpu_parity import EDGE_PARAMS, THREADS, TOL_RMS, _scene, assert_exact, gamma_rms, pixel_exact

pytestmark = pytest.mark.gpu

FOLD = rtnw.RT_FLAG_RIGHT_FOLD
RT_ERR_INVALID, RT_ERR_UNSUPPORTED = -1, -4   # include/rt_hip.h rt_status


def bits(a):
    return a.view(np.uint32)


def fold_render(scene, nx, ny, ns, *, seed=0, chunk=0, rect=None, flags=0, stats=False, sc=None, **kw):
    cam_name, bg, depth = rtnw.SCENE_DEFAULTS[scene]
    kw.setdefault("max_depth", depth)
    kw.setdefault("background", bg)
    p = rtnw.RenderParams(nx, ny, ns, chunk=chunk, seed=seed, flags=FOLD | flags, **kw)
    x0, y0, w, h = rect if rect else (0, 0, nx, ny)
    return (sc or _scene(scene)).render_tile(rtnw.Camera.preset(cam_name, nx, ny), p, x0, y0, w, h, stats=stats)


def fold_spec(scene, nx, ny, ns, *, seed=0, chunk=0, **kw):
    """What the fold variants compute: right fold, media after the surface pass."""
    return O.RenderSpec(scene=scene, nx=nx, ny=ny, ns=ns, rng="counter", seed=seed, media_after=True, forward=False,
                        chunk=chunk, threads=THREADS, **kw)


def check_against_oracle(what, g, o):
    pinned, why = O.host_libm_pinned()
    print(f"host_libm_pinned: {pinned} ({why})")
    assert g.shape == o.shape
    rms = gamma_rms(g, o)
    exact = pixel_exact(g, o)
    print(f"{what}: gamma RMS {rms}, bit-exact pixels {exact:.4f}")
    assert (rms <= TOL_RMS).all(), rms
    assert_exact(exact)


# ---- 1. the reference executable's framebuffers, bit for bit ---------------------------
@pytest.mark.parametrize("name", ["c1_random", "c2_cornell", "c3_motion", "c4_final", "smoke", "simple_light",
                                  "earth", "edge_empty", "edge_single", "edge_degenerate", "edge_chains"])
def test_right_fold_equals_the_reference_framebuffer_bitwise(golden, name):
    c = golden["counter_fb"][name]
    ref = np.load(os.path.join(GOLDEN, f"ref_{name}.npy"))
    g = fold_render(c["scene"], c["nx"], c["ny"], c["ns"], seed=c["seed"], chunk=0)
    assert g.shape == ref.shape
    differing = int(np.sum(np.any(bits(g) != bits(ref), axis=-1)))
    print(f"{name}: {differing} of {ref.shape[0] * ref.shape[1]} pixels differ from the reference framebuffer")
    assert np.array_equal(bits(g), bits(ref))


# ---- 2. the live oracle ---------------------------------------------------------------
@pytest.mark.parametrize("scene,nx,ny,ns,chunk,seed", [("cornell_smoke", 24, 24, 8, 8, 5), ("test", 32, 16, 8, 3, 7),
                                                       ("two_spheres", 24, 24, 4, 4, 8)])
def test_right_fold_matches_oracle_on_scenes_without_a_golden(scene, nx, ny, ns, chunk, seed):
    g = fold_render(scene, nx, ny, ns, seed=seed, chunk=chunk)
    o = O.render(fold_spec(scene, nx, ny, ns, seed=seed, chunk=chunk))[0]
    check_against_oracle(scene, g, o)


@pytest.mark.parametrize("scene,nx,ny,ns,chunk,depth,bg,tmin", EDGE_PARAMS)
def test_right_fold_matches_oracle_at_parameter_edges(scene, nx, ny, ns, chunk, depth, bg, tmin):
    bg0 = rtnw.SCENE_DEFAULTS[scene][1]
    bgv = bg0 if bg is None else (rtnw.RT_BG_SKY if bg == "sky" else rtnw.RT_BG_BLACK)
    g = fold_render(scene, nx, ny, ns, seed=21, chunk=chunk, max_depth=depth, background=bgv, t_min=tmin)
    o = O.render(fold_spec(scene, nx, ny, ns, seed=21, chunk=chunk, max_depth=depth, tmin=tmin,
                           background=None if bg is None else bg))[0]
    assert g.shape == (ny, nx, 3)
    assert np.isfinite(g).all() and (g >= 0).all()
    check_against_oracle(f"{scene} depth {depth} t_min {tmin}", g, o)


def test_right_fold_chunked_partial_sums_match_oracle():
    g = fold_render("final", 16, 16, 8, seed=6, chunk=3)
    o = O.render(fold_spec("final", 16, 16, 8, seed=6, chunk=3))[0]
    check_against_oracle("final chunk 3", g, o)


# ---- 3. full-spp crops against the oracle's reference order (list order, right fold) ----
@pytest.mark.parametrize("scene,nx,ny,ns,rects", [("final", 500, 500, 1000, [(246, 246, 8, 8), (131, 402, 8, 8)]),
                                                  ("cornell_box", 400, 400, 200, [(196, 196, 8, 8), (57, 311, 8, 8)])])
def test_right_fold_full_spp_crops_match_the_reference_order(scene, nx, ny, ns, rects):
    exact = []
    for rect in rects:
        g = fold_render(scene, nx, ny, ns, seed=2024, rect=rect)
        o = O.render(O.RenderSpec(scene=scene, nx=nx, ny=ny, ns=ns, rng="counter", seed=2024, rect=rect,
                                  threads=THREADS))[0]
        rms = gamma_rms(g, o)
        exact.append(pixel_exact(g, o))
        assert (rms <= TOL_RMS).all(), (rect, rms)
    pinned, why = O.host_libm_pinned()
    print(f"host_libm_pinned: {pinned} ({why})")
    print(f"{scene} {nx}x{ny}x{ns}: crops' bit-exact pixels {exact}")
    assert_exact(min(exact))


# ---- 4. invariances, all bitwise with the flag set ----------------------------------------
def test_right_fold_tile_decomposition_is_bitwise_invariant():
    nx, ny, ns = 64, 48, 8
    full = fold_render("final", nx, ny, ns, seed=3)
    quad = np.zeros_like(full)
    for (x0, y0, w, h) in [(0, 0, 32, 24), (32, 0, 32, 24), (0, 24, 32, 24), (32, 24, 32, 24)]:
        quad[y0:y0 + h, x0:x0 + w] = fold_render("final", nx, ny, ns, seed=3, rect=(x0, y0, w, h))
    assert np.array_equal(bits(full), bits(quad))


def test_right_fold_sample_batches_equal_one_launch(monkeypatch):
    nx, ny, ns = 96, 64, 21
    ref, st1 = fold_render("cornell_box", nx, ny, ns, seed=12, chunk=4, stats=True)
    assert st1["batches"] == 1
    monkeypatch.setenv("RTNW_SLAB_BUDGET", str(nx * ny * 12 * 2))   # 2 chunks of 12-B sums per launch
    img, st = fold_render("cornell_box", nx, ny, ns, seed=12, chunk=4, stats=True)
    assert st["batches"] >= 3, st["batches"]
    assert np.array_equal(bits(img), bits(ref))


def test_right_fold_resumes_from_sums_bitwise():
    nx, ny, ns = 48, 32, 12
    full = fold_render("final", nx, ny, ns, seed=77)
    sums = fold_render("final", nx, ny, 5, seed=77, flags=rtnw.RT_FLAG_SUM_OUT)
    cam = rtnw.Camera.preset("cornell", nx, ny)
    p2 = rtnw.RenderParams(nx, ny, ns - 5, seed=77, sample_offset=5, flags=FOLD | rtnw.RT_FLAG_SUM_IN)
    resumed = _scene("final").render_tile(cam, p2, 0, 0, nx, ny, sums=sums)
    assert np.array_equal(bits(resumed), bits(full))


@pytest.mark.parametrize("scene,nx,ny,ns", [("final", 48, 48, 16), ("cornell_smoke", 32, 32, 8)])
def test_right_fold_search_modes_agree_bitwise(monkeypatch, scene, nx, ny, ns):
    """BVH2 nodes in LDS, in HBM, and the flat scan (width 2's three search modes, each
    with fold variants of its own) give one image."""
    out, how = {}, {}
    monkeypatch.setenv("RTNW_BVH_WIDTH", "2")
    for lds, scan in (("1", "1"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("RTNW_LDS_BVH", lds)
        monkeypatch.setenv("RTNW_SCAN", scan)
        monkeypatch.setenv("RTNW_PRESCAN", "0" if lds == "0" else "1")
        sc = rtnw.Scene.builtin(scene)   # fixed when the scene is built
        try:
            out[lds, scan], st = fold_render(scene, nx, ny, ns, seed=11, chunk=4, stats=True, sc=sc)
        finally:
            sc.close()
        how[lds, scan] = (st["lds_level"], st["scan_groups"] > 0)
    small = scene != "final"   # <= 64 primitives: scanned by default
    assert how == {("1", "1"): (0.0, True) if small else (1.0, False), ("1", "0"): (1.0, False),
                   ("0", "0"): (0.0, False)}, how
    for k, img in out.items():
        assert np.array_equal(bits(img), bits(out["0", "0"])), k


def test_right_fold_ignores_the_ball_waves(monkeypatch):
    nx, ny, ns = 64, 48, 8
    imgs = {}
    for w in ("0", "3"):
        monkeypatch.setenv("RTNW_BALL_WAVES", w)
        imgs[w] = fold_render("final", nx, ny, ns, seed=33)
    assert np.array_equal(bits(imgs["0"]), bits(imgs["3"]))


# ---- 5. validation ---------------------------------------------------------------------------
@pytest.mark.parametrize("other,name", [(rtnw.RT_FLAG_COUNT, "RT_FLAG_COUNT"), (rtnw.RT_FLAG_PROFILE, "RT_FLAG_PROFILE")])
def test_right_fold_with_count_or_profile_is_invalid(other, name):
    with pytest.raises(rtnw.RtError) as e:
        fold_render("final", 16, 16, 2, flags=other)
    assert e.value.code == RT_ERR_INVALID
    assert "RT_FLAG_RIGHT_FOLD" in str(e.value) and name in str(e.value)


def test_right_fold_on_a_wide_bvh_is_unsupported(monkeypatch):
    monkeypatch.setenv("RTNW_BVH_WIDTH", "4")
    sc = rtnw.Scene.builtin("final")
    try:
        with pytest.raises(rtnw.RtError) as e:
            fold_render("final", 16, 16, 2, sc=sc)
    finally:
        sc.close()
    assert e.value.code == RT_ERR_UNSUPPORTED


def test_right_fold_stack_over_the_budget_is_invalid_and_harmless():
    sc = rtnw.Scene.builtin("final")
    cam = rtnw.Camera.preset("cornell", 16, 16)
    try:
        with pytest.raises(rtnw.RtError) as e:
            fold_render("final", 16, 16, 2, max_depth=2 ** 30, sc=sc)
        after = sc.render_tile(cam, rtnw.RenderParams(16, 16, 2, seed=1), 0, 0, 16, 16)
    finally:
        sc.close()
    assert e.value.code == RT_ERR_INVALID
    assert "max_depth" in str(e.value)
    before = _scene("final").render_tile(cam, rtnw.RenderParams(16, 16, 2, seed=1), 0, 0, 16, 16)
    assert np.array_equal(bits(after), bits(before))


# ---- 6. the flag off is untouched ----------------------------------------------------------
def test_flag_off_is_the_kernel_order_and_differs_from_the_fold():
    scene, nx, ny, ns, chunk, seed = "final", 32, 32, 16, 16, 4
    cam_name, bg, depth = rtnw.SCENE_DEFAULTS[scene]
    p = rtnw.RenderParams(nx, ny, ns, max_depth=depth, background=bg, chunk=chunk, seed=seed)
    plain = _scene(scene).render_tile(rtnw.Camera.preset(cam_name, nx, ny), p, 0, 0, nx, ny)
    o = O.render(O.kernel_spec(scene, nx, ny, ns, seed=seed, chunk=chunk, threads=THREADS))[0]
    check_against_oracle("flags 0 against kernel_spec", plain, o)
    fold = fold_render(scene, nx, ny, ns, seed=seed, chunk=chunk)
    assert not np.array_equal(bits(plain), bits(fold))
