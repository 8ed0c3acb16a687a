"""The ball waves' fused in-ball step (rt_megakernel.h stage 3, RTNW_BALL_FAST; DESIGN.md §5c
round 8).

A ball wave serves the segments that start inside final()'s dense medium, are decided by the
medium cell and scatter at a medium in a loop of its own, with the generic stages' own
expressions (lockstep_prims, medium_one, coop_reject_mixed): every sample's draws, adds and slab
slot stay what they were, so every setting must give the framebuffer of a render without ball
waves bit for bit, and the count variant's lane-level totals must not move.  Scene lowering
enables the step only where every medium's material is an isotropic of constant texture.
"""
import ctypes

import numpy as np
import pytest

import rtnw
from test_gpu_parity import _scene, assert_exact, gamma_rms, oracle_render, pixel_exact, TOL_RMS

gpu = pytest.mark.gpu

NX, NY, NS, SEED = 160, 120, 24, 33
KNOBS = ("RTNW_BALL_WAVES", "RTNW_BALL_FAST", "RTNW_BALL_CLAIM", "RTNW_BALL_PARK", "RTNW_BALL_BATCH", "RTNW_BALL_DRAIN",
         "RTNW_SLAB_BUDGET", "RTNW_CELL")
# lane-level totals of the count variant: a segment is counted once, by the path that serves it
TOTALS = ("samples", "segments", "medium_tests", "shades", "lane_scatters", "lane_sphere_draw_trips")
# ... and those that also depend on the lanes a segment shares its wave with (see the count test)
ROUTED = ("sphere_tests", "moving_sphere_tests", "rect_tests")
ROUTED_REL = 0.005   # their bound between two renders, relative (derived in the count test's docstring)


def bits(a):
    return a.view(np.uint32)


def render(monkeypatch, env, *, rect=None, scene="final", stats=False, **params):
    """final() through the `cornell` preset at 160 x 120 x 24 spp, seed 33, under `env` alone."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    p = rtnw.RenderParams(NX, NY, NS, seed=SEED, **params)
    x0, y0, w, h = rect if rect else (0, 0, NX, NY)
    return _scene(scene).render_tile(rtnw.Camera.preset("cornell", NX, NY), p, x0, y0, w, h, stats=stats)


_ref = {}


def reference(monkeypatch, **params):
    """The RTNW_BALL_WAVES=0 framebuffer of the same job, rendered once per parameter set."""
    key = tuple(sorted(params.items()))
    if key not in _ref:
        img = render(monkeypatch, {"RTNW_BALL_WAVES": 0}, **params)
        img.setflags(write=False)
        _ref[key] = img
    return _ref[key]


def fast_env(fast, **more):
    env = dict(more)
    if fast is not None:   # None: the compiled default
        env["RTNW_BALL_FAST"] = fast
    return env


@gpu
@pytest.mark.parametrize("waves", [3, 16])
@pytest.mark.parametrize("fast", [0, None, 1, 64])
def test_thresholds_and_wave_counts_leave_the_image_bitwise_unchanged(monkeypatch, fast, waves):
    ref = reference(monkeypatch)
    assert np.isfinite(ref).all() and ref.max() > 0
    img = render(monkeypatch, fast_env(fast, RTNW_BALL_WAVES=waves))
    differing = int(np.sum(np.any(bits(img) != bits(ref), axis=-1)))
    print(f"fast {fast} waves {waves}: {differing} of {NX * NY} pixels differ")
    assert np.array_equal(bits(img), bits(ref))


@gpu
@pytest.mark.parametrize("max_depth", [1, 2, 50])
def test_the_depth_cap_ends_paths_in_the_generic_code(monkeypatch, max_depth):
    """A lane at the cap is not eligible: its last segment is the generic stages' (a path of
    max_depth 1 never runs a fused trip, one of 2 at most one)."""
    ref = reference(monkeypatch, max_depth=max_depth)
    for fast in (None, 1):
        img = render(monkeypatch, fast_env(fast), max_depth=max_depth)
        assert np.array_equal(bits(img), bits(ref)), (max_depth, fast)


@gpu
def test_chunks_carry_the_partial_sum_through_fused_scatters(monkeypatch):
    ref = reference(monkeypatch, chunk=4)
    for fast in (None, 1):
        img = render(monkeypatch, fast_env(fast), chunk=4)
        assert np.array_equal(bits(img), bits(ref)), fast


@gpu
def test_five_slab_batches(monkeypatch):
    ref = reference(monkeypatch)
    img = render(monkeypatch, {"RTNW_SLAB_BUDGET": NX * NY * 12 * 5})   # 5 samples per launch
    assert np.array_equal(bits(img), bits(ref))


@gpu
def test_the_loop_runs_in_the_drain(monkeypatch):
    """One 8 x 8 tile on the subsurface sphere: 1,536 samples exhaust the claims at once, so the
    ball waves' fused trips all run after the pool is dry."""
    ref = reference(monkeypatch)
    for fast in (None, 1):
        tiny = render(monkeypatch, fast_env(fast), rect=(72, 40, 8, 8))
        assert np.array_equal(bits(tiny), bits(ref[40:48, 72:80])), fast


@gpu
@pytest.mark.parametrize("env", [{"RTNW_BALL_CLAIM": 1}, {"RTNW_BALL_PARK": 0}, {"RTNW_BALL_CLAIM": 1, "RTNW_BALL_PARK": 0}])
def test_claim_and_park_knobs_with_the_step_on(monkeypatch, env):
    ref = reference(monkeypatch)
    for fast in (None, 1):
        img = render(monkeypatch, fast_env(fast, **env))
        assert np.array_equal(bits(img), bits(ref)), (env, fast)
        tiny = render(monkeypatch, fast_env(fast, **env), rect=(72, 40, 8, 8))
        assert np.array_equal(bits(tiny), bits(ref[40:48, 72:80])), (env, fast)


@gpu
@pytest.mark.parametrize("env", [{}, {"RTNW_BALL_WAVES": 16, "RTNW_BALL_PARK": 0}])
def test_count_totals_are_the_same_with_the_step_on_and_off(monkeypatch, env):
    """Samples, segments, medium evaluations, shades, scattering lanes and the sampler's draws
    are properties of the paths: equal with the step on and off under any setting, and asserted so.

    The sphere and rect tests are not a property of the paths in this kernel, with or without
    the step: a lane that holds a leaf keeps taking node steps against its old best_t while the
    rest of its wave still descends (rt_device.h descend), so the primitives a segment tests
    depend on the lanes it shares a wave with, and that on the claims' and the pools' timing.
    Two renders of one setting with the step off differ (measured on this job, every wave a ball
    wave and no parking: sphere tests 4,413,790 and 4,413,631, rect tests 1,124,621 and
    1,124,864, under 0.03 %; between settings 4,402,118 against 4,401,985 and 1,126,416 against
    1,127,176, under 0.07 %).  Exact equality cannot hold, so each of these totals is asserted
    within ROUTED_REL = 0.5 % of the step-off render's.  What the bound is for: the step counts
    the cell's tests for the lanes it serves and takes them back for the others, which the
    generic block then counts.  The step serves about a third of this job's 1.45 M segments, 2
    cell primitives each, against 5.6 M primitive tests in all: dropping its count would lower
    the cell primitives' totals by about a million tests (some 20 % of the sphere tests if both
    are spheres), dropping the take-back (about a tenth of the eligible lanes per trip) would
    raise them by some 2 %, and more at RTNW_BALL_FAST=1, where trips run for a few lanes."""
    _, off = render(monkeypatch, dict(env, RTNW_BALL_FAST=0), flags=rtnw.RT_FLAG_COUNT, stats=True)
    _, off2 = render(monkeypatch, dict(env, RTNW_BALL_FAST=0), flags=rtnw.RT_FLAG_COUNT, stats=True)
    assert off["samples"] == NX * NY * NS and off["medium_tests"] > 0 and off["lane_scatters"] > 0
    for k in ROUTED:
        print(f"{env} off twice {k}: {off[k]:.0f} and {off2[k]:.0f}")
    for k in TOTALS:
        assert off2[k] == off[k], k
    for k in ROUTED:
        assert abs(off2[k] - off[k]) <= ROUTED_REL * off[k], (k, off2[k], off[k])
    for fast in (None, 1, 64):
        img, on = render(monkeypatch, fast_env(fast, **env), flags=rtnw.RT_FLAG_COUNT, stats=True)
        for k in TOTALS + ROUTED:
            print(f"{env} fast {fast} {k}: {on[k]:.0f} (off {off[k]:.0f})")
        for k in TOTALS:
            assert on[k] == off[k], (fast, k)
        for k in ROUTED:
            assert abs(on[k] - off[k]) <= ROUTED_REL * off[k], (fast, k, on[k], off[k])
        assert np.array_equal(bits(img), bits(reference(monkeypatch)))


@gpu
def test_the_balls_pixels_equal_the_oracle(monkeypatch):
    img = render(monkeypatch, {})
    o = oracle_render("final", NX, NY, NS, seed=SEED, chunk=1, rect=(72, 40, 8, 8))
    crop = np.ascontiguousarray(img[40:48, 72:80])
    rms = gamma_rms(crop, o)
    exact = pixel_exact(crop, o)
    print(f"ball crop: gamma RMS {rms}, bit-exact pixels {exact:.4f}")
    assert (rms <= TOL_RMS).all(), rms
    assert_exact(exact)


@gpu
def test_a_scene_that_does_not_qualify_renders_the_same(monkeypatch):
    """cornell_smoke's media sit in instance chains (no medium cell): the step stays off."""
    a = render(monkeypatch, {}, scene="cornell_smoke")
    b = render(monkeypatch, {"RTNW_BALL_FAST": 0}, scene="cornell_smoke")
    c = render(monkeypatch, {"RTNW_BALL_FAST": 1}, scene="cornell_smoke")
    assert a.max() > 0
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))


# ------------------------------------------------------------------ scene lowering, no GPU
def lowering_enables(desc):
    fn = rtnw.lib().rt_scene_desc_ball_fast
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(rtnw.RtSceneDesc)]
    rc = fn(desc.ptr)
    assert rc >= 0, rtnw.lib().rt_last_error().decode()
    return rc == 1


def test_lowering_enables_the_step_for_constant_isotropic_media_only():
    RT_MAT_ISOTROPIC, RT_MAT_LAMBERTIAN, RT_TEX_CONSTANT, RT_TEX_NOISE = 4, 0, 0, 2
    assert lowering_enables(rtnw.SceneDesc.builtin("final"))
    assert not lowering_enables(rtnw.SceneDesc.builtin("cornell_smoke"))   # instanced boundaries: no medium cell
    assert not lowering_enables(rtnw.SceneDesc.builtin("cornell_box"))     # no media

    # final() with the dense medium's isotropic reading the scene's noise texture instead
    desc = rtnw.SceneDesc.builtin("final")
    d = desc.contents
    assert d.nmedia == 2
    dense = max(range(d.nmedia), key=lambda i: d.media[i].density)
    m = d.media[dense].material
    assert d.materials[m].kind == RT_MAT_ISOTROPIC and d.textures[d.materials[m].texture].kind == RT_TEX_CONSTANT
    noise = [t for t in range(d.ntextures) if d.textures[t].kind == RT_TEX_NOISE]
    assert noise
    d.materials[m].texture = noise[0]
    assert not lowering_enables(desc)

    # ... and with the fog's material no isotropic
    desc = rtnw.SceneDesc.builtin("final")
    d = desc.contents
    d.materials[d.media[1 - dense].material].kind = RT_MAT_LAMBERTIAN
    assert not lowering_enables(desc)


def test_lowering_answers_for_the_generated_ball_cases():
    """tests/gen_scenes.py ball_*: 1 for every variant the step is meant to run on; 0 for three
    media and for a noise texture; 1 for with_instance, where lowering says yes and the kernel
    variant with instance chains has no ball waves (tests/test_gpu_ball_generated.py)."""
    import gen_scenes as G
    want = {v: True for v in G.BALL_QUALIFY}
    want.update(three_media=False, noise_medium=False, with_instance=True)
    assert set(want) == set(G.BALL_QUALIFY + G.BALL_DECLINE)
    for v, w in want.items():
        desc, _ = G.build(G.BY_NAME["ball_" + v])
        d = desc.contents
        assert lowering_enables(desc) == w, v
        assert d.nprims > 64 and d.ninstances == (1 if v == "with_instance" else 0), v
        # every medium an isotropic; of a constant texture (noise_medium's second apart), pairwise distinct, no 0 or 1
        cols = []
        for i in range(d.nmedia):
            m = d.materials[d.media[i].material]
            assert m.kind == 4
            t = d.textures[m.texture]
            if t.kind == 0:
                cols.append(tuple(t.color))
        assert len(cols) == d.nmedia - (v == "noise_medium") and len(set(cols)) == len(cols), v
        assert all(0 < x < 1 for col in cols for x in col), v
