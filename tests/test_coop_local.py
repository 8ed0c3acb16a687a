"""The shading stage's rejection sampler with local first candidates (rt_device.h
coop_reject_mixed, RTNW_COOP_LOCAL / RTNW_COOP_LOCAL_MIN).

A requesting lane's local candidates are the first iterations of its own sequential
rejection loop (material.h:41-47, camera.h:6-12), so every setting of the knobs must give
the framebuffer of RTNW_COOP_LOCAL=0 bit for bit, and the candidates each owner consumes
(lane_sphere_draw_trips of the count variant) must not change either.  The four scenes
cover the LDS-BVH variant with ball waves (final), the instance + media variant
(cornell_smoke), a non-zero aperture with the pre-scan (random_motion) and the flat scan
(cornell_box).
"""
import numpy as np
import pytest

import rtnw
from test_gpu_parity import _scene, assert_exact, gamma_rms, oracle_render, pixel_exact, TOL_RMS

pytestmark = pytest.mark.gpu

SCENES = ["final", "cornell_smoke", "random_motion", "cornell_box"]
SETTINGS = [(1, 1), (2, 33), (3, 64), (2, 1)]   # (RTNW_COOP_LOCAL, RTNW_COOP_LOCAL_MIN)
NX = NY = 64
NS = 8
SEED = 19
CHUNK = 8


def bits(a):
    return a.view(np.uint32)


def render(monkeypatch, scene, nx, ny, ns, local, nmin=None, flags=0, stats=False):
    monkeypatch.setenv("RTNW_COOP_LOCAL", str(local))
    if nmin is None:
        monkeypatch.delenv("RTNW_COOP_LOCAL_MIN", raising=False)
    else:
        monkeypatch.setenv("RTNW_COOP_LOCAL_MIN", str(nmin))
    cam_name, bg, depth = rtnw.SCENE_DEFAULTS[scene]
    p = rtnw.RenderParams(nx, ny, ns, max_depth=depth, background=bg, chunk=CHUNK, seed=SEED, flags=flags)
    return _scene(scene).render_tile(rtnw.Camera.preset(cam_name, nx, ny), p, 0, 0, nx, ny, stats=stats)


_base = {}


def base_image(monkeypatch, scene, nx=NX, ny=NY, ns=NS):
    """The RTNW_COOP_LOCAL=0 framebuffer (the cooperative rounds alone), rendered once."""
    key = (scene, nx, ny, ns)
    if key not in _base:
        img = render(monkeypatch, scene, nx, ny, ns, 0)
        img.setflags(write=False)
        _base[key] = img
    return _base[key]


@pytest.mark.parametrize("local,nmin", SETTINGS)
@pytest.mark.parametrize("scene", SCENES)
def test_local_candidates_leave_the_framebuffer_bitwise_unchanged(monkeypatch, scene, local, nmin):
    ref = base_image(monkeypatch, scene)
    assert np.isfinite(ref).all() and ref.max() > 0
    img = render(monkeypatch, scene, NX, NY, NS, local, nmin)
    differing = int(np.sum(np.any(bits(img) != bits(ref), axis=-1)))
    print(f"{scene} local {local} min {nmin}: {differing} of {NX * NY} pixels differ")
    assert np.array_equal(bits(img), bits(ref))


def test_default_setting_is_the_same_framebuffer(monkeypatch):
    ref = base_image(monkeypatch, "final")
    for name in ("RTNW_COOP_LOCAL", "RTNW_COOP_LOCAL_MIN"):
        monkeypatch.delenv(name, raising=False)
    cam_name, bg, depth = rtnw.SCENE_DEFAULTS["final"]
    p = rtnw.RenderParams(NX, NY, NS, max_depth=depth, background=bg, chunk=CHUNK, seed=SEED)
    img = _scene("final").render_tile(rtnw.Camera.preset(cam_name, NX, NY), p, 0, 0, NX, NY)
    assert np.array_equal(bits(img), bits(ref))


def test_final_equals_the_oracle_image(monkeypatch):
    """The unchanged image is the oracle's kernel_spec image (bit for bit where the host libm is pinned)."""
    o = oracle_render("final", NX, NY, NS, seed=SEED, chunk=CHUNK)
    for local, nmin in [(0, None)] + SETTINGS:
        g = render(monkeypatch, "final", NX, NY, NS, local, nmin)
        rms = gamma_rms(g, o)
        exact = pixel_exact(g, o)
        print(f"final local {local} min {nmin}: gamma RMS {rms}, bit-exact pixels {exact:.4f}")
        assert (rms <= TOL_RMS).all(), rms
        assert_exact(exact)


@pytest.mark.parametrize("nmin", [1, 64])
def test_threshold_extremes_on_a_tiny_job(monkeypatch, nmin):
    """16 x 16 x 2 spp: 512 samples over the whole grid leave every wave a few lanes, so
    min = 1 runs the local candidates with very few requesters and min = 64 never runs them."""
    nx = ny = 16
    ns = 2
    ref = base_image(monkeypatch, "final", nx, ny, ns)
    for local in (1, 2, 3):
        img = render(monkeypatch, "final", nx, ny, ns, local, nmin)
        assert np.array_equal(bits(img), bits(ref)), local


@pytest.mark.parametrize("scene", ["final", "random_motion"])
def test_owners_consume_the_same_candidates(monkeypatch, scene):
    """Count variant: the candidates the owners consumed (tried locally or handed out by a
    round) are those of their sequential loops whatever the setting; the image stays too."""
    _, st0 = render(monkeypatch, scene, NX, NY, NS, 0, flags=rtnw.RT_FLAG_COUNT, stats=True)
    assert st0["lane_sphere_draw_trips"] > 0 and st0["wave_sphere_draw_trips"] > 0
    for local, nmin in SETTINGS:
        img, st = render(monkeypatch, scene, NX, NY, NS, local, nmin, flags=rtnw.RT_FLAG_COUNT, stats=True)
        print(f"{scene} local {local} min {nmin}: lane trips {st['lane_sphere_draw_trips']:.0f} "
              f"(rounds alone {st0['lane_sphere_draw_trips']:.0f}), wave trips {st['wave_sphere_draw_trips']:.0f} "
              f"(rounds alone {st0['wave_sphere_draw_trips']:.0f})")
        assert st["lane_sphere_draw_trips"] == st0["lane_sphere_draw_trips"]
        assert st["samples"] == st0["samples"] and st["segments"] == st0["segments"]
        assert np.array_equal(bits(img), bits(base_image(monkeypatch, scene)))
