"""Camera samples of provably empty pixels finished at the work claim (rt_megakernel.h refill,
RTNW_EMPTY_FAST).

refill builds such a sample's pinhole ray, runs the media against t_max = FLT_MAX from the
sample's own medium stream with the generic stages' own functions and, unless a medium scatters,
writes the miss radiance to the sample's slab slot and drops the item; a sample that scatters
stays among the sample starts and is served from scratch.  So the framebuffer must be the same
bit for bit with the feature on and off and equal to the oracle's, under every way the claims
can fall (batches, sample offsets, claim sizes, the drain, rank shares), the count variant's
path totals must not move, and rt_stats.empty_fast_samples must say that the path ran.

Mutations of refill that each fail tests here are listed in profiles/r16/README.md.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import gen_scenes as G
import oracle as O
import rtnw
from test_gpu_parity import THREADS, TOL_RMS, _scene, assert_exact, gamma_rms, pixel_exact

pytestmark = pytest.mark.gpu

KNOBS = ("RTNW_EMPTY_FAST", "RTNW_SLAB_BUDGET", "RTNW_CLAIM", "RTNW_TAIL_CLAIMS")
BG = {"sky": rtnw.RT_BG_SKY, "black": rtnw.RT_BG_BLACK}
TOTALS = ("samples", "segments", "medium_tests", "shades")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def check_oracle(what, g, o):
    rms, exact = gamma_rms(g, o), pixel_exact(g, o)
    print(f"{what}: gamma RMS {rms}, bit-exact pixels {exact:.4f}")
    assert (rms <= TOL_RMS).all(), rms
    assert_exact(exact)


def pinhole(name, nx, ny):
    p = rtnw.CAMERA_PRESETS[name]
    return rtnw.Camera(p["lookfrom"], p["lookat"], (0, 1, 0), p["vfov"], float(np.float32(nx) / np.float32(ny)), 0.0, 10.0, 0.0, 1.0)


def render(monkeypatch, sc, cam, p, env, rect=None, stats=False):
    set_env(monkeypatch, env)
    x0, y0, w, h = rect if rect else (0, 0, p.nx, p.ny)
    return sc.render_tile(cam, p, x0, y0, w, h, stats=stats)


def on_off_count(monkeypatch, sc, cam, nx, ny, ns, **kw):
    """The job with the feature on and off in the plain and the count variant: the four images
    bitwise equal, the path totals equal.  Returns (image, rt_stats with the feature on)."""
    p = rtnw.RenderParams(nx, ny, ns, chunk=1, **kw)
    pc = rtnw.RenderParams(nx, ny, ns, chunk=1, flags=rtnw.RT_FLAG_COUNT, **kw)
    on = render(monkeypatch, sc, cam, p, {})
    off = render(monkeypatch, sc, cam, p, {"RTNW_EMPTY_FAST": 0})
    con, son = render(monkeypatch, sc, cam, pc, {}, stats=True)
    coff, soff = render(monkeypatch, sc, cam, pc, {"RTNW_EMPTY_FAST": 0}, stats=True)
    assert np.isfinite(on).all()
    assert np.array_equal(bits(on), bits(off))
    assert np.array_equal(bits(con), bits(on)) and np.array_equal(bits(coff), bits(on))
    print({k: (son[k], soff[k]) for k in TOTALS + ("empty_fast_samples", "empty_pixels")})
    for k in TOTALS:
        assert son[k] == soff[k], k
    assert son["samples"] == nx * ny * ns
    assert soff["empty_fast_samples"] == 0 and soff["empty_pixels"] == 0
    assert son["empty_fast_samples"] <= son["empty_pixels"] * ns
    return on, son


# ------------------------------------------------------------------ the built-in scenes
def test_final_64x64x8_on_off_and_oracle(monkeypatch):
    nx, ny, ns, seed = 64, 64, 8, 21
    img, st = on_off_count(monkeypatch, _scene("final"), rtnw.Camera.preset("cornell", nx, ny), nx, ny, ns, seed=seed)
    assert 0 < st["empty_fast_samples"] < st["empty_pixels"] * ns   # both outcomes: the fog scatters some
    check_oracle("final", img, O.render(O.kernel_spec("final", nx, ny, ns, seed=seed, chunk=1, threads=THREADS))[0])


def test_final_50x37x4_as_two_tiles_with_offsets(monkeypatch):
    """A frame whose width is no multiple of 8, as a job of two tiles that start off the
    frame's origin (claims of 64 items run across the bands' ragged ends and across tiles)."""
    nx, ny, ns, seed = 50, 37, 4, 22
    tiles = [(1, 2, 27, 33), (28, 1, 21, 35)]
    sc, cam = _scene("final"), rtnw.Camera.preset("cornell", nx, ny)
    L = rtnw.lib()
    n = sum(w * h for _, _, w, h in tiles) * 3
    out = {}
    for flags in (0, rtnw.RT_FLAG_COUNT):
        for knob in ("1", "0"):
            set_env(monkeypatch, {"RTNW_EMPTY_FAST": knob})
            dev = ctypes.c_void_p()
            assert L.rt_device_alloc(0, n * 4, ctypes.byref(dev)) == 0
            st = sc.render_tiles(cam, rtnw.RenderParams(nx, ny, ns, chunk=1, seed=seed, flags=flags), tiles, dev.value)
            packed = np.zeros(n, np.float32)
            assert L.rt_copy_to_host(packed.ctypes.data, dev, n * 4) == 0
            L.rt_device_free(dev)
            out[flags, knob] = (packed, st)
    ref = out[0, "0"][0]
    for k, (packed, _) in out.items():
        assert np.array_equal(bits(packed), bits(ref)), k
    son, soff = out[rtnw.RT_FLAG_COUNT, "1"][1], out[rtnw.RT_FLAG_COUNT, "0"][1]
    for k in TOTALS:
        assert son[k] == soff[k], k
    assert 0 < son["empty_fast_samples"] <= son["empty_pixels"] * ns and soff["empty_fast_samples"] == 0
    img = rtnw.unpack_tiles(ref, tiles, np.zeros((ny, nx, 3), np.float32))
    for x0, y0, w, h in tiles:
        o = O.render(O.kernel_spec("final", nx, ny, ns, seed=seed, chunk=1, rect=(x0, y0, w, h), threads=THREADS))[0]
        check_oracle(f"final tile {x0},{y0}", np.ascontiguousarray(img[y0:y0 + h, x0:x0 + w]), o)


def test_random_motion_64x32x4_sky_and_no_media(monkeypatch):
    """random_motion through a pinhole, under the sky.  Its kernel variant (checker textures, a
    pre-scanned ground) does not carry refill's code, which cost c3 1.2 % by its mere presence
    (DESIGN.md §5c round 16): the scene leaves the feature off, and the image is the oracle's."""
    nx, ny, ns, seed = 64, 32, 4, 23
    cam = pinhole("random", nx, ny)
    img, st = on_off_count(monkeypatch, _scene("random_motion"), cam, nx, ny, ns, seed=seed, background=rtnw.RT_BG_SKY)
    assert st["empty_pixels"] == 0 and st["empty_fast_samples"] == 0
    o = O.render_desc(rtnw.SceneDesc.builtin("random_motion"), cam,
                      O.desc_spec(nx, ny, ns, max_depth=50, background="sky", seed=seed, chunk=1, threads=THREADS))[0]
    check_oracle("random_motion pinhole", img, o)


def test_a_scene_without_media_under_the_sky(monkeypatch):
    """edge_single (one sphere, no medium, no feature: the media variant with an empty media
    list) through a pinhole: the sky's radiance reads the ray's unit direction, and with no
    medium every sample of a flagged pixel is decided at the claim.  Through the preset's lens
    (aperture 0.1) the feature is off."""
    nx, ny, ns, seed = 64, 32, 4, 23
    cam = pinhole("random", nx, ny)
    img, st = on_off_count(monkeypatch, _scene("edge_single"), cam, nx, ny, ns, seed=seed, background=rtnw.RT_BG_SKY)
    assert st["empty_pixels"] > 0.5 * nx * ny and st["empty_fast_samples"] == st["empty_pixels"] * ns
    o = O.render_desc(rtnw.SceneDesc.builtin("edge_single"), cam,
                      O.desc_spec(nx, ny, ns, max_depth=50, background="sky", seed=seed, chunk=1, threads=THREADS))[0]
    check_oracle("edge_single pinhole", img, o)
    _, lens = render(monkeypatch, _scene("edge_single"), rtnw.Camera.preset("random", nx, ny),
                     rtnw.RenderParams(nx, ny, ns, chunk=1, seed=seed, background=rtnw.RT_BG_SKY, flags=rtnw.RT_FLAG_COUNT), {},
                     stats=True)
    assert lens["empty_fast_samples"] == 0 and lens["empty_pixels"] == 0


def test_cornell_smoke_32x32x2_flags_nothing(monkeypatch):
    nx, ny, ns, seed = 32, 32, 2, 24
    img, st = on_off_count(monkeypatch, _scene("cornell_smoke"), rtnw.Camera.preset("cornell", nx, ny), nx, ny, ns, seed=seed)
    assert st["empty_fast_samples"] == 0 and st["empty_pixels"] == 0
    check_oracle("cornell_smoke", img, O.render(O.kernel_spec("cornell_smoke", nx, ny, ns, seed=seed, chunk=1, threads=THREADS))[0])


# ------------------------------------------------------------------ generated scenes
def fog_desc(moving_boundary=False):
    """70 small spheres in a fog ball of radius 30 around them and the camera, whose mean free path
    (50) is near the scene's size: a primary ray that leaves through the ball's far side, 39 away,
    scatters with probability 1 - exp(-39 / 50) ~ 0.54, so blocks hold both outcomes.  More than
    64 primitives: the BVH variants (final()'s)."""
    b = G.Builder(np.random.default_rng(11))
    b.add(*G.small_spheres(b, 70, lo=(-1.5, 0.2, -1.5), hi=(1.5, 2.0, 1.5), r=(0.08, 0.2)))
    g = b.glass()
    bound = b.msphere((0, 1, 0), (0.2, 1, 0), 0, 1, 30.0, g) if moving_boundary else b.sphere((0, 1, 0), 30.0, g)
    b.medium(bound, 0.02, b.const(0.8, 0.8, 0.8))
    return b.desc()


def fog_camera(nx, ny, aperture=0.0, lookfrom=(0.0, 1.5, 9.0)):
    return rtnw.Camera(lookfrom, (0, 1, 0), (0, 1, 0), 40.0, float(np.float32(nx) / np.float32(ny)), aperture, 9.0, 0.0, 1.0)


def nine_media_desc():
    """Six spheres and nine nested fog balls around them and the camera (radii 12 .. 20, a mean
    free path of 250 each): every primary ray crosses all nine, some 225 of path in all, so about
    0.4 of the rays leave unscattered, and the ninth, which the kernel reads from HBM
    (RT_LDS_MEDIA = 8), scatters about a tenth of the rays that reach it.  At most 64 primitives:
    the flat-scan variant."""
    b = G.Builder(np.random.default_rng(12))
    b.add(*G.small_spheres(b, 6, lo=(-1.5, 0.3, -1.5), hi=(1.5, 2.0, 1.5), r=(0.2, 0.4)))
    g = b.glass()
    for k in range(9):
        b.medium(b.sphere((0.1 * k, 1.0, 0.05 * k), 12.0 + k, g), 0.004, b.const(0.2 + 0.08 * k, 0.9 - 0.07 * k, 0.5))
    return b.desc()


_gen = {}


def generated(name):
    if name not in _gen:
        desc = {"fog": fog_desc, "nine": nine_media_desc}[name]()
        _gen[name] = (desc, rtnw.Scene(desc))
    return _gen[name]


@pytest.mark.parametrize("name,bg", [("fog", "black"), ("fog", "sky"), ("nine", "sky")])
def test_generated_media_scenes_32x32x16(monkeypatch, name, bg):
    nx, ny, ns, seed = 32, 32, 16, 25
    desc, sc = generated(name)
    cam = fog_camera(nx, ny)
    img, st = on_off_count(monkeypatch, sc, cam, nx, ny, ns, seed=seed, background=BG[bg])
    flagged = st["empty_pixels"]
    # both outcomes, and often: between a tenth and nine tenths of the flagged pixels' samples scatter
    assert flagged > 0.3 * nx * ny and 0.1 * flagged * ns < st["empty_fast_samples"] < 0.9 * flagged * ns
    assert st["scan_groups"] == (1 if name == "nine" else 0)
    o = O.render_desc(desc, cam, O.desc_spec(nx, ny, ns, max_depth=50, background=bg, seed=seed, chunk=1, threads=THREADS))[0]
    check_oracle(f"{name} {bg}", img, o)


# ------------------------------------------------------------------ the ways claims fall
NX, NY, NS, SEED = 64, 64, 8, 26
_ref = {}


def final_reference(monkeypatch, **kw):
    """final() 64 x 64 x 8 with the feature off, once per parameter set."""
    key = tuple(sorted(kw.items()))
    if key not in _ref:
        img = render(monkeypatch, _scene("final"), rtnw.Camera.preset("cornell", NX, NY),
                     rtnw.RenderParams(NX, NY, NS, chunk=1, seed=SEED, **kw), {"RTNW_EMPTY_FAST": 0})
        img.setflags(write=False)
        _ref[key] = img
    return _ref[key]


@pytest.mark.parametrize("env", [{"RTNW_SLAB_BUDGET": NX * NY * 12 * 3}, {"RTNW_CLAIM": 1}, {"RTNW_CLAIM": 1, "RTNW_TAIL_CLAIMS": 0},
                                 {"RTNW_CLAIM": 8, "RTNW_TAIL_CLAIMS": 0}], ids=str)
def test_batches_and_claim_sizes(monkeypatch, env):
    """Three sample batches (3 + 3 + 2 samples per launch), and claims of 64 and of 512 items."""
    ref = final_reference(monkeypatch)
    p = rtnw.RenderParams(NX, NY, NS, chunk=1, seed=SEED, flags=rtnw.RT_FLAG_COUNT)
    img, st = render(monkeypatch, _scene("final"), rtnw.Camera.preset("cornell", NX, NY), p, env, stats=True)
    assert np.array_equal(bits(img), bits(ref))
    assert st["empty_fast_samples"] > 0 and st["batches"] == (3 if "RTNW_SLAB_BUDGET" in env else 1)


def test_sample_offset(monkeypatch):
    """Samples 5 .. 12 of every pixel: the keys, and so the medium streams, are those samples'."""
    ref = final_reference(monkeypatch, sample_offset=5)
    assert not np.array_equal(bits(ref), bits(final_reference(monkeypatch)))
    p = rtnw.RenderParams(NX, NY, NS, chunk=1, seed=SEED, sample_offset=5)
    img = render(monkeypatch, _scene("final"), rtnw.Camera.preset("cornell", NX, NY), p, {})
    assert np.array_equal(bits(img), bits(ref))
    o = O.render(O.kernel_spec("final", NX, NY, NS, seed=SEED, chunk=1, sample_offset=5, rect=(0, 0, NX, 16), threads=THREADS))[0]
    check_oracle("final samples 5..12, top rows", np.ascontiguousarray(img[:16]), o)


def test_an_8x8_job_runs_in_the_drain(monkeypatch):
    """One block of sky (the frame's top left corner: every pixel flagged) and one on the scene:
    512 samples exhaust the claims at once."""
    ref = final_reference(monkeypatch)
    p = rtnw.RenderParams(NX, NY, NS, chunk=1, seed=SEED, flags=rtnw.RT_FLAG_COUNT)
    for rect, all_flagged in (((0, 0, 8, 8), True), ((24, 40, 8, 8), False)):
        tiny, st = render(monkeypatch, _scene("final"), rtnw.Camera.preset("cornell", NX, NY), p, {}, rect=rect, stats=True)
        x0, y0, w, h = rect
        assert np.array_equal(bits(tiny), bits(ref[y0:y0 + h, x0:x0 + w])), rect
        if all_flagged:
            assert st["empty_pixels"] == 64 and 0 < st["empty_fast_samples"] < 64 * NS


@pytest.mark.parametrize("world", [2, 3])
def test_rank_shares_give_the_one_gpu_image(monkeypatch, world):
    """The interleaved pixel shares of `world` ranks (rtnw.pixels_for_rank: jobs of 1 x 1 tiles
    whose neighbours in the list are `world` pixels apart), gathered."""
    ref = final_reference(monkeypatch)
    set_env(monkeypatch, {})
    sc, cam = _scene("final"), rtnw.Camera.preset("cornell", NX, NY)
    L = rtnw.lib()
    img = np.zeros((NY, NX, 3), np.float32)
    fast = 0
    for r in range(world):
        tiles = rtnw.pixels_for_rank(NX, NY, r, world)
        n = len(tiles) * 3
        dev = ctypes.c_void_p()
        assert L.rt_device_alloc(0, n * 4, ctypes.byref(dev)) == 0
        st = sc.render_tiles(cam, rtnw.RenderParams(NX, NY, NS, chunk=1, seed=SEED, flags=rtnw.RT_FLAG_COUNT), tiles, dev.value)
        fast += st["empty_fast_samples"]
        packed = np.zeros(n, np.float32)
        assert L.rt_copy_to_host(packed.ctypes.data, dev, n * 4) == 0
        L.rt_device_free(dev)
        rtnw.unpack_tiles(packed, tiles, img)
    assert np.array_equal(bits(img), bits(ref))
    assert fast > 0


# ------------------------------------------------------------------ the feature turns itself off
def test_each_self_disabling_condition_counts_no_fast_sample(monkeypatch):
    nx, ny, ns, seed = 32, 32, 4, 27
    desc, sc = generated("fog")

    def fast(scene, cam, env=None, **kw):
        kw.setdefault("chunk", 1)
        p = rtnw.RenderParams(nx, ny, ns, seed=seed, flags=rtnw.RT_FLAG_COUNT, **kw)
        _, st = render(monkeypatch, scene, cam, p, env or {}, stats=True)
        assert st["samples"] == nx * ny * ns
        return st["empty_fast_samples"], st["empty_pixels"]

    f, n = fast(sc, fog_camera(nx, ny))
    assert 0 < f < n * ns
    assert fast(sc, fog_camera(nx, ny), t_min=0.0)[0] > 0
    assert fast(sc, fog_camera(nx, ny), {"RTNW_EMPTY_FAST": 0}) == (0, 0)
    assert fast(sc, fog_camera(nx, ny, aperture=0.1)) == (0, 0)                    # lens > 0
    assert fast(sc, fog_camera(nx, ny), t_min=-1.0) == (0, 0)                      # t_min < 0
    assert fast(sc, fog_camera(nx, ny, lookfrom=(-0.0, 1.5, 9.0))) == (0, 0)       # a -0.0 origin component
    assert fast(sc, fog_camera(nx, ny), chunk=2) == (0, 0)                         # two samples per work item
    moving = rtnw.Scene(fog_desc(moving_boundary=True))                            # a moving boundary, the shutter open
    assert fast(moving, fog_camera(nx, ny)) == (0, 0)
    moving.close()


def test_right_fold_and_chunks_render_as_without_the_feature(monkeypatch):
    """Renders that leave the feature off right after one that used the job's bits (the job
    cache holds them): the right fold and two samples per work item."""
    nx, ny, ns, seed = 32, 32, 4, 28
    desc, sc = generated("fog")
    cam = fog_camera(nx, ny)
    for kw in (dict(chunk=1, flags=rtnw.RT_FLAG_RIGHT_FOLD), dict(chunk=2)):
        render(monkeypatch, sc, cam, rtnw.RenderParams(nx, ny, ns, chunk=1, seed=seed), {})
        a = render(monkeypatch, sc, cam, rtnw.RenderParams(nx, ny, ns, seed=seed, **kw), {})
        b = render(monkeypatch, sc, cam, rtnw.RenderParams(nx, ny, ns, seed=seed, **kw), {"RTNW_EMPTY_FAST": 0})
        assert np.array_equal(bits(a), bits(b)), kw


def test_a_camera_change_remakes_the_bits(monkeypatch):
    """The bits are cached with the job's pixel lists under a key that holds the camera: the same
    tiles through another camera must not reuse them."""
    nx, ny, ns, seed = 32, 32, 4, 29
    desc, sc = generated("fog")
    p = rtnw.RenderParams(nx, ny, ns, chunk=1, seed=seed)
    for lookfrom in ((0.0, 1.5, 9.0), (6.0, 4.0, 5.0), (0.0, 1.5, 9.0)):
        cam = fog_camera(nx, ny, lookfrom=lookfrom)
        a = render(monkeypatch, sc, cam, p, {})
        b = render(monkeypatch, sc, cam, p, {"RTNW_EMPTY_FAST": 0})
        assert np.array_equal(bits(a), bits(b)), lookfrom
