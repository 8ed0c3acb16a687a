"""Radiance queries on the GPU (rt_radiance_rays and its _dev form) held to the
ray-tracing identity of rt_hip.h: a record that restates the camera ray of (pixel, sample), with
the draws that sample spent before color() as its skip, must come back with that sample's
radiance: one pixel of rt_render_tile(spp = 1, sample_offset = sample), bit for bit, and through
it the oracle's image.  The rays are made outside the library by test_radiance_spec's
lens_camera_rays (the oracle's camera with its lens and shutter).  Every comparison is of bits:
there is no tolerance in this file.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import gen_scenes as G
import oracle as O
import rtnw
from test_gpu_generated import BG, params, spec
from test_gpu_parity import LIBM_PINNED
from test_radiance_spec import camera_records as records_of

pytestmark = pytest.mark.gpu

BALL = "ball_" + G.BALL_QUALIFY[0]
CASES = ["scan64_mixed", "scan65_mixed", "prescan9", "media9_scan", "media9_bvh", "boundaries_bvh", "cell_near_inst_moving",
         BALL, "cloud1736", "quad4095", "chains_long", "image_rects", "textures_by_kind"]
RT_ERR_UNSUPPORTED = -4


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def same_records(a, b):
    return a.dtype == b.dtype == rtnw.RADIANCE_DTYPE and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def qparams(c, **kw):
    """The query's parameters: what it reads of the case's (max_depth, background, seed; t_min is
    the default of both), with a frame and a sample count it must ignore."""
    kw = dict(dict(max_depth=c.max_depth, background=BG[c.background], seed=c.seed), **kw)
    return rtnw.RenderParams(7, 5, 3, chunk=2, sample_offset=11, **kw)


def camera_records(c, cam):
    """The rt_path_ray records of every camera sample of the case's frame through `cam`."""
    return records_of(cam, c.nx, c.ny, c.spp, c.seed)


_views = {}


def view(name):
    """(case, desc, camera, scene, rays, records) of a case through its own camera, made once and
    left unchanged."""
    if name not in _views:
        c = G.BY_NAME[name]
        desc, cam = G.build(c)
        sc = rtnw.Scene(desc)
        rays = camera_records(c, cam)
        _views[name] = (c, desc, cam, sc, rays, sc.radiance_rays(qparams(c), rays))
    return _views[name]


def sample_render(c, sc, cam, s, **kw):
    """The frame's image of sample s alone."""
    kw = dict(dict(max_depth=c.max_depth, background=BG[c.background], seed=c.seed), **kw)
    p = rtnw.RenderParams(c.nx, c.ny, 1, chunk=1, sample_offset=s, **kw)
    return sc.render_tile(cam, p, 0, 0, c.nx, c.ny)


# ------------------------------------------------------------------ 1. the identity
@pytest.mark.parametrize("name", CASES)
def test_camera_records_return_the_renders_samples_and_the_oracles_image(name):
    c, desc, cam, sc, rays, rec = view(name)
    # asserted, not tolerated: a zero component would put rects outside the parity contract
    assert (rays["dir"] != 0).all(), "a rebuilt camera ray has a zero direction component: change the seed"
    assert rays["skip"].min() == 5 and rays["skip"].max() > 5 and rays["skip"].max() <= rtnw.RT_RADIANCE_MAX_SKIP
    assert (rec["status"] == 0).all()
    rgb = rec["rgb"].reshape(c.ny, c.nx, c.spp, 3)
    acc = np.zeros((c.ny, c.nx, 3), np.float32)
    for s in range(c.spp):
        img = sample_render(c, sc, cam, s)
        differ = int((bits(rgb[:, :, s]) != bits(img)).any(axis=-1).sum())
        print(f"{name} sample {s}: {differ} of {c.nx * c.ny} pixels differ from the render")
        assert differ == 0
        acc = acc + rgb[:, :, s]                    # col += temp, main.cpp:311
    mean = acc * np.float32(1.0 / c.spp)            # vec3.h:134-141
    assert mean.dtype == np.float32
    full = sc.render_tile(cam, params(c, chunk=1), 0, 0, c.nx, c.ny)
    assert same(mean, full)
    ref = O.render_desc(desc, cam, spec(c, chunk=1))[0]
    agree = (bits(full) == bits(ref)).all(axis=-1)   # where the render itself is the oracle's, bit for bit: everywhere ...
    print(f"{name}: the render equals the oracle on {agree.mean():.4f} of the pixels; lit share {float((mean > 0).mean()):.3f}")
    if LIBM_PINNED:                                  # ... on a host whose libm is the one rt_libm.h restates
        assert agree.all()
    assert agree.mean() > 0.5 and same(mean[agree], ref[agree])
    assert (mean > 0).any()


# ------------------------------------------------------------------ 2. per-ray independence
def test_a_shuffled_batch_returns_the_shuffled_records():
    c, _, _, sc, rays, rec = view("scan65_mixed")
    order = np.random.default_rng(3).permutation(len(rays))
    assert same_records(sc.radiance_rays(qparams(c), rays[order]), rec[order])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 513])
def test_any_number_of_rays_returns_a_prefix(n):
    c, _, _, sc, rays, rec = view("scan65_mixed")
    assert n <= len(rays)
    assert same_records(sc.radiance_rays(qparams(c), rays[:n]), rec[:n])


CHILD = """
import sys
sys.path[:0] = {paths!r}
import numpy as np
import gen_scenes as G, rtnw
from test_radiance_spec import camera_records
c = G.BY_NAME[{name!r}]
desc, cam = G.build(c)
sc = rtnw.Scene(desc)
p = rtnw.RenderParams(1, 1, 1, max_depth=c.max_depth, background={bg!r}[c.background], seed=c.seed)
try:
    rec = sc.radiance_rays(p, camera_records(cam, c.nx, c.ny, c.spp, c.seed))
    np.save({out!r}, rec)
except rtnw.RtError as e:
    np.save({out!r}, np.array([e.code]))
    print(e)
"""


def run_child(tmp_path, name, **env):
    out = str(tmp_path / "child.npy")
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here, os.path.dirname(rtnw.__file__), os.path.dirname(O.__file__)]
    res = subprocess.run([sys.executable, "-c", CHILD.format(paths=paths, name=name, out=out, bg=BG)], check=True,
                         env=dict(os.environ, **env), timeout=120, capture_output=True, text=True)
    return np.load(out), res.stdout


def test_small_batches_return_the_same_bytes(tmp_path):
    """RTNW_RADIANCE_BATCH=100 in a fresh process: 15 full batches and a short one."""
    _, _, _, _, rays, rec = view("scan65_mixed")
    assert len(rays) > 100 and len(rays) % 100 != 0
    small, _ = run_child(tmp_path, "scan65_mixed", RTNW_RADIANCE_BATCH="100")
    assert same_records(small, rec)


def test_the_device_form_on_a_callers_stream_equals_the_host_form():
    import torch
    c, _, _, sc, rays, rec = view("prescan9")
    n = len(rays)
    stream = torch.cuda.Stream()
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_out = torch.full((n * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert d_rays.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    sc.radiance_rays_dev(qparams(c), d_rays.data_ptr(), n, d_out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert same_records(d_out.cpu().numpy().view(rtnw.RADIANCE_DTYPE), rec)


# ------------------------------------------------------------------ 3. two views in one call
def test_two_cameras_interleaved_in_one_call_each_equal_their_own_render():
    c, _, cam_a, sc, rays_a, rec_a = view("scan64_mixed")
    aspect = float(np.float32(c.nx) / np.float32(c.ny))
    cam_b = rtnw.Camera((3.5, 1.2, -6.0), (0.3, 0.7, 0.2), (0, 1, 0), 55.0, aspect, 0.2, 6.5, 0.25, 0.75)
    rays_b = camera_records(c, cam_b)
    assert (rays_b["dir"] != 0).all()
    both = np.empty(2 * len(rays_a), rtnw.PATH_RAY_DTYPE)
    both[0::2], both[1::2] = rays_a, rays_b
    rec = sc.radiance_rays(qparams(c), both)
    assert same_records(np.ascontiguousarray(rec[0::2]), rec_a)
    rgb = rec["rgb"][1::2].reshape(c.ny, c.nx, c.spp, 3)
    for s in range(c.spp):
        assert same(rgb[:, :, s], sample_render(c, sc, cam_b, s)), s
    assert not same(rec["rgb"][1::2], rec_a["rgb"])


# ------------------------------------------------------------------ 4. parameter edges
@pytest.mark.parametrize("background", ["sky", "black"])
@pytest.mark.parametrize("max_depth", [1, 0])
def test_depth_limits_and_backgrounds_follow_the_renders(max_depth, background):
    c, _, cam, sc, rays, rec = view("scan_five_kinds")
    kw = dict(max_depth=max_depth, background=BG[background])
    got = sc.radiance_rays(qparams(c, **kw), rays)
    rgb = got["rgb"].reshape(c.ny, c.nx, c.spp, 3)
    for s in range(c.spp):
        assert same(rgb[:, :, s], sample_render(c, sc, cam, s, **kw)), s
    assert (got["status"] == 0).all() and not same(got["rgb"], rec["rgb"])
    if background == "black" and max_depth == 0:    # nothing scatters and nothing but a light is seen
        assert (rgb.reshape(-1, 3)[:, 0] == 0).any()


def light_and_wall(b):
    """A white diffuse floor, a grey diffuse sphere and a light over them."""
    b.add(b.rect(G.XZ, -20, 20, -20, 20, 0.0, b.lambert(b.const(0.8, 0.8, 0.8))),
          b.sphere((-1.5, 1.0, 0.0), 1.0, b.lambert(b.const(0.5, 0.5, 0.5))),
          b.sphere((1.5, 1.0, 0.0), 0.6, b.light(b.const(4.0, 3.0, 2.0))))


def test_seed_and_skip_move_diffuse_results_and_leave_a_light_alone():
    case = G.Case(name="radiance_light_and_wall", make=light_and_wall, seed=12)
    sc = rtnw.Scene(case.builder().desc())
    n = 64
    eye = np.array([0.0, 1.5, 8.0], np.float32)
    jit = np.random.default_rng(5).uniform(-0.2, 0.2, (n, 3)).astype(np.float32)
    to_wall = np.array([-1.5, 1.0, 0.0], np.float32) + jit - eye
    to_light = np.array([1.5, 1.0, 0.0], np.float32) + jit - eye
    pix = np.arange(n, dtype=np.uint32) * 977
    p = rtnw.RenderParams(1, 1, 1, max_depth=50, background=rtnw.RT_BG_SKY, seed=9)
    wall = rtnw.pack_path_rays(eye, to_wall, 0.0, pix, 3, 5)
    light = rtnw.pack_path_rays(eye, to_light, 0.0, pix, 3, 5)
    w0, l0 = sc.radiance_rays(p, wall), sc.radiance_rays(p, light)
    assert (l0["rgb"] == np.array([4, 3, 2], np.float32)).all() and (w0["rgb"] > 0).all()
    assert len({tuple(x) for x in bits(w0["rgb"]).tolist()}) == n    # each key its own path
    # another seed: other scatter draws
    p2 = rtnw.RenderParams(1, 1, 1, max_depth=50, background=rtnw.RT_BG_SKY, seed=10)
    w_seed = sc.radiance_rays(p2, wall)
    assert (bits(w_seed["rgb"]) != bits(w0["rgb"])).any(axis=1).all()
    assert same_records(sc.radiance_rays(p2, light), l0)
    # another skip on the same (pixel, sample): the scatter draws start elsewhere in the stream
    for skip in (0, 7, rtnw.RT_RADIANCE_MAX_SKIP):
        wall["skip"] = light["skip"] = skip
        w_skip = sc.radiance_rays(p, wall)
        assert (bits(w_skip["rgb"]) != bits(w0["rgb"])).any(axis=1).all(), skip
        assert same_records(sc.radiance_rays(p, light), l0), skip
    # the first skip again: the first records
    wall["skip"] = 5
    assert same_records(sc.radiance_rays(p, wall), w0)
    sc.close()


# ------------------------------------------------------------------ 5. invalid rays
def test_invalid_rays_report_invalid_and_leave_the_others_alone():
    name = "scan64_mixed"    # moving spheres: the time span counts
    c, _, _, sc, rays, rec = view(name)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    bad = []
    for field in ("origin", "dir"):
        for value in (nan, inf, -inf):
            for comp in range(3):
                bad.append((field, comp, value))
    for value in (nan, inf, -inf, np.float32(-0.5), np.float32(1.5)):
        bad.append(("time", None, value))
    bad += [("dir", None, np.float32(0)), ("skip", None, rtnw.RT_RADIANCE_MAX_SKIP + 1), ("skip", None, 2 ** 32 - 1)]
    r = rays[:4 * len(bad)].copy()
    where = np.arange(len(bad)) * 4 + 1    # interleaved with valid rays
    for at, (field, comp, value) in zip(where, bad):
        if comp is None:
            r[field][at] = value
        else:
            r[field][at, comp] = value
    got = sc.radiance_rays(qparams(c), r)
    invalid = np.zeros(len(r), bool)
    invalid[where] = True
    assert (got["status"][invalid] == rtnw.RT_HIT_INVALID).all() and (got["status"][~invalid] == 0).all()
    assert not bits(got["rgb"][invalid]).any()    # +0, not -0
    alone = sc.radiance_rays(qparams(c), r[~invalid])
    assert same_records(np.ascontiguousarray(got[~invalid]), alone)
    assert same_records(alone, np.ascontiguousarray(rec[:len(r)][~invalid]))
    # a call of invalid rays only, and the largest legal skip among them
    only = sc.radiance_rays(qparams(c), r[invalid])
    assert (only["status"] == rtnw.RT_HIT_INVALID).all() and not bits(only["rgb"]).any()
    edge = rays[:2].copy()
    edge["skip"] = rtnw.RT_RADIANCE_MAX_SKIP
    assert (sc.radiance_rays(qparams(c), edge)["status"] == 0).all()
    # without moving spheres the time is not tested
    c3, _, _, sc3, rays3, rec3 = view("cloud1736")
    r3 = rays3[:64].copy()
    r3["time"] = np.float32(7.0)
    assert same_records(sc3.radiance_rays(qparams(c3), r3), rec3[:64])


# ------------------------------------------------------------------ 6. wide BVH
def test_a_wide_bvh_is_unsupported(tmp_path):
    code, out = run_child(tmp_path, "cloud1736", RTNW_BVH_WIDTH="4")
    assert code.tolist() == [RT_ERR_UNSUPPORTED] and "2-wide BVH" in out, (code, out)
