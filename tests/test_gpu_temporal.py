"""The reprojected frame history on the GPU: rt_temporal and rt_temporal_dev equal the numpy
statement of tests/test_temporal_spec.py bit for bit — colour, moments and len — on analytic
planes seen by two cameras, on arbitrary guides and on rendered frames; the accumulated frame
goes through the denoiser as the statement's does; and a static camera's accumulation is the
long render but for the blend's roundings.
"""
import ctypes

import numpy as np
import pytest

import rtnw
from test_denoise_spec import synthetic
from test_denoise_varfilter_spec import denoise_vf_ref
from test_gpu_denoise import mismatch, same
from test_gpu_parity import _scene, gamma_rms
from test_temporal_spec import SETTINGS, temporal_ref, two_camera_case, view, without_moments

pytestmark = pytest.mark.gpu

# both sides of the edges of a 64 x 4 block
SIZES = [(1, 1), (1, 9), (9, 1), (64, 4), (65, 5), (130, 9), (33, 40)]
F = np.float32
_arbitrary = {}


def arbitrary_case(nx, ny):
    """test_denoise_spec.synthetic's arbitrary guides for both frames, where most taps fail: (cur,
    cam, hist, prev_cam) with the two-camera case's cameras; made once and left unchanged."""
    if (nx, ny) not in _arbitrary:
        _, cam, _, prev_cam = two_camera_case(nx, ny)
        rng = np.random.default_rng(7 * nx + ny)
        frames = []
        for seed in (100 * nx + ny, 100 * nx + ny + 1):
            d = synthetic(nx, ny, seed)
            cov = np.where(d["depth"] > 0, F(1), F(0))
            cov[rng.random((ny, nx)) < 0.05] = F(0.5)
            f = dict(albedo=d["albedo"], normal=d["normal"], depth=d["depth"] * F(1.8), coverage=cov)
            frames.append(dict(color=d["color"], features=rtnw.pack_guides(f), moments=d["moments"], len=d["spp"].copy()))
        hist, cur = frames
        hist["len"][rng.random((ny, nx)) < 0.1] = 0
        del cur["len"]
        for fr in frames:
            for v in fr.values():
                v.setflags(write=False)
        _arbitrary[(nx, ny)] = (cur, cam, hist, prev_cam)
    return _arbitrary[(nx, ny)]


def arguments(inputs, nx, ny, case, moments):
    cur, cam, hist, prev_cam = (two_camera_case if inputs == "planes" else arbitrary_case)(nx, ny)
    if not moments:
        cur, hist = without_moments(cur), without_moments(hist)
    if case == "first":
        hist, prev_cam = None, None
    elif case == "equal":
        prev_cam = view(nx, ny, (0.45, 0.55, -5.9), (0.35, 0.3, 0.0))   # another object, the same bytes
        assert prev_cam is not cam and bytes(prev_cam.desc) == bytes(cam.desc)
    return cur, cam, hist, prev_cam


_want = {}


def statement(inputs, nx, ny, case, moments):
    """temporal_ref on that case, computed once."""
    key = (inputs, nx, ny, case, moments)
    if key not in _want:
        cur, cam, hist, prev_cam = arguments(*key)
        _want[key] = temporal_ref(cur, cam, hist, prev_cam, **SETTINGS)
    return _want[key]


def check(got, want, what):
    assert same(got, want), (what, mismatch(got, want))


def run(cur, cam, hist, prev_cam, **kw):
    return rtnw.temporal(cur["color"], cur["features"], cur["moments"], kw.pop("frame_spp"), cam, hist, prev_cam, **kw)


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no-moments"])
@pytest.mark.parametrize("case", ["first", "equal", "two-cameras"])
@pytest.mark.parametrize("inputs", ["planes", "arbitrary"])
@pytest.mark.parametrize("nx,ny", SIZES)
def test_temporal_equals_the_statement(nx, ny, inputs, case, moments):
    cur, cam, hist, prev_cam = arguments(inputs, nx, ny, case, moments)
    want, want_mom, want_len = statement(inputs, nx, ny, case, moments)
    assert np.isfinite(want).all()
    if case != "first" and nx * ny >= 256:   # some pixels take history and some do not
        took = int((want_len != SETTINGS["frame_spp"]).sum())
        assert 1 <= took < nx * ny, took
    got, got_mom, got_len = run(cur, cam, hist, prev_cam, **SETTINGS)
    check(got, want, "colour")
    assert got_len.dtype == np.int32 and np.array_equal(got_len, want_len), int((got_len != want_len).sum())
    if moments:
        check(got_mom, want_mom, "moments")
    else:
        assert got_mom is None and want_mom is None


def test_the_host_form_with_moments_and_no_output_moments():
    """rt_temporal itself (rtnw.temporal always asks for the moments it can have) on a history
    with moments and out->moments null, at 67 x 9, a column past a 64-wide block and a row past
    two 4-row blocks: colour and len equal the statement bit for bit."""
    nx, ny = 67, 9
    cur, cam, hist, prev_cam = arguments("planes", nx, ny, "two-cameras", True)
    want, _, want_len = statement("planes", nx, ny, "two-cameras", True)
    keep = [np.ascontiguousarray(fr[k], t) for fr in (cur, hist) for k, t in (("color", F), ("features", F), ("moments", F))]
    keep.append(np.ascontiguousarray(hist["len"], np.int32))
    out, out_len = np.zeros((ny, nx, 3), F), np.zeros((ny, nx), np.int32)
    ptr = [a.ctypes.data for a in keep]
    fcur, fhist = rtnw.RtTemporalFrame(*ptr[0:3], None), rtnw.RtTemporalFrame(*ptr[3:7])
    fout = rtnw.RtTemporalFrame(out.ctypes.data, None, None, out_len.ctypes.data)
    tp = rtnw.temporal_params(**SETTINGS)
    rtnw._check(rtnw.lib().rt_temporal(0, nx, ny, ctypes.byref(fcur), ctypes.byref(cam.desc), ctypes.byref(fhist),
                                       ctypes.byref(prev_cam.desc), ctypes.byref(tp), ctypes.byref(fout), None))
    check(out, want, "colour")
    assert np.array_equal(out_len, want_len), int((out_len != want_len).sum())


class DeviceArrays:
    """Device copies of host arrays in one allocation (16-B aligned each), freed on exit."""

    def __init__(self, arrays):
        self.L = rtnw.lib()
        self.host = [np.ascontiguousarray(a) for a in arrays]
        sizes = [(a.nbytes + 255) // 256 * 256 for a in self.host]
        self.dev = ctypes.c_void_p()
        rtnw._check(self.L.rt_device_alloc(0, sum(sizes), ctypes.byref(self.dev)))
        self.ptr, off = [], 0
        for a, n in zip(self.host, sizes):
            self.ptr.append(self.dev.value + off)
            rtnw._check(self.L.rt_copy_to_device(ctypes.c_void_p(self.dev.value + off), a.ctypes.data, a.nbytes))
            off += n

    def read(self, k):
        out = np.zeros_like(self.host[k])
        rtnw._check(self.L.rt_copy_to_host(out.ctypes.data, ctypes.c_void_p(self.ptr[k]), out.nbytes))
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.L.rt_device_free(self.dev)


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no-moments"])
def test_device_entry_point_equals_the_host_one_over_a_chain_of_three_calls(moments):
    """A first frame, a camera step and a frame at the camera's rest, on device buffers with two
    history sets that ping-pong: every call's output equals the host form's."""
    nx, ny = 130, 9
    cur, cam, hist0, prev_cam = two_camera_case(nx, ny)
    rest = view(nx, ny, (0.45, 0.55, -5.9), (0.35, 0.3, 0.0))
    frames = [dict(hist0, color=hist0["color"][::-1].copy()), cur, dict(cur, color=cur["color"][:, ::-1].copy())]
    if not moments:
        frames = [without_moments(f) for f in frames]
    cams = [prev_cam, cam, rest]
    kw = dict(SETTINGS, max_history=6)       # the third call meets the cap
    tp = rtnw.temporal_params(**kw)
    host, h = [], None
    for k in range(3):
        c, m, ln = run(frames[k], cams[k], h, cams[k - 1] if k else None, **kw)
        host.append((c, m, ln))
        h = dict(color=c, moments=m, len=ln, features=frames[k]["features"])
    assert (host[2][2] == 10).any() and (host[1][2] == 8).any() and (host[2][2] == 4).sum() < (host[1][2] == 4).sum()
    zc, zm, zl = np.zeros((ny, nx, 3), F), np.zeros((ny, nx, 2), F), np.zeros((ny, nx), np.int32)
    arrays = []
    for f in frames:     # 0..8: colour, guides, moments of the three frames
        arrays += [f["color"], f["features"], f["moments"] if moments else zm]
    arrays += [zc, zm, zl, zc, zm, zl]       # 9..14: the two history sets
    L = rtnw.lib()
    with DeviceArrays(arrays) as d:
        def frame(k):
            return rtnw.RtTemporalFrame(d.ptr[3 * k], d.ptr[3 * k + 1], d.ptr[3 * k + 2] if moments else None, None)

        def history(s, k):   # set s holds the output of the call on frame k
            return rtnw.RtTemporalFrame(d.ptr[9 + 3 * s], d.ptr[3 * k + 1] if k is not None else None,
                                        d.ptr[10 + 3 * s] if moments else None, d.ptr[11 + 3 * s])
        for k in range(3):
            c, o = frame(k), history(k & 1, None)
            hs = history((k - 1) & 1, k - 1) if k else None
            rtnw._check(L.rt_temporal_dev(0, nx, ny, ctypes.byref(c), ctypes.byref(cams[k].desc),
                                          ctypes.byref(hs) if hs else None, ctypes.byref(cams[k - 1].desc) if k else None,
                                          ctypes.byref(tp), ctypes.byref(o), None))
            s = 9 + 3 * (k & 1)
            check(d.read(s), host[k][0], f"colour of call {k}")
            assert np.array_equal(d.read(s + 2), host[k][2]), k
            if moments:
                check(d.read(s + 1), host[k][1], f"moments of call {k}")
        for k in range(3):   # the inputs were only read
            check(d.read(3 * k), frames[k]["color"], "input colour")


# ------------------------------------------------------------------ rendered frames
NX, NY, SPP, SEED = 48, 32, 4, 23
_rendered = {}


def rendered():
    """random_scene 48 x 32: two frames of 4 spp (samples 0..3, 4..7) from two cameras a small
    step apart, with moments and features, and the second frame at 512 spp with another seed;
    rendered once."""
    if not _rendered:
        _, bg, depth = rtnw.SCENE_DEFAULTS["random_scene"]
        sc = _scene("random_scene")
        aspect = float(F(NX) / F(NY))
        cams = [rtnw.Camera(lf, (0, 0, 0), (0, 1, 0), 20.0, aspect, 0.1, 10.0) for lf in ((13, 2, 3), (13.0, 2.1, 3.25))]
        frames = []
        for k, cam in enumerate(cams):
            p = rtnw.RenderParams(NX, NY, SPP, max_depth=depth, background=bg, seed=SEED, chunk=1, sample_offset=k * SPP)
            color, mom = sc.render_tile_moments(cam, p, 0, 0, NX, NY)
            f = sc.render_features(cam, p, 0, 0, NX, NY)
            for v in (color, mom, *f.values()):
                v.setflags(write=False)
            frames.append(dict(color=color, features=f, moments=mom))
        pr = rtnw.RenderParams(NX, NY, 512, max_depth=depth, background=bg, seed=977, chunk=1)
        ref = sc.render_tile(cams[1], pr, 0, 0, NX, NY)
        ref.setflags(write=False)
        _rendered.update(cams=cams, frames=frames, ref=ref)
    return _rendered


RENDERED = dict(frame_spp=SPP, max_history=32, cos_normal=0.9, sigma_depth=0.1)


def test_on_rendered_frames_the_accumulation_equals_the_statement_and_feeds_the_denoiser():
    """rtnw.temporal on two rendered frames equals temporal_ref bit for bit, and
    rtnw.denoise of it, its len as the spp map and the variance pre-filter on, equals
    denoise_vf_ref of the statement's.  Prints the gamma RMS of the second frame against 512 spp
    with another seed: raw, accumulated, accumulated then denoised.  Not asserted: an MI355X
    printed 0.0920, 0.0665 and 0.0809 with 75 % of the pixels finding a history (DESIGN.md §7h has
    the figures over a longer camera move, and why the filter costs on this scene)."""
    r = rendered()
    cams, (f0, f1), ref = r["cams"], r["frames"], r["ref"]
    c0, m0, l0 = run(f0, cams[0], None, None, **RENDERED)
    check(c0, f0["color"], "first frame")
    check(m0, f0["moments"], "first frame's moments")
    assert (l0 == SPP).all()
    hist = dict(color=c0, moments=m0, len=l0, features=f0["features"])
    got, got_mom, got_len = run(f1, cams[1], hist, cams[0], **RENDERED)
    want, want_mom, want_len = temporal_ref(f1, cams[1], hist, cams[0], **RENDERED)
    check(got, want, "colour")
    check(got_mom, want_mom, "moments")
    assert np.array_equal(got_len, want_len)
    share = float((got_len == 2 * SPP).mean())
    assert set(np.unique(got_len)) == {SPP, 2 * SPP} and 0.25 < share < 1, share
    kw = dict(rtnw.DENOISE_DEFAULTS)
    f = f1["features"]
    den = rtnw.denoise(got, f, got_mom, got_len, variance_filter=1, **kw)
    want_den = denoise_vf_ref(want, f["albedo"], f["normal"], f["depth"], want_mom, want_len, variance_filter=1, **kw)
    check(den, want_den, "accumulated then denoised")
    rms = [float(gamma_rms(img, ref).mean()) for img in (f1["color"], got, den)]
    print(f"random_scene {NX}x{NY}, {SPP} spp a frame, {share:.3f} of the pixels with history: gamma RMS against 512 spp "
          f"{rms[0]:.4f} raw -> {rms[1]:.4f} accumulated -> {rms[2]:.4f} accumulated, then denoised")


def test_a_static_camera_accumulates_to_the_long_render():
    """Four frames of 4 spp at sample_offset 0, 4, 8, 12, equal cameras, max_history 16: out.len is
    16 everywhere and the colour is render_tile(spp=16) within 80 * 2^-24 of that render's value.

    The bound, from the roundings the statement performs (u = 2^-24, radiance non-negative, L
    the long render's mean, every sample sum below in any order of adding):
      * a frame mean is a sum of 4 non-negative samples (relative error at most 3u) times 1/4
        (exact), and at most 4 L, a frame holding at most all of the 16 samples' radiance: each
        frame mean is within 12 u L of its exact value, and so is their average;
      * a blend c + (f - c) * a rounds four times — the subtraction, a = float(4) / float(n) (exact
        for n = 8 and 16, one rounding for n = 12), the product, the sum — each on a value of at
        most 4 L: at most 16 u L a blend, and an earlier error passes through a later blend
        multiplied by 1 - a < 1.  Three blends (the first frame is copied): 48 u L;
      * in exact arithmetic the running mean with a = 4 / n is the mean of the 16 samples;
      * the long render adds 16 non-negative samples (relative error at most 15u) and multiplies
        by 1/16 (exact): within 15 u L.
    Together 75 u L; 80 leaves room for the second-order terms and for L itself being rounded."""
    _, bg, depth = rtnw.SCENE_DEFAULTS["random_scene"]
    sc, cam = _scene("random_scene"), rendered()["cams"][0]
    hist = None
    for k in range(4):
        p = rtnw.RenderParams(NX, NY, SPP, max_depth=depth, background=bg, seed=SEED, chunk=1, sample_offset=k * SPP)
        color, mom = (rendered()["frames"][0][n] for n in ("color", "moments")) if k == 0 else \
            sc.render_tile_moments(cam, p, 0, 0, NX, NY)
        f = sc.render_features(cam, p, 0, 0, NX, NY)
        c, m, ln = rtnw.temporal(color, f, mom, SPP, cam, hist, cam if hist else None, max_history=16)
        assert (ln == SPP * (k + 1)).all(), k
        hist = dict(color=c, moments=m, len=ln, features=f)
    p = rtnw.RenderParams(NX, NY, 4 * SPP, max_depth=depth, background=bg, seed=SEED, chunk=1)
    long, long_mom = sc.render_tile_moments(cam, p, 0, 0, NX, NY)
    assert (long >= 0).all() and (ln == 16).all()
    err = np.abs(c.astype(np.float64) - long.astype(np.float64))
    bound = 80 * 2.0 ** -24 * long.astype(np.float64)
    worst = float((err / np.maximum(long, 1e-30)).max() / 2.0 ** -24)
    print(f"static camera, 4 x {SPP} spp against 16 spp: largest error {worst:.2f} u L (bound 80)")
    assert (err <= bound).all(), worst
    # the moments likewise: y and y * y are non-negative, a frame's sums are at most the long render's, the
    # divisions by float(4) and the last product with float(16) are exact, so the same steps give the same bound
    assert (long_mom >= 0).all()
    assert (np.abs(m.astype(np.float64) - long_mom.astype(np.float64)) <= 80 * 2.0 ** -24 * long_mom.astype(np.float64)).all()
