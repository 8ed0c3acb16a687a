"""The frame history for background and edge pixels on the GPU: rt_temporal_cover and
rt_temporal_cover_dev equal the numpy statement of tests/test_temporal_cover_spec.py bit for bit —
colour, moments, len, the mask of clipped channels and the source of every pixel's history — on
analytic planes under a band of misses with partly covered pixels, on arbitrary guides and on
rendered frames; with its settings zeroed, on a first frame and under equal cameras they equal
rt_temporal_clamped's and rt_temporal's own output; and the accumulated frame goes through the
denoiser as the statement's does.
"""
import ctypes

import numpy as np
import pytest

import rtnw
from test_denoise_varfilter_spec import denoise_vf_ref
from test_gpu_parity import _scene
from test_gpu_temporal import DeviceArrays, arbitrary_case, check
from test_gpu_temporal_clamp import SIZES
from test_temporal_clamp_spec import GAMMA
from test_temporal_cover_spec import COVER, SRC_BACKGROUND, SRC_EDGE, SRC_NONE, SRC_SAME, SRC_SURFACE, cover_case, temporal_cover_ref
from test_temporal_spec import SETTINGS, flat, two_camera_case, view, without_moments

pytestmark = pytest.mark.gpu
F = np.float32


def arguments(inputs, nx, ny, moments):
    cur, cam, hist, prev_cam = (cover_case if inputs == "cover" else arbitrary_case)(nx, ny)
    if not moments:
        cur, hist = without_moments(cur), without_moments(hist)
    return cur, cam, hist, prev_cam


def run(cur, cam, hist, prev_cam, *, entry="cover", **kw):
    fn = {"cover": rtnw.temporal_cover, "clamped": rtnw.temporal_clamped, "plain": rtnw.temporal}[entry]
    return fn(cur["color"], cur["features"], cur["moments"], kw.pop("frame_spp"), cam, hist, prev_cam, **kw)


def compare(got, want, moments):
    """Colour, moments, len, and as far as `want` goes, clipped and source."""
    check(got[0], want[0], "colour")
    assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2]), int((got[2] != want[2]).sum())
    if moments:
        check(got[1], want[1], "moments")
    else:
        assert got[1] is None and want[1] is None
    for k, what in ((3, "clipped"), (4, "source")):
        if len(want) > k:
            assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, int((got[k] != want[k]).sum()))


_want = {}


def statement(inputs, nx, ny, moments, **kw):
    """temporal_cover_ref on that case and those settings, computed once."""
    key = (inputs, nx, ny, moments, tuple(sorted(kw.items())))
    if key not in _want:
        _want[key] = temporal_cover_ref(*arguments(inputs, nx, ny, moments), **kw)
    return _want[key]


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no-moments"])
@pytest.mark.parametrize("radius", [0, 2])
@pytest.mark.parametrize("background,edges", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("inputs", ["cover", "arbitrary"])
@pytest.mark.parametrize("nx,ny", SIZES)
def test_cover_equals_the_statement(nx, ny, inputs, background, edges, radius, moments):
    cur, cam, hist, prev_cam = arguments(inputs, nx, ny, moments)
    kw = dict(SETTINGS, radius=radius, gamma=GAMMA, background=background, edges=edges, sigma_coverage=0.25)
    want = statement(inputs, nx, ny, moments, **kw)
    assert np.isfinite(want[0]).all()
    if inputs == "cover" and nx * ny >= 256:   # every class the settings allow is met, and some pixels find nothing
        met = set(np.unique(want[4]))
        allowed = {SRC_NONE, SRC_SURFACE} | ({SRC_BACKGROUND} if background else set()) | \
                  ({SRC_SURFACE | SRC_EDGE} if edges else set()) | ({SRC_BACKGROUND | SRC_EDGE} if background and edges else set())
        assert met == allowed, (met, allowed)
        assert radius == 0 or (1 <= int((want[3] != 0).sum()) < int((want[4] != 0).sum()))
    compare(run(cur, cam, hist, prev_cam, **kw), want, moments)


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no-moments"])
@pytest.mark.parametrize("radius", [0, 2])
@pytest.mark.parametrize("inputs", ["cover", "arbitrary"])
@pytest.mark.parametrize("nx,ny", [(67, 9), (33, 40)])
def test_zeroed_settings_are_rt_temporal_clampeds_output(nx, ny, inputs, radius, moments):
    cur, cam, hist, prev_cam = arguments(inputs, nx, ny, moments)
    kw = dict(SETTINGS, radius=radius, gamma=GAMMA)
    want = run(cur, cam, hist, prev_cam, entry="clamped", **kw)
    for sigma in (0.0, 0.25):
        got = run(cur, cam, hist, prev_cam, background=0, edges=0, sigma_coverage=sigma, **kw)
        compare(got, want, moments)
        took = got[2] != SETTINGS["frame_spp"]
        assert took.any() and np.array_equal(got[4], np.where(took, SRC_SURFACE, SRC_NONE))


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no-moments"])
@pytest.mark.parametrize("nx,ny", [(67, 9), (33, 40)])
def test_a_first_frame_and_equal_cameras_are_rt_temporals_output(nx, ny, moments):
    cur, cam, hist, _ = arguments("cover", nx, ny, moments)
    same = view(nx, ny, (0.45, 0.55, -5.9), (0.35, 0.3, 0.0))
    assert same is not cam and bytes(same.desc) == bytes(cam.desc)
    kw = dict(SETTINGS, radius=3, gamma=0.0, **COVER)
    got = run(cur, cam, None, None, **kw)
    compare(got, run(cur, cam, None, None, entry="plain", **SETTINGS), moments)
    assert not got[3].any() and not got[4].any()
    got = run(cur, cam, hist, same, **kw)
    compare(got, run(cur, cam, hist, same, entry="plain", **SETTINGS), moments)
    took = np.minimum(hist["len"], SETTINGS["max_history"]) > 0
    assert not got[3].any() and took.any() and not took.all()
    assert np.array_equal(got[4], np.where(took, SRC_SAME, SRC_NONE))
    compare(got, temporal_cover_ref(cur, cam, hist, same, **kw), moments)


def test_the_host_form_without_mask_source_output_moments_and_time():
    """rt_temporal_cover itself with clipped, source, out->moments and ms null, on a history with
    moments at 67 x 9: colour and len equal the statement bit for bit."""
    nx, ny = 67, 9
    cur, cam, hist, prev_cam = arguments("cover", nx, ny, True)
    kw = dict(SETTINGS, radius=3, gamma=GAMMA, **COVER)
    want = statement("cover", nx, ny, True, **kw)
    keep = [np.ascontiguousarray(fr[k], t) for fr in (cur, hist) for k, t in (("color", F), ("features", F), ("moments", F))]
    keep.append(np.ascontiguousarray(hist["len"], np.int32))
    out, out_len = np.zeros((ny, nx, 3), F), np.zeros((ny, nx), np.int32)
    ptr = [a.ctypes.data for a in keep]
    fcur, fhist = rtnw.RtTemporalFrame(*ptr[0:3], None), rtnw.RtTemporalFrame(*ptr[3:7])
    fout = rtnw.RtTemporalFrame(out.ctypes.data, None, None, out_len.ctypes.data)
    tp, cp, vp = rtnw.temporal_params(**SETTINGS), rtnw.temporal_clamp_params(3, GAMMA), rtnw.temporal_cover_params(**COVER)
    rtnw._check(rtnw.lib().rt_temporal_cover(0, nx, ny, ctypes.byref(fcur), ctypes.byref(cam.desc), ctypes.byref(fhist),
                                             ctypes.byref(prev_cam.desc), ctypes.byref(tp), ctypes.byref(cp), ctypes.byref(vp),
                                             ctypes.byref(fout), None, None, None))
    check(out, want[0], "colour")
    assert np.array_equal(out_len, want[2]), int((out_len != want[2]).sum())


@pytest.mark.parametrize("source", [True, False], ids=["source", "no-source"])
@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no-moments"])
def test_device_entry_point_equals_the_host_one_and_the_statement_over_a_chain_of_three_calls(moments, source):
    """A first frame, a camera step (both classes, clamped) and a frame at the camera's rest (equal
    cameras), on device buffers with two history sets that ping-pong, one mask and one source
    buffer full of sevens before the first call, or source_dev null (the sevens then stay): every
    call's output equals the host form's and the statement's, and the inputs are only read."""
    nx, ny = 130, 9
    cur, cam, hist0, prev_cam = cover_case(nx, ny)
    rest = view(nx, ny, (0.45, 0.55, -5.9), (0.35, 0.3, 0.0))
    frames = [dict(hist0, color=hist0["color"][::-1].copy()), cur, dict(cur, color=cur["color"][:, ::-1].copy())]
    if not moments:
        frames = [without_moments(f) for f in frames]
    cams = [prev_cam, cam, rest]
    kw = dict(SETTINGS, max_history=6, radius=2, gamma=GAMMA, **COVER)       # the third call meets the cap
    tp, cp = rtnw.temporal_params(**SETTINGS | dict(max_history=6)), rtnw.temporal_clamp_params(2, GAMMA)
    vp = rtnw.temporal_cover_params(**COVER)
    host, h = [], None
    for k in range(3):
        res = run(frames[k], cams[k], h, cams[k - 1] if k else None, **kw)
        compare(res, temporal_cover_ref(frames[k], cams[k], h, cams[k - 1] if k else None, **kw), moments)
        host.append(res)
        h = dict(color=res[0], moments=res[1], len=res[2], features=frames[k]["features"])
    assert host[1][3].any() and not host[0][3].any() and not host[2][3].any()
    assert not host[0][4].any() and {1, 2, 5, 6} <= set(np.unique(host[1][4])) and set(np.unique(host[2][4])) == {SRC_SAME}
    assert (host[2][2] == 10).any() and (host[1][2] == 8).any()
    zc, zm, zl = np.zeros((ny, nx, 3), F), np.zeros((ny, nx, 2), F), np.zeros((ny, nx), np.int32)
    arrays = []
    for f in frames:     # 0..8: colour, guides, moments of the three frames
        arrays += [f["color"], f["features"], f["moments"] if moments else zm]
    arrays += [zc, zm, zl, zc, zm, zl, zl + 7, zl + 7]   # 9..14: the two history sets; 15: the mask; 16: the source
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
            rtnw._check(L.rt_temporal_cover_dev(0, nx, ny, ctypes.byref(c), ctypes.byref(cams[k].desc),
                                                ctypes.byref(hs) if hs else None,
                                                ctypes.byref(cams[k - 1].desc) if k else None, ctypes.byref(tp),
                                                ctypes.byref(cp), ctypes.byref(vp), ctypes.byref(o), ctypes.c_void_p(d.ptr[15]),
                                                ctypes.c_void_p(d.ptr[16]) if source else None, None))
            s = 9 + 3 * (k & 1)
            check(d.read(s), host[k][0], f"colour of call {k}")
            assert np.array_equal(d.read(s + 2), host[k][2]), k
            assert np.array_equal(d.read(15), host[k][3]), k
            assert np.array_equal(d.read(16), host[k][4] if source else zl + 7), k
            if moments:
                check(d.read(s + 1), host[k][1], f"moments of call {k}")
        for k in range(3):   # the inputs were only read
            check(d.read(3 * k), frames[k]["color"], "input colour")
            check(d.read(3 * k + 1), rtnw.pack_guides(frames[k]["features"]), "input guides")


def test_a_frame_taller_than_the_grid_walks_its_row_blocks():
    """2 x 262150: 65538 blocks of 4 rows against a grid capped at 65535, so three blocks go round
    the row loop a second time, reload the tile behind its barrier and work on rows 262140 and
    beyond.  The planes from two cameras a small step apart in height, the top third misses, a
    sprinkle of partly covered pixels at the bottom; radius 3."""
    nx, ny = 2, 262150
    prev_cam, cam = view(nx, ny, (0.0, 0.5, -6.0), (0.0, 0.3, 0.0)), view(nx, ny, (0.0, 0.501, -6.0), (0.0, 0.301, 0.0))
    rng = np.random.default_rng(33)

    def frame(seed, c):
        fr = flat(nx, ny, seed, c)
        g = fr["features"]
        g[:ny // 3] = np.array([1, 1, 1, 0, 0, 0, 0, 0], F)
        scale = np.where((g[..., 3] == F(1)) & (rng.random((ny, nx)) < 0.2), rng.choice(np.array([0.25, 0.5, 0.75], F), (ny, nx)),
                         F(1)).astype(F)
        g[..., 3:8] = g[..., 3:8] * scale[..., None]
        return fr
    cur = frame(21, cam)
    hist = dict(frame(22, prev_cam), len=np.full((ny, nx), 8, np.int32))
    kw = dict(SETTINGS, radius=3, gamma=GAMMA, **COVER)
    want = temporal_cover_ref(cur, cam, hist, prev_cam, **kw)
    second = slice(65535 * 4, ny)
    assert (want[2][second] == 12).any() and (want[3][second] != 0).any() and (want[3][second] == 0).any()
    assert {1, 5} <= set(np.unique(want[4][second])) and {0, 1, 2, 5, 6} <= set(np.unique(want[4]))
    compare(run(cur, cam, hist, prev_cam, **kw), want, True)


# ------------------------------------------------------------------ rendered frames
NX, NY, SPP, SEED = 48, 32, 4, 23


def test_on_rendered_frames_the_cover_accumulation_equals_the_statement_and_feeds_the_denoiser():
    """random_scene 48 x 32, two frames of 4 spp (samples 0..3, 4..7) from two cameras a small
    step apart (test_gpu_temporal_clamp's recipe): rtnw.temporal_cover of the second frame on the
    first equals temporal_cover_ref bit for bit, more pixels take a history than under
    rtnw.temporal, and rtnw.denoise of the result, its len as the spp map and the variance
    pre-filter on, equals denoise_vf_ref of the statement's."""
    _, bg, depth = rtnw.SCENE_DEFAULTS["random_scene"]
    sc = _scene("random_scene")
    aspect = float(F(NX) / F(NY))
    cams = [rtnw.Camera(lf, (0, 0, 0), (0, 1, 0), 20.0, aspect, 0.1, 10.0) for lf in ((13, 2, 3), (13.0, 2.1, 3.25))]
    frames = []
    for k, cam in enumerate(cams):
        p = rtnw.RenderParams(NX, NY, SPP, max_depth=depth, background=bg, seed=SEED, chunk=1, sample_offset=k * SPP)
        color, mom = sc.render_tile_moments(cam, p, 0, 0, NX, NY)
        frames.append(dict(color=color, features=sc.render_features(cam, p, 0, 0, NX, NY), moments=mom))
    f0, f1 = frames
    base = dict(frame_spp=SPP, max_history=32, cos_normal=0.9, sigma_depth=0.1)
    kw = dict(base, radius=1, gamma=GAMMA, **COVER)
    c0, m0, l0, k0, s0 = run(f0, cams[0], None, None, **kw)
    check(c0, f0["color"], "first frame")
    assert (l0 == SPP).all() and not k0.any() and not s0.any()
    hist = dict(color=c0, moments=m0, len=l0, features=f0["features"])
    got = run(f1, cams[1], hist, cams[0], **kw)
    want = temporal_cover_ref(f1, cams[1], hist, cams[0], **kw)
    compare(got, want, True)
    plain = run(f1, cams[1], hist, cams[0], entry="plain", **base)
    took, before = got[2] != SPP, plain[2] != SPP
    counts = {int(v): int((got[4] == v).sum()) for v in np.unique(got[4])}
    print(f"random_scene {NX}x{NY}, {SPP} spp a frame: {int(before.sum())} pixels with history under rt_temporal, "
          f"{int(took.sum())} under cover; pixels per source value {counts}; the clamp moved {int((got[3] != 0).sum())}")
    assert (took | ~before).all() and took.sum() > before.sum()
    assert (got[4] == SRC_BACKGROUND).any() and np.array_equal(took, got[4] != 0)
    dn = dict(rtnw.DENOISE_DEFAULTS)
    f = f1["features"]
    den = rtnw.denoise(got[0], f, got[1], got[2], variance_filter=1, **dn)
    want_den = denoise_vf_ref(want[0], f["albedo"], f["normal"], f["depth"], want[1], want[2], variance_filter=1, **dn)
    check(den, want_den, "covered, accumulated, then denoised")
