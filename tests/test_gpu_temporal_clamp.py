"""The clamped frame history on the GPU: rt_temporal_clamped and rt_temporal_clamped_dev equal the
numpy statement of tests/test_temporal_clamp_spec.py bit for bit — colour, moments, len and the
mask of clipped channels — on analytic planes seen by two cameras, on arbitrary guides and on
rendered frames; where nothing is clamped they equal rt_temporal's own output; and the clamped
frame goes through the denoiser as the statement's does.
"""
import ctypes

import numpy as np
import pytest

import rtnw
from test_denoise_varfilter_spec import denoise_vf_ref
from test_gpu_parity import _scene
from test_gpu_temporal import DeviceArrays, arbitrary_case, check
from test_temporal_clamp_spec import GAMMA, temporal_clamped_ref
from test_temporal_spec import SETTINGS, flat, two_camera_case, view, without_moments

pytestmark = pytest.mark.gpu

# images smaller than the window; both sides of the edges of a 64 x 4 block, the halo of 130 x 9
# crossing three blocks; several blocks of rows
SIZES = [(1, 1), (1, 9), (9, 1), (3, 2), (64, 4), (65, 5), (67, 9), (130, 9), (33, 40)]
F = np.float32


def arguments(inputs, nx, ny, moments):
    cur, cam, hist, prev_cam = (two_camera_case if inputs == "planes" else arbitrary_case)(nx, ny)
    if not moments:
        cur, hist = without_moments(cur), without_moments(hist)
    return cur, cam, hist, prev_cam


def run(cur, cam, hist, prev_cam, *, clamped=True, **kw):
    fn = rtnw.temporal_clamped if clamped else rtnw.temporal
    return fn(cur["color"], cur["features"], cur["moments"], kw.pop("frame_spp"), cam, hist, prev_cam, **kw)


def compare(got, want, moments):
    check(got[0], want[0], "colour")
    assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2]), int((got[2] != want[2]).sum())
    if moments:
        check(got[1], want[1], "moments")
    else:
        assert got[1] is None and want[1] is None
    if len(want) > 3:
        assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3]), int((got[3] != want[3]).sum())


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no-moments"])
@pytest.mark.parametrize("gamma", [GAMMA, 0.0])
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("inputs", ["planes", "arbitrary"])
@pytest.mark.parametrize("nx,ny", SIZES)
def test_clamped_equals_the_statement(nx, ny, inputs, radius, gamma, moments):
    cur, cam, hist, prev_cam = arguments(inputs, nx, ny, moments)
    kw = dict(SETTINGS, radius=radius, gamma=gamma)
    want = temporal_clamped_ref(cur, cam, hist, prev_cam, **kw)
    assert np.isfinite(want[0]).all()
    if inputs == "planes" and gamma > 0 and nx * ny >= 256:   # the clamp binds on some pixels and not on others
        assert 1 <= int((want[3] != 0).sum()) < int((want[2] != SETTINGS["frame_spp"]).sum())
    compare(run(cur, cam, hist, prev_cam, **kw), want, moments)


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no-moments"])
@pytest.mark.parametrize("nx,ny", [(67, 9), (33, 40)])
def test_where_nothing_is_clamped_the_output_is_rt_temporals(nx, ny, moments):
    """Radius 0 under two cameras, equal cameras at radius 3 and a first frame at radius 3: the
    unclamped entry point's output bit for bit, and a mask of zeros."""
    cur, cam, hist, prev_cam = arguments("planes", nx, ny, moments)
    same = view(nx, ny, (0.45, 0.55, -5.9), (0.35, 0.3, 0.0))
    assert same is not cam and bytes(same.desc) == bytes(cam.desc)
    for h, pc, radius in ((hist, prev_cam, 0), (hist, same, 3), (None, None, 3)):
        want = run(cur, cam, h, pc, clamped=False, **SETTINGS)
        got = run(cur, cam, h, pc, radius=radius, gamma=0.0, **SETTINGS)
        compare(got, want, moments)
        assert not got[3].any()


def test_the_host_form_without_a_mask_and_without_output_moments():
    """rt_temporal_clamped itself with clipped, out->moments and ms null, on a history with
    moments at 67 x 9: colour and len equal the statement bit for bit."""
    nx, ny = 67, 9
    cur, cam, hist, prev_cam = arguments("planes", nx, ny, True)
    kw = dict(SETTINGS, radius=3, gamma=GAMMA)
    want, _, want_len, _ = temporal_clamped_ref(cur, cam, hist, prev_cam, **kw)
    keep = [np.ascontiguousarray(fr[k], t) for fr in (cur, hist) for k, t in (("color", F), ("features", F), ("moments", F))]
    keep.append(np.ascontiguousarray(hist["len"], np.int32))
    out, out_len = np.zeros((ny, nx, 3), F), np.zeros((ny, nx), np.int32)
    ptr = [a.ctypes.data for a in keep]
    fcur, fhist = rtnw.RtTemporalFrame(*ptr[0:3], None), rtnw.RtTemporalFrame(*ptr[3:7])
    fout = rtnw.RtTemporalFrame(out.ctypes.data, None, None, out_len.ctypes.data)
    tp, cp = rtnw.temporal_params(**SETTINGS), rtnw.temporal_clamp_params(3, GAMMA)
    rtnw._check(rtnw.lib().rt_temporal_clamped(0, nx, ny, ctypes.byref(fcur), ctypes.byref(cam.desc), ctypes.byref(fhist),
                                               ctypes.byref(prev_cam.desc), ctypes.byref(tp), ctypes.byref(cp),
                                               ctypes.byref(fout), None, None))
    check(out, want, "colour")
    assert np.array_equal(out_len, want_len), int((out_len != want_len).sum())


@pytest.mark.parametrize("mask", [True, False], ids=["mask", "no-mask"])
@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no-moments"])
def test_device_entry_point_equals_the_host_one_and_the_statement_over_a_chain_of_three_calls(moments, mask):
    """A first frame, a camera step (clamped) and a frame at the camera's rest (equal cameras: not
    clamped), on device buffers with two history sets that ping-pong and one mask, full of sevens
    before the first call, or clipped_dev null (the sevens then stay): every call's output equals
    the host form's and the statement's."""
    nx, ny = 130, 9
    cur, cam, hist0, prev_cam = two_camera_case(nx, ny)
    rest = view(nx, ny, (0.45, 0.55, -5.9), (0.35, 0.3, 0.0))
    frames = [dict(hist0, color=hist0["color"][::-1].copy()), cur, dict(cur, color=cur["color"][:, ::-1].copy())]
    if not moments:
        frames = [without_moments(f) for f in frames]
    cams = [prev_cam, cam, rest]
    kw = dict(SETTINGS, max_history=6, radius=2, gamma=GAMMA)       # the third call meets the cap
    tp, cp = rtnw.temporal_params(**SETTINGS | dict(max_history=6)), rtnw.temporal_clamp_params(2, GAMMA)
    host, h = [], None
    for k in range(3):
        res = run(frames[k], cams[k], h, cams[k - 1] if k else None, **kw)
        compare(res, temporal_clamped_ref(frames[k], cams[k], h, cams[k - 1] if k else None, **kw), moments)
        host.append(res)
        h = dict(color=res[0], moments=res[1], len=res[2], features=frames[k]["features"])
    assert host[1][3].any() and not host[0][3].any() and not host[2][3].any()
    assert (host[2][2] == 10).any() and (host[1][2] == 8).any()
    zc, zm, zl = np.zeros((ny, nx, 3), F), np.zeros((ny, nx, 2), F), np.zeros((ny, nx), np.int32)
    arrays = []
    for f in frames:     # 0..8: colour, guides, moments of the three frames
        arrays += [f["color"], f["features"], f["moments"] if moments else zm]
    arrays += [zc, zm, zl, zc, zm, zl, zl + 7]   # 9..14: the two history sets; 15: the mask
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
            rtnw._check(L.rt_temporal_clamped_dev(0, nx, ny, ctypes.byref(c), ctypes.byref(cams[k].desc),
                                                  ctypes.byref(hs) if hs else None,
                                                  ctypes.byref(cams[k - 1].desc) if k else None, ctypes.byref(tp),
                                                  ctypes.byref(cp), ctypes.byref(o),
                                                  ctypes.c_void_p(d.ptr[15]) if mask else None, None))
            s = 9 + 3 * (k & 1)
            check(d.read(s), host[k][0], f"colour of call {k}")
            assert np.array_equal(d.read(s + 2), host[k][2]), k
            assert np.array_equal(d.read(15), host[k][3] if mask else zl + 7), k
            if moments:
                check(d.read(s + 1), host[k][1], f"moments of call {k}")
        for k in range(3):   # the inputs were only read
            check(d.read(3 * k), frames[k]["color"], "input colour")


def test_a_frame_taller_than_the_grid_walks_its_row_blocks():
    """2 x 262150: 65538 blocks of 4 rows against a grid capped at 65535, so three blocks go round
    the row loop a second time, reload the tile behind its barrier and work on rows 262140 and
    beyond.  The planes from two cameras a small step apart in height; radius 3."""
    nx, ny = 2, 262150
    prev_cam, cam = view(nx, ny, (0.0, 0.5, -6.0), (0.0, 0.3, 0.0)), view(nx, ny, (0.0, 0.501, -6.0), (0.0, 0.301, 0.0))
    cur = flat(nx, ny, 21, cam)
    hist = dict(flat(nx, ny, 22, prev_cam), len=np.full((ny, nx), 8, np.int32))
    kw = dict(SETTINGS, radius=3, gamma=GAMMA)
    want = temporal_clamped_ref(cur, cam, hist, prev_cam, **kw)
    second = slice(65535 * 4, ny)
    assert (want[2][second] == 12).all() and (want[3][second] != 0).any() and (want[3][second] == 0).any()
    assert (want[3] != 0).mean() > 0.1
    compare(run(cur, cam, hist, prev_cam, **kw), want, True)


# ------------------------------------------------------------------ rendered frames
NX, NY, SPP, SEED = 48, 32, 2, 23


def test_on_rendered_frames_the_clamped_accumulation_equals_the_statement_and_feeds_the_denoiser():
    """random_scene 48 x 32, two frames of 2 spp (samples 0..1, 2..3) from two cameras a small
    step apart (test_gpu_temporal.rendered's recipe): rtnw.temporal_clamped of the second frame
    on the first equals temporal_clamped_ref bit for bit, the clamp binds on some pixels, and
    rtnw.denoise of the result, its len as the spp map and the variance pre-filter on, equals
    denoise_vf_ref of the statement's."""
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
    kw = dict(frame_spp=SPP, max_history=32, cos_normal=0.9, sigma_depth=0.1, radius=2, gamma=GAMMA)
    c0, m0, l0, k0 = run(f0, cams[0], None, None, **kw)
    check(c0, f0["color"], "first frame")
    assert (l0 == SPP).all() and not k0.any()
    hist = dict(color=c0, moments=m0, len=l0, features=f0["features"])
    got = run(f1, cams[1], hist, cams[0], **kw)
    want = temporal_clamped_ref(f1, cams[1], hist, cams[0], **kw)
    compare(got, want, True)
    took, bound = int((got[2] == 2 * SPP).sum()), int((got[3] != 0).sum())
    print(f"random_scene {NX}x{NY}, {SPP} spp a frame: {took} pixels with history, the clamp moved {bound} of them")
    assert set(np.unique(got[2])) == {SPP, 2 * SPP} and 1 <= bound < took
    dn = dict(rtnw.DENOISE_DEFAULTS)
    f = f1["features"]
    den = rtnw.denoise(got[0], f, got[1], got[2], variance_filter=1, **dn)
    want_den = denoise_vf_ref(want[0], f["albedo"], f["normal"], f["depth"], want[1], want[2], variance_filter=1, **dn)
    check(den, want_den, "clamped, accumulated, then denoised")
