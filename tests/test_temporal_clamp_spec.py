"""The clamped frame history, the CPU side: the exact statement of the rule, the ABI's struct and
entry points, and the argument checks of rt_temporal_clamped / rt_temporal_clamped_dev (made
before any HIP call, so they answer without a GPU).

The rule is rt_temporal's (tests/test_temporal_spec.py, whose `_reproject` this file calls) with
one step between the history fetch and the blend, stated here in numpy float32:
tests/test_gpu_temporal_clamp.py imports `temporal_clamped_ref` and compares the GPU's result with
it bit for bit.  The step's operations are add, subtract, multiply, IEEE divide, sqrt, comparisons
and selects on float32 values, in the order written; rt_temporal.hip's clamped kernel performs the
same sequence without contraction.  With the settings radius = r and gamma besides rt_temporal's:

    no history (first frame):   rt_temporal's rule;  clipped = 0
    cameras bytewise equal:     rt_temporal's rule, whatever r and gamma;  clipped = 0
    r = 0:                      rt_temporal's rule;  clipped = 0
    otherwise, for a pixel (x, y) with `use` true, c_h, mu_h = (u1, u2) and n_h as _reproject returns them:
        cnt = 0, S1 = 0, S2 = 0
        for dy = -r..r (outer), dx = -r..r (inner), when 0 <= x+dx < nx and 0 <= y+dy < ny:
            v = c_f[y+dy, x+dx];  cnt += 1;  S1 = S1 + v;  S2 = S2 + v*v             # per channel
        m = S1 / float(cnt);  var = S2 / float(cnt) - m*m;  var = var < 0 ? 0 : var;  sd = sqrt(var)
        lo = m - gamma*sd;  hi = m + gamma*sd
        c_h' = c_h < lo ? lo : (c_h > hi ? hi : c_h)                                 # per channel
        clipped = sum over the channels c of (c_h'[c] != c_h[c]) << c
        with moments and clipped != 0:
            y = (c_h[0] + c_h[1]) + c_h[2];  y' = (c_h'[0] + c_h'[1]) + c_h'[2]
            u1' = u1 + (y' - y);  u1' = u1' < 0 ? 0 : u1'
            v = u2 - u1*u1;  v = v < 0 ? 0 : v;  u2' = v + u1'*u1'
        otherwise u1' = u1, u2' = u2 bit for bit;  n_h is unchanged
        the blend is rt_temporal's on c_h', (u1', u2'), n_h
    a pixel with `use` false:   the frame's pixel bit for bit;  clipped = 0

A Jacobi pass: every value read is an input; window cells outside the image do not exist.
"""
import ctypes
import re

import numpy as np
import pytest

import rtnw
from test_temporal_spec import (DEV_WITHOUT_GPU, HAVE_DEVICE, RT_ERR_HIP, RT_ERR_INVALID, SETTINGS, _camera, _good,
                                _reproject, _struct_fields, bits, temporal_ref, two_camera_case, view, without_moments)

F = np.float32
# the box's half-width of the GPU tests: the value at which the two-camera case meets every class of
# test_the_two_camera_case_clamps_in_every_way below (gamma 1.0, the first candidate, does)
GAMMA = 1.0


# ------------------------------------------------------------------ the rule, in numpy
def temporal_clamped_ref(cur, cam, hist=None, prev_cam=None, *, radius, gamma, frame_spp, max_history, cos_normal,
                         sigma_depth, debug=None):
    """rt_temporal_clamped on host arrays, bit for bit: (colour, moments' or None, len, clipped).
    The arguments are temporal_ref's.  `debug`: a dict that receives, per pixel, the window's cell
    count `cnt`, its mean `mean`, the history colour before (`c_h`) and after (`c_h_clamped`) the
    step, `use`, and the masks `at_lo`, `at_hi` (a channel clipped there), `guard_u1`, `guard_v`
    (the moments' guard taken); all zero where the step did not run."""
    cf = np.ascontiguousarray(cur["color"], F)
    ny, nx, _ = cf.shape
    g = rtnw.pack_guides(cur["features"])
    S = None if cur.get("moments") is None else np.asarray(cur["moments"], F)
    n_f, r = int(frame_spp), int(radius)
    use = np.zeros((ny, nx), bool)
    nh = np.zeros((ny, nx), np.int64)
    ch = np.zeros((ny, nx, 3), F)
    mu = np.zeros((ny, nx, 2), F)
    clipped = np.zeros((ny, nx), np.int32)
    dbg = dict(cnt=np.zeros((ny, nx), np.int32), mean=np.zeros((ny, nx, 3), F), c_h=np.zeros((ny, nx, 3), F),
               c_h_clamped=np.zeros((ny, nx, 3), F), at_lo=np.zeros((ny, nx), bool), at_hi=np.zeros((ny, nx), bool),
               guard_u1=np.zeros((ny, nx), bool), guard_v=np.zeros((ny, nx), bool))
    if hist is not None:
        hc, hg = np.asarray(hist["color"], F), rtnw.pack_guides(hist["features"])
        hl = np.asarray(hist["len"], np.int32)
        hm = None if S is None else np.asarray(hist["moments"], F)
        with np.errstate(all="ignore"):
            if bytes(cam.desc) == bytes(prev_cam.desc):
                nh = np.minimum(hl, max_history).astype(np.int64)
                use = nh > 0
                ch = hc
                if S is not None:
                    mu = hm / hl.astype(F)[..., None]
            else:
                use, nh, ch, mu = _reproject(nx, ny, g, _camera(cam), hc, hg, hm, hl, _camera(prev_cam), max_history,
                                             cos_normal, sigma_depth, None)
                if r >= 1:
                    ch, mu, clipped = _clamp(cf, use, ch, mu, S is not None, r, F(gamma), dbg)
    with np.errstate(all="ignore"):
        n = np.where(use, nh + n_f, n_f).astype(np.int32)
        fn, nf = n.astype(F), F(n_f)
        a = nf / fn
        out = np.where(use[..., None], ch + (cf - ch) * a[..., None], cf)
        mom = None
        if S is not None:
            mom = np.where(use[..., None], (mu + (S / nf - mu) * a[..., None]) * fn[..., None], S)
            assert mom.dtype == F
    assert out.dtype == F and clipped.dtype == np.int32
    if debug is not None:
        debug.update(dbg, use=use)
    return out, mom, n, clipped


def _clamp(cf, use, ch, mu, have, r, gamma, dbg):
    """The inserted step on every pixel with `use`: (c_h', mu', clipped)."""
    ny, nx, _ = cf.shape
    cnt = np.zeros((ny, nx), np.int32)
    S1, S2 = np.zeros((ny, nx, 3), F), np.zeros((ny, nx, 3), F)
    X, Y = np.arange(nx)[None, :], np.arange(ny)[:, None]
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            inn = (X + dx >= 0) & (X + dx < nx) & (Y + dy >= 0) & (Y + dy < ny)
            v = cf[np.clip(Y + dy, 0, ny - 1), np.clip(X + dx, 0, nx - 1)]   # any in-image cell: `inn` masks it
            cnt = cnt + inn
            S1 = np.where(inn[..., None], S1 + v, S1)
            S2 = np.where(inn[..., None], S2 + v * v, S2)
    fc = cnt.astype(F)[..., None]
    m = S1 / fc
    var = S2 / fc - m * m
    var = np.where(var < F(0), F(0), var)
    sd = np.sqrt(var)
    lo, hi = m - gamma * sd, m + gamma * sd
    assert lo.dtype == hi.dtype == F
    chc = np.where(ch < lo, lo, np.where(ch > hi, hi, ch))
    moved = use[..., None] & (chc != ch)
    clipped = (moved * np.array([1, 2, 4], np.int32)).sum(-1).astype(np.int32)
    chc = np.where(use[..., None], chc, ch)
    mu2 = mu
    if have:
        y = (ch[..., 0] + ch[..., 1]) + ch[..., 2]
        yc = (chc[..., 0] + chc[..., 1]) + chc[..., 2]
        u1, u2 = mu[..., 0], mu[..., 1]
        w1 = u1 + (yc - y)
        g1 = w1 < F(0)
        w1 = np.where(g1, F(0), w1)
        v = u2 - u1 * u1
        gv = v < F(0)
        v = np.where(gv, F(0), v)
        w2 = v + w1 * w1
        hit = clipped != 0
        mu2 = np.where(hit[..., None], np.stack([w1, w2], -1), mu)
        assert mu2.dtype == F
        dbg.update(guard_u1=hit & g1, guard_v=hit & gv)
    dbg.update(cnt=np.where(use, cnt, 0).astype(np.int32), mean=np.where(use[..., None], m, F(0)),
               c_h=np.where(use[..., None], ch, F(0)), c_h_clamped=np.where(use[..., None], chc, F(0)),
               at_lo=(moved & (ch < lo)).any(-1), at_hi=(moved & (ch > hi)).any(-1))
    return chc, mu2, clipped


CLAMP = dict(radius=2, gamma=GAMMA)


# ------------------------------------------------------------------ properties of the rule
@pytest.mark.parametrize("gamma", [0.0, 1.0, 7.5])
@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no-moments"])
@pytest.mark.parametrize("nx,ny", [(130, 9), (33, 40)])
def test_radius_zero_is_the_unclamped_rule_bit_for_bit(nx, ny, moments, gamma):
    cur, cam, hist, prev_cam = two_camera_case(nx, ny)
    if not moments:
        cur, hist = without_moments(cur), without_moments(hist)
    want, want_mom, want_len = temporal_ref(cur, cam, hist, prev_cam, **SETTINGS)
    out, mom, ln, clipped = temporal_clamped_ref(cur, cam, hist, prev_cam, radius=0, gamma=gamma, **SETTINGS)
    assert np.array_equal(bits(out), bits(want)) and np.array_equal(ln, want_len) and not clipped.any()
    assert (mom is None and want_mom is None) if not moments else np.array_equal(bits(mom), bits(want_mom))
    # a first frame likewise, at any radius
    out, mom, ln, clipped = temporal_clamped_ref(cur, cam, radius=3, gamma=gamma, **SETTINGS)
    assert np.array_equal(bits(out), bits(cur["color"])) and (ln == SETTINGS["frame_spp"]).all() and not clipped.any()


def test_equal_cameras_are_not_clamped():
    nx, ny = 33, 40
    cur, cam, hist, _ = two_camera_case(nx, ny)
    same = view(nx, ny, (0.45, 0.55, -5.9), (0.35, 0.3, 0.0))
    assert same is not cam and bytes(same.desc) == bytes(cam.desc)
    want, want_mom, want_len = temporal_ref(cur, cam, hist, same, **SETTINGS)
    out, mom, ln, clipped = temporal_clamped_ref(cur, cam, hist, same, radius=3, gamma=0.0, **SETTINGS)
    assert np.array_equal(bits(out), bits(want)) and np.array_equal(bits(mom), bits(want_mom))
    assert np.array_equal(ln, want_len) and not clipped.any()


@pytest.mark.parametrize("radius,gamma", [(1, 0.0), (2, 1.0), (3, 2.5)])
def test_a_constant_frame_replaces_every_history_colour_by_the_constant(radius, gamma):
    """sd = 0, so lo = hi = m = the constant (a sum of cnt <= 49 equal values of 0.375 is exact, and
    so is its quotient), and the blend of equal values returns it."""
    nx, ny = 33, 40
    cur, cam, hist, prev_cam = two_camera_case(nx, ny)
    const = np.broadcast_to(np.array([0.375, 1.5, 0.0], F), (ny, nx, 3)).copy()
    dbg = {}
    out, mom, ln, clipped = temporal_clamped_ref(dict(cur, color=const), cam, hist, prev_cam, radius=radius, gamma=gamma,
                                                 debug=dbg, **SETTINGS)
    assert dbg["use"].sum() * 4 >= nx * ny
    assert np.array_equal(bits(out), bits(const))
    # an arbitrary history differs from the constant in every channel
    assert (clipped[dbg["use"]] == 7).all() and not clipped[~dbg["use"]].any()
    _, _, want_len = temporal_ref(cur, cam, hist, prev_cam, **SETTINGS)
    assert np.array_equal(ln, want_len)                       # n_h is unchanged


def test_gamma_zero_moves_a_clipped_channel_to_the_window_mean():
    cur, cam, hist, prev_cam = two_camera_case(33, 40)
    dbg = {}
    _, _, _, clipped = temporal_clamped_ref(cur, cam, hist, prev_cam, radius=2, gamma=0.0, debug=dbg, **SETTINGS)
    assert (clipped != 0).sum() * 4 >= 33 * 40
    for c in range(3):
        hit = (clipped >> c & 1) == 1
        assert hit.any() and np.array_equal(bits(dbg["c_h_clamped"][hit, c]), bits(dbg["mean"][hit, c]))
        keep = dbg["use"] & ~hit
        assert np.array_equal(bits(dbg["c_h_clamped"][keep, c]), bits(dbg["c_h"][keep, c]))


def test_a_corner_pixel_at_radius_three_uses_sixteen_cells():
    """On a 5 x 4 image the 7 x 7 window of a corner keeps 4 x 4 cells; an exact camera step of one
    pixel gives every column but the last a history."""
    from test_temporal_spec import plane_guides
    nx, ny = 5, 4
    wall = [((0.0, 0.0, -1.0), (0.0, 0.0, 8.0), -1e9, 1e9, 1e9, (0.5, 0.5, 0.5))]
    cam, prev_cam = view(nx, ny, (0.2, 0.0, -8.0), (0.2, 0.0, 0.0)), view(nx, ny, (0.0, 0.0, -8.0), (0.0, 0.0, 0.0))
    rng = np.random.default_rng(11)
    cur = dict(color=(rng.random((ny, nx, 3)) * 2).astype(F), features=plane_guides(cam, nx, ny, wall), moments=None)
    hist = dict(color=(rng.random((ny, nx, 3)) * 2).astype(F), features=plane_guides(prev_cam, nx, ny, wall), moments=None,
                len=np.full((ny, nx), 8, np.int32))
    dbg = {}
    temporal_clamped_ref(cur, cam, hist, prev_cam, radius=3, gamma=1.0, debug=dbg, **SETTINGS)
    assert dbg["use"][0, 0] and dbg["use"][ny - 1, 0] and dbg["use"][0, nx - 1] and dbg["use"][ny - 1, nx - 1]
    assert dbg["cnt"][0, 0] == 16 and dbg["cnt"][ny - 1, 0] == 16          # x 0..3, y 0..3 / y 0..3
    assert dbg["cnt"][0, nx - 1] == 16 and dbg["cnt"][ny - 1, nx - 1] == 16   # x 1..4
    assert dbg["cnt"][1, 2] == 20                                        # x 0..4, y 0..3: the whole image
    # the mean of a corner's window, added in the statement's order
    s = F(0)
    for y in range(4):
        for x in range(4):
            s = s + cur["color"][y, x, 1]
    assert dbg["mean"][0, 0, 1] == s / F(16)


@pytest.mark.parametrize("nx,ny", [(130, 9), (33, 40)])
def test_the_two_camera_case_clamps_in_every_way(nx, ny):
    """What tests/test_gpu_temporal_clamp.py compares on the GPU, at radius 2 and GAMMA, exercises
    both ends of the box, unclipped pixels, windows cut by the border and the moments' guard."""
    cur, cam, hist, prev_cam = two_camera_case(nx, ny)
    dbg = {}
    out, mom, ln, clipped = temporal_clamped_ref(cur, cam, hist, prev_cam, debug=dbg, **CLAMP, **SETTINGS)
    assert np.isfinite(out).all() and np.isfinite(mom).all()
    use = dbg["use"]
    n = int(use.sum())
    lo, hi, free = int(dbg["at_lo"].sum()), int(dbg["at_hi"].sum()), int((use & (clipped == 0)).sum())
    cut = int(((clipped != 0) & (dbg["cnt"] < 25)).sum())
    guard = int((dbg["guard_u1"] | dbg["guard_v"]).sum())
    print(f"{nx}x{ny}, radius 2, gamma {GAMMA}: {n} pixels with history; clipped at lo {lo}, at hi {hi}, not at all {free}; "
          f"clipped with a cut window {cut}; guard taken {guard} (u1 {int(dbg['guard_u1'].sum())}, v {int(dbg['guard_v'].sum())})")
    assert n * 4 >= nx * ny
    assert lo * 20 >= n and hi * 20 >= n and free * 4 >= n
    assert cut >= 1 and guard >= 1
    assert not clipped[~use].any() and ((clipped >= 0) & (clipped <= 7)).all()
    # without moments: the same colour, len and mask
    out2, none, ln2, clipped2 = temporal_clamped_ref(without_moments(cur), cam, without_moments(hist), prev_cam, **CLAMP,
                                                     **SETTINGS)
    assert none is None and np.array_equal(bits(out), bits(out2)) and np.array_equal(ln, ln2)
    assert np.array_equal(clipped, clipped2)
    # an unclipped pixel's moments are the unclamped rule's bit for bit; len is unchanged everywhere
    want, want_mom, want_len = temporal_ref(cur, cam, hist, prev_cam, **SETTINGS)
    assert np.array_equal(ln, want_len)
    keep = clipped == 0
    assert np.array_equal(bits(out[keep]), bits(want[keep])) and np.array_equal(bits(mom[keep]), bits(want_mom[keep]))
    assert not np.array_equal(bits(out[~keep]), bits(want[~keep]))


# ------------------------------------------------------------------ the ABI
def test_the_clamp_struct_and_entry_points_match_the_header():
    want = _struct_fields("rt_temporal_clamp_params")
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    got = list(rtnw.RtTemporalClampParams._fields_)
    assert [n for n, _ in got] == [re.sub(r"\[.*\]", "", n) for n, _ in want] == ["radius", "gamma", "pad"]
    for (n, t), (wn, wt) in zip(got, want):
        size = re.search(r"\[(\d+)\]", wn)
        assert t == (ctype[wt] * int(size.group(1)) if size else ctype[wt]), n
    assert ctypes.sizeof(rtnw.RtTemporalClampParams) == 32
    L = rtnw.lib()
    for name in ("rt_temporal_clamped", "rt_temporal_clamped_dev", "rt_launch_temporal_clamped"):
        assert hasattr(L, name), name
    assert {"rt_temporal_clamped", "rt_temporal_clamped_dev"} <= set(rtnw.header_symbols())
    assert L.rt_temporal_clamped.argtypes is not None and L.rt_temporal_clamped_dev.argtypes is not None
    cp = rtnw.temporal_clamp_params(2, 1.5)
    assert cp.radius == 2 and cp.gamma == 1.5 and list(cp.pad) == [0] * 6
    d = rtnw.temporal_clamp_params()
    assert d.radius == rtnw.TEMPORAL_CLAMP_DEFAULTS["radius"] and d.gamma == F(rtnw.TEMPORAL_CLAMP_DEFAULTS["gamma"])
    assert hasattr(rtnw, "temporal_clamped")


# ------------------------------------------------------------------ argument checks, no GPU
def _call(tp, cp, *, nx=4, ny=3, null=None, moments="both", out_moments=True, history=True, alias=None, dev=False,
          clipped=True):
    """rt_temporal_clamped / rt_temporal_clamped_dev on small host buffers (never read when a
    check fails; the device form's pointers are never read on the host at all)."""
    L = rtnw.lib()
    h, w = min(max(ny, 1), 8), min(max(nx, 1), 8)   # an oversized image fails the size check: nothing is read
    mk = lambda c: np.zeros((h, w, c), np.float32)
    buf = {"cur.color": mk(3), "cur.guides": mk(8), "cur.moments": mk(2), "hist.color": mk(3), "hist.guides": mk(8),
           "hist.moments": mk(2), "hist.len": np.ones((h, w), np.int32), "out.color": mk(3), "out.moments": mk(2),
           "out.len": np.zeros((h, w), np.int32), "clipped": np.zeros((h, w), np.int32)}
    ptr = {k: (None if k == null else v.ctypes.data) for k, v in buf.items()}
    if moments in ("none", "hist"):
        ptr["cur.moments"] = None
    if moments in ("none", "cur"):
        ptr["hist.moments"] = None
    if not out_moments:
        ptr["out.moments"] = None
    if alias:
        ptr[alias[0]] = ptr[alias[1]]
    cur = rtnw.RtTemporalFrame(ptr["cur.color"], ptr["cur.guides"], ptr["cur.moments"], None)
    hist = rtnw.RtTemporalFrame(ptr["hist.color"], ptr["hist.guides"], ptr["hist.moments"], ptr["hist.len"])
    out = rtnw.RtTemporalFrame(ptr["out.color"], None, ptr["out.moments"], ptr["out.len"])
    cam = rtnw.Camera.preset("cornell", w, h)
    prev = rtnw.Camera.preset("final_alt", w, h)
    ref = lambda name, v: None if null == name else ctypes.byref(v)
    args = (0, nx, ny, ref("cur", cur), ref("cam", cam.desc), ref("hist", hist) if history else None,
            ref("prev_cam", prev.desc) if history else None, ref("tp", tp), ref("cp", cp), ref("out", out),
            ptr["clipped"] if clipped else None)
    rc = L.rt_temporal_clamped_dev(*args, None) if dev else L.rt_temporal_clamped(*args, None)
    return rc, L.rt_last_error().decode()


def _clamp_params(radius=2, gamma=GAMMA, pad=None):
    cp = rtnw.RtTemporalClampParams(radius, gamma)
    if pad is not None:
        cp.pad[pad] = 1
    return cp


@pytest.mark.parametrize("dev", [False, DEV_WITHOUT_GPU])
def test_valid_arguments_reach_the_device_check(dev):
    for cp, kw in ((_clamp_params(), {}), (_clamp_params(radius=0), {}), (_clamp_params(radius=3), {}),
                   (_clamp_params(gamma=0.0), {}), (_clamp_params(gamma=1e30), {}), (_clamp_params(), dict(clipped=False)),
                   (_clamp_params(), dict(history=False)), (_clamp_params(), dict(moments="none", out_moments=False)),
                   (_clamp_params(), dict(alias=("out.moments", "cur.moments")))):
        rc, msg = _call(_good(), cp, dev=dev, **kw)
        assert rc != RT_ERR_INVALID, (rc, msg)
        if HAVE_DEVICE:   # the host form stages its host buffers itself: a legal call
            assert rc == rtnw.RT_OK, (rc, msg)
        else:             # nothing about the arguments
            assert rc == RT_ERR_HIP and "hipSetDevice" in msg, (rc, msg)


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("null", ["cur", "cam", "prev_cam", "tp", "cp", "out", "cur.color", "cur.guides", "hist.color",
                                  "hist.guides", "hist.len", "out.color", "out.len"])
def test_null_arguments_are_invalid(null, dev):
    rc, msg = _call(_good(), _clamp_params(), null=null, dev=dev)
    assert rc == RT_ERR_INVALID and "null argument" in msg and null.replace(".", "->") in msg, msg
    assert ("rt_temporal_clamped_dev:" if dev else "rt_temporal_clamped:") in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("field,value", [("radius", -1), ("radius", 4), ("radius", 1 << 30), ("gamma", -0.5),
                                         ("gamma", float("nan")), ("gamma", float("inf")), ("gamma", float("-inf")),
                                         ("pad", 0), ("pad", 5)])
def test_bad_clamp_parameters_are_invalid(field, value, dev):
    rc, msg = _call(_good(), _clamp_params(**{field: value}), dev=dev)
    assert rc == RT_ERR_INVALID and field in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("field,value", [
    ("max_history", -1), ("max_history", (1 << 23) + 1), ("cos_normal", -1.5), ("cos_normal", 1.01),
    ("cos_normal", float("nan")), ("sigma_depth", -1.0), ("sigma_depth", float("nan")), ("frame_spp", 0),
    ("frame_spp", 65536), ("pad", 0), ("pad", 3),
])
def test_the_unclamped_rules_bad_parameters_are_invalid(field, value, dev):
    rc, msg = _call(_good(**{field: value}), _clamp_params(), dev=dev)
    assert rc == RT_ERR_INVALID and field in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("nx,ny", [(0, 3), (4, 0), (-1, 3), (65536, 32768), (1 << 30, 2)])
def test_empty_and_oversized_images_are_invalid(nx, ny, dev):
    rc, msg = _call(_good(), _clamp_params(), nx=nx, ny=ny, dev=dev)
    assert rc == RT_ERR_INVALID and "nx and ny" in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("moments,out_moments,word", [("cur", True, "hist->moments"), ("hist", False, "cur->moments"),
                                                      ("none", True, "out->moments")])
def test_moments_given_inconsistently_are_invalid(moments, out_moments, word, dev):
    rc, msg = _call(_good(), _clamp_params(), moments=moments, out_moments=out_moments, dev=dev)
    assert rc == RT_ERR_INVALID and word in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("a,b", [("out.color", "cur.color"), ("out.color", "hist.color"), ("out.moments", "hist.moments"),
                                 ("out.len", "hist.len")])
def test_in_place_is_invalid(a, b, dev):
    rc, msg = _call(_good(), _clamp_params(), alias=(a, b), dev=dev)
    assert rc == RT_ERR_INVALID and a.replace(".", "->") in msg and b.replace(".", "->") in msg, msg


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("other", ["cur.color", "cur.guides", "cur.moments", "hist.color", "hist.guides", "hist.moments",
                                   "hist.len", "out.color", "out.moments", "out.len"])
def test_a_mask_that_is_one_of_the_frames_arrays_is_invalid(other, dev):
    rc, msg = _call(_good(), _clamp_params(), alias=("clipped", other), dev=dev)
    assert rc == RT_ERR_INVALID and "clipped" in msg, msg
