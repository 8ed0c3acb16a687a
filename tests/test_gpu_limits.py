"""GPU parity at the ABI's numeric limits (include/rt_hip.h, rt_render_params): far tiles of a
65535 x 65535 frame, the last legal sample indices, seeds with the top bit set, chunks up to
INT_MAX, and the refusal of everything beyond.

The cases are tests/limit_cases.py's; tests/test_limits_spec.py has already shown, without a
GPU, that the oracle's image of each can tell its pixels apart, so a wrong pixel key, packed
coordinate or sample index changes the image compared here.  The bar is
tests/test_gpu_parity.py's (TOL_RMS everywhere, every pixel bitwise where the host libm is the
pinned one); cornell_box calls no libm function on the device, so it is held bit for bit on
any host.  Every render is of at most a few hundred pixels at 1-8 spp, the strips' 65535
pixels at 1 spp.
"""
import ctypes

import numpy as np
import pytest

import limit_cases as LC
import oracle as O
import rtnw
from limit_cases import Case
from test_adaptive_guard_spec import count_map, predict_guarded
from test_gpu_adaptive import bits, np_moments, np_sums, same
from test_gpu_generated import no_sine_prims
from test_gpu_parity import THREADS, TOL_RMS, _scene, assert_exact, gamma_rms, pixel_exact

pytestmark = pytest.mark.gpu

N, T = LC.N, LC.T
RT_ERR_INVALID = -1
SENTINEL = np.float32(-7.25)
SUM_IN = rtnw.RT_FLAG_SUM_IN
ids = dict(ids=lambda c: c.name)
BATCHED = 64 * 16   # RTNW_SLAB_BUDGET with room for one work item of each of a tile's 64 pixels: a launch per chunk


# ------------------------------------------------------------------ harness
_cams, _oracle, _one = {}, {}, {}


def frame(scene):
    """(scene on the device, the frame's camera): test_gpu_parity's scene cache."""
    if scene not in _cams:
        _cams[scene] = Case(scene, LC.FAR).camera()
    return _scene(scene), _cams[scene]


def oracle_both(case, **kw):
    """(image, axis mask) of the case in the oracle's statement (limit_cases.oracle_image, fields
    replaced by kw), rendered once, never written."""
    key = (case, tuple(sorted(kw.items())))
    if key not in _oracle:
        img, axis = LC.oracle_image(case, THREADS, **kw)
        img.setflags(write=False)
        axis.setflags(write=False)
        _oracle[key] = (img, axis)
    return _oracle[key]


def oracle(case, **kw):
    return oracle_both(case, **kw)[0]


def gpu(case, stats=False, **kw):
    sc, cam = frame(case.scene)
    return sc.render_tile(cam, case.params(**kw), *case.rect, stats=stats)


def gpu_samples(case, n):
    """[n, h, w, 3]: sample k's radiance from one-sample renders (spp 1 at sample_offset k)."""
    key = (case.scene, case.rect, case.seed)
    if key not in _one or _one[key].shape[0] < n:
        one = np.stack([gpu(case, spp=1, chunk=1, sample_offset=k) for k in range(n)])
        one.setflags(write=False)
        _one[key] = one
    return _one[key][:n]


def oracle_samples(case, n, first=0):
    return np.stack([oracle(case, ns=1, chunk=1, sample_offset=first + k) for k in range(n)])


def hold(case, exact):
    """The bit-exact bar: on any host for cornell_box (no libm call), else assert_exact's policy."""
    if case.scene == "cornell_box":
        assert exact == 1.0, exact
    else:
        assert_exact(exact)


def check(case, g, o, what=""):
    assert g.shape == o.shape
    assert np.isfinite(g).all() and (g >= 0).all()
    rms, exact = gamma_rms(g, o), pixel_exact(g, o)
    print(f"{case.name}{what}: gamma RMS {rms}, bit-exact pixels {exact:.4f}")
    for q in np.nonzero((bits(g) != bits(o)).any(axis=-1).ravel())[0][:8]:   # what differs, before any bar
        print(f"  pixel {q}: {g.reshape(-1, 3)[q]} against the oracle's {o.reshape(-1, 3)[q]}")
    assert (rms <= TOL_RMS).all(), rms
    hold(case, exact)


class Dev:
    """Device memory holding a copy of a host array."""

    def __init__(self, host):
        self.host = np.ascontiguousarray(host)
        self.p = ctypes.c_void_p()
        rtnw._check(rtnw.lib().rt_device_alloc(0, self.host.nbytes, ctypes.byref(self.p)))
        rtnw._check(rtnw.lib().rt_copy_to_device(self.p, self.host.ctypes.data, self.host.nbytes))

    def read(self):
        out = np.empty_like(self.host)
        rtnw._check(rtnw.lib().rt_copy_to_host(out.ctypes.data, self.p, out.nbytes))
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        rtnw.lib().rt_device_free(self.p)


def tile_array(rects):
    return np.ascontiguousarray(np.asarray(rects, np.int32).reshape(-1, 4))


# ------------------------------------------------------------------ 1. frames
def repeated(px):
    """[n] bool: the pixels of px [n, 3] that bit-equal another one of them."""
    _, inverse, counts = np.unique(bits(px), axis=0, return_inverse=True, return_counts=True)
    return counts[inverse.ravel()] > 1


@pytest.mark.parametrize("case", LC.FRAME_CASES, **ids)
def test_far_tiles_corner_pixels_and_strips_match_the_oracle(case):
    """Every pixel, but for the strips' few whose oracle path holds a ray exactly parallel to an
    axis (limit_cases.AXIS_PIXELS: outside the parity contract).  A strip's 65535 one-sample
    pixels hold some bit-equal ones; they are the same pixels on both sides."""
    g = gpu(case)
    o, axis = oracle_both(case)
    assert int(axis.sum()) == LC.AXIS_PIXELS.get((case.scene, case.rect), 0)
    assert np.isfinite(g).all() and (g >= 0).all()
    keep = ~axis
    check(case, g[keep][None], o[keep][None], f" without {int(axis.sum())} pixels" if axis.any() else "")
    if case.strip:
        assert np.array_equal(repeated(g[keep]), repeated(o[keep]))


# ------------------------------------------------------------------ 2. every entry point at a far tile
@pytest.mark.parametrize("case", LC.FOLD_CASES, **ids)
def test_right_fold_at_far_tiles_matches_the_oracles_right_fold(case):
    check(case, gpu(case), oracle(case))


@pytest.mark.parametrize("scene", LC.SCENES)
def test_tiles_and_corner_pixels_in_one_call_equal_the_single_tile_renders(scene):
    """rt_render_tiles packs the tiles back to back: each tile's base offset, and on final the
    deep pixels of all tiles ahead of the others."""
    rects = LC.tiles(scene) + LC.PIXELS
    sc, cam = frame(scene)
    total = sum(w * h for _, _, w, h in rects)
    with Dev(np.full(total * 3 + 3, SENTINEL, np.float32)) as d:
        sc.render_tiles(cam, Case(scene, LC.FAR).params(), tile_array(rects), d.p.value)
        packed = d.read()
    off = 0
    for r in rects:
        n = r[2] * r[3] * 3
        assert same(packed[off:off + n].reshape(r[3], r[2], 3), gpu(Case(scene, r))), r
        off += n
    assert (packed[off:] == SENTINEL).all()   # nothing past the last tile


@pytest.mark.parametrize("case", LC.ENTRY_CASES, **ids)
def test_moments_at_far_tiles_are_the_float32_sums_of_the_one_sample_renders(case):
    sc, cam = frame(case.scene)
    out, mom = sc.render_tile_moments(cam, case.params(), *case.rect)
    assert same(out, gpu(case))
    one = gpu_samples(case, case.spp)
    assert same((np_sums(one) * np.float32(1.0 / case.spp)).astype(np.float32), out)
    assert same(np_moments(one), mom)
    assert (mom[..., 1] > 0).mean() >= 0.5
    exact = float(np.mean(np.all(bits(np_moments(oracle_samples(case, case.spp))) == bits(mom), axis=-1)))
    print(f"{case.name}: moments bit-exact against the oracle on {exact:.4f} of the pixels")
    hold(case, exact)


@pytest.mark.parametrize("r", [None, 0, 2])
@pytest.mark.parametrize("rect", LC.entry_tiles(LC.ADAPTIVE_SCENE))
def test_adaptive_renders_at_far_tiles(rect, r):
    """rt_render_adaptive (r None) and rt_render_adaptive_guarded: the sample counts follow
    tests/test_adaptive_guard_spec.py's statement on the GPU's own one-sample renders of the far
    tile, and a pixel that got n samples is that pixel of the fixed n-spp render."""
    a = LC.ADAPTIVE
    mn, step, cap, tol, floor = a["mn"], a["step"], a["cap"], a["tol"], a["floor"]
    case = Case(LC.ADAPTIVE_SCENE, rect, spp=cap, chunk=1)
    sc, cam = frame(case.scene)
    img, spp, mom, st = sc.render_adaptive(cam, case.params(), *rect, min_spp=mn, step_spp=step, tolerance=tol,
                                           floor=floor, guard_radius=r)
    want_spp, want_mom, held = predict_guarded(gpu_samples(case, cap), mn, step, cap, tol, floor, r or 0)
    counts = count_map(spp)
    print(f"{case.name} r {r}: spp map {counts}, held {int(held.sum())}")
    assert np.array_equal(spp, want_spp)
    assert same(mom, want_mom)
    for n in counts:
        sel = spp == n
        assert np.array_equal(bits(img)[sel], bits(gpu(case, spp=n))[sel]), n
    assert st["samples"] == int(spp.sum())
    assert len(counts) >= 2
    assert bool(held.any()) == (r == 2)
    # cornell_box calls no libm function: the oracle's samples predict the same map on any host
    o_spp, _, _ = predict_guarded(oracle_samples(case, cap), mn, step, cap, tol, floor, r or 0)
    assert np.array_equal(spp, o_spp)


def check_features(case, f, fh, desc):
    """tests/test_gpu_generated.py's bar for the feature pass: coverage, depth and normal bit for
    bit, and the albedo wherever no sample's colour involves a sine; the rest by assert_exact."""
    o = O.feature_means(fh)
    share = {k: float(np.mean(bits(f[k]) == bits(o[k]))) for k in ("coverage", "albedo", "depth", "normal")}
    print(f"{case.name}: feature bit-exact shares {share}, coverage {float(o['coverage'].mean()):.3f}")
    for k in ("coverage", "depth", "normal"):
        assert np.array_equal(bits(f[k]), bits(o[k])), k
    no_sine = no_sine_prims(desc)[fh["prim"]].all(axis=-1)
    assert np.array_equal(bits(f["albedo"])[no_sine], bits(o["albedo"])[no_sine])
    if O.host_libm_pinned()[0]:
        assert np.array_equal(bits(f["albedo"]), bits(o["albedo"]))
    return o


@pytest.mark.parametrize("case", LC.FEATURE_CASES, **ids)
def test_features_at_far_tiles_match_the_oracles_first_hits(case):
    sc, cam = frame(case.scene)
    f = sc.render_features(cam, case.params(), *case.rect)
    o = check_features(case, f, O.first_hits_desc(sc.desc, cam, case.desc_spec(threads=THREADS)), sc.desc)
    assert (o["coverage"] == 1).all() and len(np.unique(bits(o["depth"]))) > T * T // 2


# ------------------------------------------------------------------ 3. the last sample indices
@pytest.mark.parametrize("budget", [None, BATCHED])
@pytest.mark.parametrize("case", LC.LAST_CASES, **ids)
def test_the_last_sample_indices_match_the_oracle(case, budget, monkeypatch):
    """Samples 0xFFFFFFF8 .. 0xFFFFFFFE in chunks of 3, in one launch and in one per chunk."""
    if budget:
        monkeypatch.setenv("RTNW_SLAB_BUDGET", str(budget))
    g, st = gpu(case, stats=True)
    assert st["batches"] == (3 if budget else 1) and st["chunk"] == 3
    check(case, g, oracle(case), f" in {int(st['batches'])} launches")
    assert not same(g, gpu(case, sample_offset=0))   # other samples than the first seven


@pytest.mark.parametrize("scene", LC.SCENES)
def test_features_at_the_last_sample_indices(scene, monkeypatch):
    case = Case(scene, LC.centre(scene), spp=LC.LAST_SPP, chunk=3, sample_offset=LC.LAST - LC.LAST_SPP)
    sc, cam = frame(scene)
    fh = O.first_hits_desc(sc.desc, cam, case.desc_spec(threads=THREADS))
    f = sc.render_features(cam, case.params(), *case.rect)
    check_features(case, f, fh, sc.desc)
    monkeypatch.setenv("RTNW_SLAB_BUDGET", str(BATCHED))
    g = sc.render_features(cam, case.params(), *case.rect)
    assert all(same(f[k], g[k]) for k in f)
    first = sc.render_features(cam, case.params(sample_offset=0), *case.rect)
    assert not same(first["depth"], f["depth"]) or not same(first["albedo"], f["albedo"])


@pytest.mark.parametrize("budget", [None, BATCHED])
@pytest.mark.parametrize("case", LC.SUM_IN_CASES, **ids)
def test_sum_in_at_the_last_sample_indices(case, budget, monkeypatch):
    """RT_FLAG_SUM_IN from arbitrary finite sums S: the output is the float32 statement
    (S + s_0 + s_1 + ...) * float(1.0 / (offset + spp)), the s_k from one-sample oracle renders;
    offset + spp is 0xFFFFFFFF, whose float is 2^32."""
    if budget:
        monkeypatch.setenv("RTNW_SLAB_BUDGET", str(budget))
    x0, y0, w, h = case.rect
    S = np.random.default_rng(11).uniform(0.0, 4.0, (h, w, 3)).astype(np.float32)
    sc, cam = frame(case.scene)
    out, st = sc.render_tile(cam, case.params(flags=SUM_IN), *case.rect, stats=True, sums=S)
    assert st["batches"] == (case.spp if budget else 1)
    one = oracle_samples(case, case.spp, first=case.sample_offset)
    acc = S.copy()
    for s in one:
        acc = (acc + s).astype(np.float32)
    k = np.float32(1.0 / float(np.float32(case.sample_offset + case.spp)))
    assert k == np.float32(2.0 ** -32)
    want = (acc * k).astype(np.float32)
    assert np.isfinite(out).all() and (out > 0).all()
    exact = pixel_exact(out, want)
    # the samples' own mean, for the RMS bar: the sums as delivered, S taken off again
    mean_g = ((out.astype(np.float64) * 2.0 ** 32 - S) / case.spp).astype(np.float32)
    mean_o = ((want.astype(np.float64) * 2.0 ** 32 - S) / case.spp).astype(np.float32)
    rms = gamma_rms(mean_g, mean_o)
    print(f"{case.name} SUM_IN in {int(st['batches'])} launches: gamma RMS of the samples' mean {rms}, bit-exact pixels {exact:.4f}")
    assert (rms <= TOL_RMS).all(), rms
    hold(case, exact)
    assert not same(out, (S * k).astype(np.float32))   # the samples were added


@pytest.fixture(scope="module")
def dist1():
    d = rtnw.Dist(rtnw.dist_unique_id(), 0, 1, 0)
    yield d
    d.close()


def refused(rc, word):
    msg = rtnw.lib().rt_last_error().decode()
    assert rc == RT_ERR_INVALID and word in msg, (rc, msg)


def every_entry_point_refuses(sc, cam, p, rect, word, adaptive):
    """RT_ERR_INVALID with `word` in the message from every render entry point that takes p, and
    sentinel-filled outputs, on the host or on the device, unchanged."""
    L = rtnw.lib()
    x0, y0, w, h = rect
    cp, pp = ctypes.byref(cam.desc), ctypes.byref(p)
    tile = tile_array([rect])
    sent = lambda *shape: np.full(shape, SENTINEL, np.float32)   # noqa: E731
    untouched = lambda a: bool((a == SENTINEL).all())            # noqa: E731
    out = sent(h, w, 3)
    refused(L.rt_render_tile(sc.handle, cp, pp, x0, y0, w, h, out.ctypes.data, None), word)
    assert untouched(out)
    with Dev(sent(h, w, 3)) as d, Dev(sent(h, w, 2)) as m, Dev(sent(h, w, 8)) as g:
        refused(L.rt_render_tiles(sc.handle, cp, pp, tile.ctypes.data, 1, d.p, None, None), word)
        # (a rank without tiles answers as the ranks with tiles do)
        refused(L.rt_render_tiles(sc.handle, cp, pp, None, 0, None, None, None), word)
        refused(L.rt_render_tiles_moments(sc.handle, cp, pp, None, 0, None, None, None, None), word)
        refused(L.rt_render_tiles_moments(sc.handle, cp, pp, tile.ctypes.data, 1, d.p, m.p, None, None), word)
        refused(L.rt_render_features_dev(sc.handle, cp, pp, x0, y0, w, h, g.p, None), word)
        assert untouched(d.read()) and untouched(m.read()) and untouched(g.read())
    f = [sent(h, w, 3), sent(h, w, 3), sent(h, w), sent(h, w)]
    refused(L.rt_render_features(sc.handle, cp, pp, x0, y0, w, h, *[a.ctypes.data for a in f]), word)
    assert all(untouched(a) for a in f)
    if adaptive:   # (the adaptive entry points take no sample_offset but 0)
        ap = rtnw.RtAdaptiveParams(min_spp=2, step_spp=1, tolerance=0.1, floor=0.01)
        for guarded in (False, True):
            out, mom, spp = sent(h, w, 3), sent(h, w, 2), np.full((h, w), -7, np.int32)
            tail = (x0, y0, w, h, out.ctypes.data, spp.ctypes.data, mom.ctypes.data, None)
            if guarded:
                refused(L.rt_render_adaptive_guarded(sc.handle, cp, pp, ctypes.byref(ap), 1, *tail), word)
            else:
                refused(L.rt_render_adaptive(sc.handle, cp, pp, ctypes.byref(ap), *tail), word)
            assert untouched(out) and untouched(mom) and (spp == -7).all()


def dist_refuses(dist1, sc, cam, p, word):
    image = np.full((p.ny, p.nx, 3), SENTINEL, np.float32)
    refused(rtnw.lib().rt_dist_render(dist1.handle, sc.handle, ctypes.byref(cam.desc), ctypes.byref(p), image.ctypes.data,
                                      None), word)
    assert (image == SENTINEL).all()


@pytest.mark.parametrize("flags", [0, SUM_IN])
@pytest.mark.parametrize("total", [2 ** 32, 2 ** 32 + 5])
def test_sample_ranges_past_the_last_index_are_refused(total, flags, dist1):
    """sample_offset + spp = 2^32 (whose uint32_t is 0: under RT_FLAG_SUM_IN the mean's divisor)
    and 2^32 + 5: RT_ERR_INVALID, the outputs untouched; one sample less is legal."""
    case = Case("random_scene", LC.FAR, spp=LC.LAST_SPP, chunk=1, sample_offset=total - LC.LAST_SPP)
    sc, cam = frame(case.scene)
    every_entry_point_refuses(sc, cam, case.params(flags=flags), case.rect, "sample_offset", adaptive=False)
    if not flags:   # (rt_dist_render takes no running sums: test_dist.py)
        small = rtnw.RenderParams(16, 16, LC.LAST_SPP, max_depth=8, background=rtnw.RT_BG_SKY, seed=1, chunk=1,
                                  sample_offset=total - LC.LAST_SPP)
        dist_refuses(dist1, sc, rtnw.Camera.preset("random", 16, 16), small, "sample_offset")
        small.sample_offset = LC.LAST - LC.LAST_SPP   # the communicator is still usable, at the last legal range
        img, st = dist1.render(sc, rtnw.Camera.preset("random", 16, 16), small)
        assert st["samples"] == 16 * 16 * LC.LAST_SPP and np.isfinite(img).all() and (img > 0).all()


# ------------------------------------------------------------------ 4. seeds and chunks
@pytest.mark.parametrize("seed", LC.SEEDS)
def test_extreme_seeds_match_the_oracle(seed):
    f = LC.FRAMES[LC.SEED_SCENE]
    nx, ny = LC.SEED_NX, LC.SEED_NY
    p = rtnw.RenderParams(nx, ny, LC.SEED_SPP, max_depth=f["max_depth"], background=LC.BG[f["background"]], chunk=2, seed=seed)
    g = _scene(LC.SEED_SCENE).render_tile(rtnw.Camera.preset(f["camera"], nx, ny), p, 0, 0, nx, ny)
    o = O.render(LC.seed_spec(seed, threads=THREADS))[0]
    check(Case(LC.SEED_SCENE, (0, 0, nx, ny), seed=seed), g, o)


@pytest.mark.parametrize("case", LC.CHUNK_CASES, **ids)
def test_chunks_larger_than_spp_match_the_oracle(case):
    """chunk = 2^31 - 1 and chunk = spp + 1: one work item per pixel holds all three samples."""
    g, st = gpu(case, stats=True)
    assert st["chunk"] == case.chunk and st["batches"] == 1 and st["samples"] == T * T * case.spp
    check(case, g, oracle(case))
    assert same(g, gpu(case, chunk=case.spp))   # as one partial sum of exactly spp samples


# ------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("nx,ny", [(N + 1, N), (N, N + 1), (N + 1, N + 1)])
def test_frames_above_65535_are_refused(nx, ny, dist1):
    sc = _scene("random_scene")
    cam = rtnw.Camera.preset("random", nx, ny)
    p = rtnw.RenderParams(nx, ny, 2, max_depth=8, background=rtnw.RT_BG_SKY, seed=1, chunk=1)
    every_entry_point_refuses(sc, cam, p, (nx - T, ny - T, T, T), "65535", adaptive=True)
    for snx, sny in ((N + 1, 1), (1, N + 1)):   # (frames whose image the root can hold)
        q = rtnw.RenderParams(snx, sny, 2, max_depth=8, background=rtnw.RT_BG_SKY, seed=1, chunk=1)
        dist_refuses(dist1, sc, rtnw.Camera.preset("random", snx, sny), q, "rt_rank_tiles")
