"""Generated-scene GPU parity: every case of tests/gen_scenes.py through rt_scene_create and the
megakernel against the oracle's image of the same descriptor (oracle.render_desc), at the bar
of tests/test_gpu_parity.py (assert_exact: every pixel bitwise where the host libm is the
pinned one; TOL_RMS everywhere), in the kernel's statement and in RT_FLAG_RIGHT_FOLD's; the
image bit-identical under the knobs that move the scene to another code path; the feature pass
against the oracle's first-hit mode; and the path each scene took read off rt_stats, on both
sides of each limit.  tests/test_oracle_desc.py has already shown, without a GPU, that every
case is valid and that its target is in view.
"""
import numpy as np
import pytest

import gen_scenes as G
import oracle as O
import rtnw
from test_gpu_parity import THREADS, TOL_RMS, assert_exact, gamma_rms, pixel_exact

pytestmark = pytest.mark.gpu

BG = {"sky": rtnw.RT_BG_SKY, "black": rtnw.RT_BG_BLACK}
ids = dict(ids=lambda c: c.name)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def params(c, **kw):
    kw.setdefault("chunk", c.spp)
    return rtnw.RenderParams(c.nx, c.ny, c.spp, max_depth=c.max_depth, background=BG[c.background], seed=c.seed, **kw)


def spec(c, **kw):
    kw.setdefault("chunk", c.spp)
    return O.desc_spec(c.nx, c.ny, c.spp, max_depth=c.max_depth, background=c.background, seed=c.seed, threads=THREADS,
                       **kw)


_built = {}


def built(c):
    """(desc, camera, scene, default image, its rt_stats) of a case, made once."""
    if c.name not in _built:
        desc, cam = G.build(c)
        sc = rtnw.Scene(desc)
        img, st = sc.render_tile(cam, params(c), 0, 0, c.nx, c.ny, stats=True)
        _built[c.name] = (desc, cam, sc, img, st)
    return _built[c.name]


def check(what, g, o):
    assert g.shape == o.shape
    assert np.isfinite(g).all() and (g >= 0).all()
    rms, exact = gamma_rms(g, o), pixel_exact(g, o)
    print(f"{what}: gamma RMS {rms}, bit-exact pixels {exact:.4f}")
    assert (rms <= TOL_RMS).all(), rms
    assert_exact(exact)


@pytest.mark.parametrize("case", G.CASES, **ids)
def test_generated_scene_matches_oracle(case):
    """(a) render_tile == oracle.render_desc in the kernel's statement, and the path taken:
    the case's expected rt_stats fields (scan_groups, prescan, lds_level, stack_depth)."""
    desc, cam, _, img, st = built(case)
    check(case.name, img, O.render_desc(desc, cam, spec(case))[0])
    got = {k: st[k] for k in case.expect}
    print(f"{case.name}: scan_groups {st['scan_groups']}, prescan {st['prescan']}, lds_level {st['lds_level']}, "
          f"stack_depth {st['stack_depth']}")
    assert got == {k: float(v) for k, v in case.expect.items()}, (got, case.expect)


@pytest.mark.parametrize("case", G.CASES, **ids)
def test_generated_scene_right_fold_matches_oracle(case):
    """(b) RT_FLAG_RIGHT_FOLD == the oracle's right fold (media after the surface pass); every
    case is built with the default 2-wide BVH."""
    desc, cam, sc, _, _ = built(case)
    g = sc.render_tile(cam, params(case, flags=rtnw.RT_FLAG_RIGHT_FOLD), 0, 0, case.nx, case.ny)
    check(case.name + " right fold", g, O.render_desc(desc, cam, spec(case, forward=False))[0])


def test_generated_scene_chunked_sums_match_oracle():
    """One sample per partial sum and chunks that do not divide spp, on a scene with media."""
    c = G.BY_NAME["boundaries_bvh"]
    desc, cam, sc, _, _ = built(c)
    for chunk in (1, 3):
        g = sc.render_tile(cam, params(c, chunk=chunk), 0, 0, c.nx, c.ny)
        check(f"{c.name} chunk {chunk}", g, O.render_desc(desc, cam, spec(c, chunk=chunk))[0])


def no_sine_prims(desc):
    """[nprims + 1] bool, the last entry for a miss (index -1): the primitive's feature colour
    is computed without sinf — a metal, a dielectric, or a texture tree with no checker or
    noise (texture.h:36, 55 are the only sines)."""
    c = desc.contents

    def plain(t):
        k = c.textures[t].kind
        return k in (0, 3)   # constant, image; a checker calls sinf whatever its leaves, noise too
    out = np.ones(c.nprims + 1, bool)
    for i in range(c.nprims):
        m = c.materials[c.prims[i].material]
        out[i] = m.kind in (1, 2) or plain(m.texture)
    return out


KNOB_FIELD = {"RTNW_SCAN": "scan_groups", "RTNW_LDS_BVH": "lds_level", "RTNW_PRESCAN": "prescan"}


@pytest.mark.parametrize("case", G.CASES, **ids)
def test_generated_scene_is_bitwise_the_same_on_every_path(monkeypatch, case):
    """(c) The image under RTNW_FEAT_ALL=1 (the all-feature kernel) and with each knob that
    applies to the scene switched off at scene creation (RTNW_SCAN, RTNW_LDS_BVH, RTNW_PRESCAN,
    RTNW_CELL = 0): bit for bit the default image, and the knob's rt_stats field shows that the
    other path ran."""
    desc, cam, sc, img, st = built(case)
    monkeypatch.setenv("RTNW_FEAT_ALL", "1")
    full = rtnw.Scene(desc).render_tile(cam, params(case), 0, 0, case.nx, case.ny)
    assert np.array_equal(bits(full), bits(img)), "RTNW_FEAT_ALL=1"
    monkeypatch.delenv("RTNW_FEAT_ALL")
    for knob in case.knobs:
        monkeypatch.setenv(knob, "0")
        other, ost = rtnw.Scene(desc).render_tile(cam, params(case), 0, 0, case.nx, case.ny, stats=True)
        monkeypatch.delenv(knob)
        assert np.array_equal(bits(other), bits(img)), knob
        f = KNOB_FIELD.get(knob)
        if f and st[f] > 0:
            assert ost[f] == 0, (knob, ost[f])
    if len(case.knobs) > 1:   # all of them off together: the plain HBM BVH over every primitive
        for knob in case.knobs:
            monkeypatch.setenv(knob, "0")
        other = rtnw.Scene(desc).render_tile(cam, params(case), 0, 0, case.nx, case.ny)
        assert np.array_equal(bits(other), bits(img)), case.knobs


@pytest.mark.parametrize("case", G.CASES, **ids)
def test_generated_scene_features_match_first_hits(case):
    """(d) rt_render_features against the oracle's first-hit mode, averaged as the feature pass
    averages (oracle.feature_means).  Observed on an MI355X: coverage, albedo, depth and normal
    all bit for bit on every case (share 1.0), so that is what is asserted.  Depth, normal and
    coverage involve no libm call; nor does the albedo of a pixel whose samples all miss or hit
    a metal, a dielectric or a constant or image texture, so those pixels are held bit for bit
    on any host.  Only pixels with a sample on a checker or noise texture (their sines) follow
    test_gpu_parity.assert_exact's policy.  Before prim_record chose a rect's (u, v) axes by
    selects, image_rects and textures_by_kind failed here: an image texture on a yz_rect read
    its texel with the xy_rect's axes in this kernel (not in the megakernel)."""
    desc, cam, sc, _, _ = built(case)
    f = sc.render_features(cam, params(case), 0, 0, case.nx, case.ny)
    fh = O.first_hits_desc(desc, cam, spec(case))
    o = O.feature_means(fh)
    share = {k: float(np.mean(bits(f[k]) == bits(o[k]))) for k in ("coverage", "albedo", "depth", "normal")}
    print(f"{case.name}: bit-exact shares {share}")
    assert o["coverage"].max() > 0
    for k in ("coverage", "depth", "normal"):
        assert np.array_equal(bits(f[k]), bits(o[k])), k
    no_sine = no_sine_prims(desc)[fh["prim"]].all(axis=-1)    # [h, w]: every sample's colour is libm-free
    print(f"{case.name}: {no_sine.mean():.3f} of the pixels' albedos involve no sine")
    assert no_sine.any()
    assert np.array_equal(bits(f["albedo"])[no_sine], bits(o["albedo"])[no_sine])
    if O.host_libm_pinned()[0]:
        assert np.array_equal(bits(f["albedo"]), bits(o["albedo"]))


@pytest.mark.parametrize("name,instanced", [("scan64_mixed", True), ("scan65_mixed", True), ("scan64_spheres", False),
                                            ("prescan8", True), ("prescan1", False), ("chains_long", True),
                                            ("media9_bvh", False), ("cell_near_inst_moving", True),
                                            ("cell_near4", False), ("chains_short", True), ("quad4095", False)])
def test_generated_scene_count_mode(name, instanced):
    """RT_FLAG_COUNT: the counting variant renders the same image, traces the oracle's number
    of segments, and reports tests through an instance chain exactly where the scene has one."""
    c = G.BY_NAME[name]
    desc, cam, sc, img, _ = built(c)
    g, st = sc.render_tile(cam, params(c, flags=rtnw.RT_FLAG_COUNT), 0, 0, c.nx, c.ny, stats=True)
    assert np.array_equal(bits(g), bits(img))
    assert st["samples"] == c.nx * c.ny * c.spp
    assert st["segments"] == O.render_desc(desc, cam, spec(c))[1]["segments"]
    assert (st["instanced_tests"] > 0) == instanced, st["instanced_tests"]
