"""The limit cases of tests/limit_cases.py, the CPU side: every case can fail.

tests/test_gpu_limits.py compares the kernels with the oracle on far tiles of a 65535 x 65535
frame, at the last sample indices and under extreme seeds and chunks.  A tile that far out
sees almost one direction; if its pixels were black or equal, a wrong pixel key or sample
index would render the same image.  So each case's ORACLE image is held to
limit_cases.powerful (at least half the pixels nonzero, no two nonzero pixels bit-equal) —
the strips to powerful_strip, for the reason limit_cases.py gives — before any GPU run.
"""
import os

import numpy as np
import pytest

import limit_cases as LC
import oracle as O
from conftest import ROOT
from test_adaptive_guard_spec import count_map, predict_guarded

THREADS = min(16, os.cpu_count() or 1)
ids = dict(ids=lambda c: c.name)


def test_the_case_names_are_distinct():
    names = [c.name for c in LC.POWER_CASES]
    assert len(set(names)) == len(names)


def test_the_tiles_are_where_the_index_arithmetic_changes():
    """The centre tile holds the first pixel whose key j * nx + x needs bit 31 and the last that
    does not; the corner tiles and pixels touch x = nx - 1, y = ny - 1 and j = ny - 1; from
    j = 32769 on the product j * nx alone is past INT_MAX."""
    N = LC.N
    x0, y0, w, h = LC.CENTRE
    keys = [(N - 1 - y) * N + x for y in range(y0, y0 + h) for x in range(x0, x0 + w)]
    assert min(keys) < 2 ** 31 - 1 and 2 ** 31 - 1 in keys and 2 ** 31 in keys and max(keys) > 2 ** 31
    assert 32768 * N <= 2 ** 31 - 1 < 32769 * N
    assert max((N - 1 - y) * N + x for x, y, _, _ in LC.PIXELS) == N * N - 1 < 2 ** 32
    for x0, y0, w, h in LC.CORNERS + (LC.CENTRE, LC.CENTRE_LEVEL) + LC.PIXELS + LC.STRIPS:
        assert 0 <= x0 and 0 <= y0 and x0 + w <= N and y0 + h <= N
    assert {(r[0] + r[2], r[1] + r[3]) for r in LC.CORNERS} >= {(N, N), (N, LC.T), (LC.T, N)}
    # the level cameras' centre tile: the same crossing in its bottom row, and not image row 32767
    x0, y0, w, h = LC.CENTRE_LEVEL
    level = [(N - 1 - y) * N + x for y in range(y0, y0 + h) for x in range(x0, x0 + w)]
    assert 2 ** 31 - 1 in level and 2 ** 31 in level and y0 + h == 32767 and N - 1 - (y0 + h - 1) == 32768
    assert all(c.sample_offset + c.spp == LC.LAST for c in LC.LAST_CASES + LC.SUM_IN_CASES)


@pytest.mark.parametrize("case", LC.POWER_CASES, **ids)
def test_the_oracles_image_of_the_case_can_tell_pixels_apart(case):
    img, axis = LC.oracle_image(case, THREADS)
    share, equal, unique = LC.power(img)
    print(f"{case.name}: nonzero {share:.4f}, bit-equal nonzero pixels {equal}, nonzero and unique {unique:.4f}, "
          f"pixels with an axis-parallel ray {int(axis.sum())}")
    assert np.isfinite(img).all()
    assert LC.powerful_strip(img) if case.strip else LC.powerful(img)
    # rays exactly parallel to an axis are outside the parity contract: none at any bounce of a
    # tile's paths, and in the strips exactly the few pixels the table lists
    assert int(axis.sum()) == LC.AXIS_PIXELS.get((case.scene, case.rect), 0)


def test_a_strips_image_does_not_depend_on_the_oracles_threads():
    case = next(c for c in LC.FRAME_CASES if c.strip and c.scene == "cornell_box" and c.rect[3] == 1)
    one, many = LC.oracle_image(case, 1), LC.oracle_image(case, THREADS)
    assert np.array_equal(one[0].view(np.uint32), many[0].view(np.uint32)) and np.array_equal(one[1], many[1])


@pytest.mark.parametrize("seed", LC.SEEDS)
def test_the_seed_frames_can_tell_pixels_apart(seed):
    axis = np.zeros((LC.SEED_NY, LC.SEED_NX), np.uint8)
    img = O.render(LC.seed_spec(seed, threads=THREADS), axis=axis)[0]
    print(f"seed {seed:#x}: {LC.power(img)}")
    assert LC.powerful(img) and not axis.any()


def test_the_extreme_seeds_give_different_images():
    a, b, c = (O.render(LC.seed_spec(s, threads=THREADS))[0] for s in LC.SEEDS)
    for u, v in ((a, b), (a, c), (b, c)):
        assert not np.array_equal(u, v)


def oracle_samples(case, n):
    """[n, h, w, 3]: the oracle's one-sample images of the case's tile, sample k at index k."""
    return np.stack([O.render(case.spec(ns=1, chunk=1, sample_offset=k, threads=THREADS))[0] for k in range(n)])


def test_the_level_cameras_centre_row_is_why_its_centre_tile_ends_above_it():
    """In image row 32767 of a level camera's frame the primary rays have direction.y == 0."""
    axis = LC.oracle_image(LC.Case("cornell_box", LC.CENTRE), THREADS)[1]
    assert axis[4].sum() == 7 and not axis[:4].any()   # 7 of that row's 8 pixels at 4 spp


@pytest.mark.parametrize("rect", LC.entry_tiles(LC.ADAPTIVE_SCENE))
def test_the_adaptive_maps_of_the_far_tiles_are_not_trivial(rect):
    """The rule of tests/test_adaptive_guard_spec.py on the oracle's samples of the tile: pixels
    stop at more than one count without a guard, and radius 2 holds some of them back."""
    a = LC.ADAPTIVE
    one = oracle_samples(LC.Case(LC.ADAPTIVE_SCENE, rect, chunk=1), a["cap"])
    spp0, _, _ = predict_guarded(one, a["mn"], a["step"], a["cap"], a["tol"], a["floor"], 0)
    spp2, _, held = predict_guarded(one, a["mn"], a["step"], a["cap"], a["tol"], a["floor"], 2)
    print(f"{rect}: r 0 {count_map(spp0)}, r 2 {count_map(spp2)}, held {int(held.sum())}")
    assert not LC.oracle_image(LC.Case(LC.ADAPTIVE_SCENE, rect, spp=a["cap"], chunk=1), THREADS)[1].any()
    assert len(count_map(spp0)) >= 2
    assert (spp2 >= spp0).all() and (spp2 > spp0).any()


@pytest.mark.parametrize("case", LC.FEATURE_CASES, **ids)
def test_the_feature_cases_have_surfaces_in_view(case):
    """Every sample of a feature case hits a surface, at more than half as many depths as pixels:
    a wrong x0 + p % w or pixel key moves a pixel's depth."""
    import rtnw
    fh = O.first_hits_desc(rtnw.SceneDesc.builtin(case.scene), case.camera(), case.desc_spec(threads=THREADS))
    o = O.feature_means(fh)
    assert (o["coverage"] == 1).all()
    assert len(np.unique(o["depth"].view(np.uint32))) > LC.T * LC.T // 2


@pytest.mark.parametrize("field", ["nx", "ny"])
def test_the_adaptive_entry_points_refuse_a_frame_above_65535_before_the_device(field):
    """With their other argument checks: a null scene is only reached by a legal frame."""
    from test_adaptive_guard_spec import _guarded
    from test_adaptive_spec import _adaptive, _good
    for call in (_adaptive, lambda p, a: _guarded(p, a, 1)):
        p, a = _good()
        setattr(p, field, 65535)
        assert "null scene" in call(p, a)[1]
        setattr(p, field, 65536)
        rc, msg = call(p, a)
        assert rc == -1 and "65535" in msg and "null scene" not in msg, msg


def test_the_header_states_the_limits():
    text = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    for words in ("1..65535", "(uint64_t)sample_offset + spp <= 0xFFFFFFFF", "any positive int32"):
        assert words in text, words
