"""The ball waves' fused in-ball step (rt_megakernel.h stage 3) on the generated ball_* scenes of
tests/gen_scenes.py: the configurations final() never shows it (one medium, the dense medium
listed second, both media scattering inside the ball, a cell primitive beyond the ball's exit, a
full cell with a moving sphere, camera rays that start inside the ball with a time of their own,
a thin, a solid and a negative-radius ball), and scenes it must stay away from.

test_gpu_generated.py already holds every case's default image to the oracle; here every setting
of the step must reproduce that image bit for bit, rt_stats' ball_fused_scatters and
ball_fused_declined say whether a trip ran at all (so that "bitwise equal" does not compare the
generic stages with themselves), and the parameter edges are held to the oracle again with the
step forced on.  No tolerance of its own: bitwise, or test_gpu_generated.check.
"""
import dataclasses

import numpy as np
import pytest

import gen_scenes as G
import oracle as O
import rtnw
import test_gpu_generated as TG
from test_ball_fast import KNOBS, TOTALS

pytestmark = pytest.mark.gpu

BALL = [c for c in G.CASES if c.name.startswith("ball_")]
EDGE = [G.BY_NAME["ball_dense_second"], G.BY_NAME["ball_full_cell"]]
FORCED = {"RTNW_BALL_FAST": 1, "RTNW_BALL_WAVES": 16}   # a trip for a single eligible lane, every wave a ball wave
SCATTERS = {"ball_" + v for v in ("one_medium", "dense_first", "dense_second", "full_cell", "negative_radius", "solid", "camera_inside")}
DECLINES = {"ball_" + v for v in ("thin", "full_cell", "in_fog_on_ground", "camera_inside")}
ids = TG.ids
bits = TG.bits


def render(monkeypatch, c, env, *, rect=None, stats=False, **kw):
    """The case's job on its scene of test_gpu_generated.built(), under `env` alone of the ball knobs."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    x0, y0, w, h = rect if rect else (0, 0, c.nx, c.ny)
    sc = TG.built(G.BY_NAME[c.name])[2]
    return sc.render_tile(c.camera(), TG.params(c, **kw), x0, y0, w, h, stats=stats)


def oracle(c, **kw):
    return O.render_desc(G.build(c)[0], c.camera(), TG.spec(c, **kw))


@pytest.mark.parametrize("case", BALL, **ids)
def test_every_setting_gives_the_default_image(monkeypatch, case):
    img = TG.built(case)[3]
    assert np.isfinite(img).all() and img.max() > 0
    envs = [{"RTNW_BALL_WAVES": 0}]
    for fast in (0, 1, 64, None):
        for waves in (None, 16):
            envs.append({k: v for k, v in (("RTNW_BALL_FAST", fast), ("RTNW_BALL_WAVES", waves)) if v is not None})
    for env in envs:
        got = render(monkeypatch, case, env)
        differing = int(np.sum(np.any(bits(got) != bits(img), axis=-1)))
        print(f"{case.name} {env}: {differing} of {case.nx * case.ny} pixels differ")
        assert np.array_equal(bits(got), bits(img)), env


@pytest.mark.parametrize("case", BALL, **ids)
def test_the_counters_say_whether_the_step_ran(monkeypatch, case):
    """RT_FLAG_COUNT with a trip for any eligible lane in every wave: the default image, the
    oracle's segments, and the two counters positive exactly where the scene is built for it."""
    img = TG.built(case)[3]
    got, st = render(monkeypatch, case, FORCED, stats=True, flags=rtnw.RT_FLAG_COUNT)
    fused, declined = st["ball_fused_scatters"], st["ball_fused_declined"]
    print(f"{case.name} forced: ball_fused_scatters {fused:.0f} ball_fused_declined {declined:.0f} lane_scatters "
          f"{st['lane_scatters']:.0f} segments {st['segments']:.0f}")
    assert np.array_equal(bits(got), bits(img))
    assert st["samples"] == case.nx * case.ny * case.spp
    assert st["segments"] == oracle(case)[1]["segments"]
    assert 0 <= fused <= st["lane_scatters"]
    if case.name in SCATTERS:
        assert fused > 0
    if case.name in DECLINES:
        assert declined > 0
    if case.name[5:] in G.BALL_DECLINE:
        assert fused == 0 and declined == 0
    else:   # the step switched off
        _, off = render(monkeypatch, case, dict(FORCED, RTNW_BALL_FAST=0), stats=True, flags=rtnw.RT_FLAG_COUNT)
        assert off["ball_fused_scatters"] == 0 and off["ball_fused_declined"] == 0
        assert off["segments"] == st["segments"]
    # without RT_FLAG_COUNT both stay 0
    _, plain = render(monkeypatch, case, FORCED, stats=True)
    assert plain["ball_fused_scatters"] == 0 and plain["ball_fused_declined"] == 0


@pytest.mark.parametrize("case", EDGE, **ids)
def test_path_totals_do_not_depend_on_the_step(monkeypatch, case):
    _, off = render(monkeypatch, case, dict(FORCED, RTNW_BALL_FAST=0), stats=True, flags=rtnw.RT_FLAG_COUNT)
    _, on = render(monkeypatch, case, FORCED, stats=True, flags=rtnw.RT_FLAG_COUNT)
    for k in TOTALS:
        print(f"{case.name} {k}: {on[k]:.0f} (off {off[k]:.0f})")
    assert on["ball_fused_scatters"] > 0 and off["medium_tests"] > 0 and off["lane_scatters"] > 0
    for k in TOTALS:
        assert on[k] == off[k], k


def edges(c):
    """(label, case with the job's parameters, render_tile's keywords, the oracle spec's)."""
    mfp = 1.0 / G.BALL_DENSITY[c.name[5:]]
    out = [(f"max_depth {k}", dataclasses.replace(c, max_depth=k), {}, {}) for k in (1, 2, 3)]
    out += [(f"t_min {t:g}", c, dict(t_min=t), dict(tmin=t)) for t in (0.25 * mfp, 2 * G.BALL_R)]
    out += [(f"chunk {k}", c, dict(chunk=k), dict(chunk=k)) for k in (1, 3)]
    return out


@pytest.mark.parametrize("edge", range(7), ids=["max_depth1", "max_depth2", "max_depth3", "t_min_quarter_mfp", "t_min_2R",
                                                  "chunk1", "chunk3"])
@pytest.mark.parametrize("case", EDGE, **ids)
def test_parameter_edges_match_the_oracle(monkeypatch, case, edge):
    """The depth cap and t_min inside the loop, and partial sums carried through fused scatters:
    the step forced on (alone, and in every wave) and the default, each against the oracle."""
    label, c, kw, okw = edges(case)[edge]
    o = oracle(c, **okw)[0]
    for env in ({"RTNW_BALL_FAST": 1}, {}, FORCED):
        TG.check(f"{case.name} {label} {env}", render(monkeypatch, c, env, **kw), o)


BIG = dict(nx=640, ny=480, spp=32)
BIG_RECT = (316, 236, 8, 8)   # on the ball, in the middle of the frame


@pytest.mark.parametrize("case", EDGE, **ids)
def test_the_compiled_threshold_is_reached_and_changes_nothing(monkeypatch, case):
    """No ball knob set: a trip needs the compiled RT_BALL_FAST = 48 eligible lanes in one ball
    wave.  Measured on an MI355X (ball_fused_scatters of dense_second / full_cell): 0 / 0 at
    160 x 120 x 16 spp (307,200 samples, about one per lane of the persistent grid), 0 / 0 at
    320 x 240 x 16 and at 400 x 300 x 32, 27,480,784 / 18,184,311 at 640 x 480 x 32 (9.8 M samples,
    kernel 28 ms), which is therefore the job here; the oracle sees its 8 x 8 crop alone."""
    big = dataclasses.replace(case, **BIG)
    x0, y0, w, h = BIG_RECT
    ref = render(monkeypatch, big, {"RTNW_BALL_WAVES": 0})
    img = render(monkeypatch, big, {})
    assert ref.max() > 0 and np.array_equal(bits(img), bits(ref))
    tile = render(monkeypatch, big, {}, rect=BIG_RECT)
    assert np.array_equal(bits(tile), bits(img[y0:y0 + h, x0:x0 + w]))
    TG.check(f"{case.name} {BIG} crop", tile, oracle(big, rect=BIG_RECT)[0])
    got, st = render(monkeypatch, big, {}, stats=True, flags=rtnw.RT_FLAG_COUNT)
    print(f"{case.name} {BIG}, compiled threshold: ball_fused_scatters {st['ball_fused_scatters']:.0f} "
          f"ball_fused_declined {st['ball_fused_declined']:.0f} lane_scatters {st['lane_scatters']:.0f} "
          f"segments {st['segments']:.0f}")
    assert np.array_equal(bits(got), bits(ref))
    assert 0 < st["ball_fused_scatters"] <= st["lane_scatters"]
