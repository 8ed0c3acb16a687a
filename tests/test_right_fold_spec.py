"""RT_FLAG_RIGHT_FOLD, the CPU side: the flag's value in both interface files, and the
oracle spec the fold variants of the megakernel implement.

The fold variants compute each sample as main.cpp:36's `emitted + attenuation*color(...)`
from the deepest hit outwards and still evaluate media after the surface pass: the
oracle's `media_after=True, forward=False`.  That spec equals the reference binary's own
framebuffers (tests/golden/ref_*.npy) on every fixture, while the default kernel order
(oracle.kernel_spec: forward throughput) differs from six of them — which is what gives
tests/test_gpu_right_fold.py's bitwise comparison its power to tell the two apart.
"""
import os
import re

import numpy as np
import pytest

import oracle as O
import rtnw
from conftest import GOLDEN, ROOT

FIXTURES = ["c1_random", "c2_cornell", "c3_motion", "c4_final", "smoke", "simple_light", "earth", "edge_empty",
            "edge_single", "edge_degenerate"]
# the fixtures on which forward throughput rounds differently from the right fold
FORWARD_DIFFERS = {"c1_random", "c2_cornell", "c3_motion", "c4_final", "smoke", "edge_degenerate"}
THREADS = min(16, os.cpu_count() or 1)


def header_flags():
    text = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {k: int(v) for k, v in re.findall(r"\b(RT_FLAG_[A-Z_]+)\s*=\s*(\d+)", text)}


def test_flag_value_matches_the_header_and_collides_with_no_other():
    flags = header_flags()
    assert flags["RT_FLAG_RIGHT_FOLD"] == 16 == rtnw.RT_FLAG_RIGHT_FOLD
    assert len(set(flags.values())) == len(flags), flags
    for name, v in flags.items():
        assert v & (v - 1) == 0 and v > 0, (name, v)          # single bits: any two compose
        assert getattr(rtnw, name) == v, name


def test_library_carries_the_fold_unit():
    """The fold variants are a translation unit of their own (csrc/hip/rt_kernel_fold.hip):
    the library a build leaves must have linked its launcher."""
    assert hasattr(rtnw.lib(), "rt_launch_megakernel_fold")


@pytest.mark.parametrize("name", FIXTURES)
def test_right_fold_with_media_after_is_the_reference_framebuffer(golden, name):
    c = golden["counter_fb"][name]
    ref = np.load(os.path.join(GOLDEN, f"ref_{name}.npy"))
    img, _ = O.render(O.RenderSpec(scene=c["scene"], nx=c["nx"], ny=c["ny"], ns=c["ns"], rng="counter", seed=c["seed"],
                                   media_after=True, forward=False, threads=THREADS))
    assert img.shape == ref.shape
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("name", FIXTURES)
def test_kernel_order_differs_from_the_reference_where_recorded(golden, name):
    c = golden["counter_fb"][name]
    ref = np.load(os.path.join(GOLDEN, f"ref_{name}.npy"))
    img, _ = O.render(O.kernel_spec(c["scene"], c["nx"], c["ny"], c["ns"], seed=c["seed"], threads=THREADS))
    differing = int(np.sum(np.any(img.view(np.uint32) != ref.view(np.uint32), axis=-1)))
    print(f"{name}: {differing} of {ref.shape[0] * ref.shape[1]} pixels differ in kernel order")
    if name in FORWARD_DIFFERS:
        assert differing >= 1
