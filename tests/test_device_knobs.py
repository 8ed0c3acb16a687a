"""Every compile-time knob of the megakernel builds with a non-default value (VERDICT r05
item 6: no `#if RT_*` branch that no test compiles).

Each build is device-only (`--cuda-device-only`) of csrc/hip/rt_kernel_knobs.hip, which
instantiates two variants — final()'s (BVH2 in LDS, media) and cornell_box's (flat scan,
instances) — instead of the whole variant set, so a knob value compiles in ~3 s.  The meta-test below
fails when a new `#if/#ifdef/#ifndef RT_*` appears in the device sources without a
value here.  CPU only: hipcc cross-compiles gfx950 without a GPU."""
import concurrent.futures as cf
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "peter-shirley-ray-tracing-the-next-week_amd")
HIPCC = "/opt/rocm/bin/hipcc"

# knob -> non-default values (the defaults are what every other build compiles)
KNOBS = {
    "RT_READY_BATCH": ["40", "64"],
    "RT_DESCEND_STEPS": ["1", "3"],
    "RT_DRY_LANES": ["0", "64"],
    "RT_WAVES_PER_SIMD": ["3", "5"],       # 5: 96 VGPRs, spills (the occupancy probe)
    "RT_DESCEND_TAIL": ["0", "12"],
    "RT_DESCEND_TAIL2": ["4", "16"],
    "RT_DESCEND_TAIL_DRY": ["4"],
    "RT_LDS_MEDIA": ["1", "16"],
    "RT_SHADE_LEAN": ["0", "127"],          # every lean bit off / on (2 and 8 spill: off by default)
    "RT_BALL_POOL": ["8", "64"],            # the ball waves' path pools (rt_megakernel.h stage 6)
    "RT_NORM_POOL": ["8", "64"],
}


def _build(defs):
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(PKG, "csrc", "host"), "--offload-arch=gfx950",
           "-munsafe-fp-atomics", "--cuda-device-only", "-c", os.path.join(PKG, "csrc", "hip", "rt_kernel_knobs.hip"),
           "-o", os.devnull] + defs
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    return r.returncode, r.stderr[-3000:]


@pytest.mark.skipif(not os.access(HIPCC, os.X_OK), reason="no hipcc")
def test_every_knob_value_compiles():
    jobs = [[f"-D{k}={v}"] if v else [] for k, vals in KNOBS.items() for v in vals]
    with cf.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        results = list(ex.map(_build, jobs))
    failed = [(j, err) for j, (rc, err) in zip(jobs, results) if rc != 0]
    assert not failed, failed[0]


def test_every_device_switch_has_a_value_here():
    switches = set()
    for f in glob.glob(os.path.join(PKG, "csrc", "hip", "*")) + glob.glob(os.path.join(PKG, "csrc", "*.h")):
        for m in re.finditer(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$", open(f).read(), re.M):
            switches.update(re.findall(r"\b(RTL?_[A-Z0-9_]+)\b", m.group(1)))
    assert switches, "no switches found: the source layout changed"
    missing = sorted(switches - set(KNOBS))
    assert not missing, f"compile-time switches without a compiled non-default value: {missing}"
