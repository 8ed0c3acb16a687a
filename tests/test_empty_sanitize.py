"""The empty-pixel classifier (csrc/host/empty_pixels.cpp) with scene lowering, the BVH build and
the scene builders under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU: a stand-alone
program with its own main (tests/native/empty_sanitize.cpp) whose every object carries the
sanitizers; no HIP, no device code.  Leak detection is off: the reference's scene API allocates
its hitables with ``new`` and never frees them, which the host API mirrors on purpose
(tests/test_sanitizers.py)."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "peter-shirley-ray-tracing-the-next-week_amd")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
UNITS = ("empty_pixels.cpp", "scene_lower.cpp", "bvh.cpp", "flatten.cpp", "rtnw.cpp", "png.cpp")


def _run(cmd, **kw):
    out = subprocess.run(cmd, capture_output=True, text=True, **kw)
    assert out.returncode == 0, " ".join(cmd) + "\n" + out.stdout[-4000:] + out.stderr[-4000:]
    return out


def test_empty_pixel_classifier_under_asan_ubsan(tmp_path):
    flags = ["g++", "-std=c++17", "-ffp-contract=off", *SAN, "-I", os.path.join(ROOT, "include"),
             "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(PKG, "csrc", "host")]
    srcs = [os.path.join(PKG, "csrc", "host", u) for u in UNITS] + [os.path.join(ROOT, "tests", "native", "empty_sanitize.cpp")]

    def compile_one(src):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        _run(flags + ["-c", src, "-o", obj])
        return obj

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(compile_one, srcs))
    exe = str(tmp_path / "empty_sanitize")
    _run(["g++", *SAN, *objs, "-o", exe, "-lz"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    out = _run([exe], env=env, timeout=600)
    print(out.stdout[-2000:])
    assert out.stdout.strip().endswith("OK")
