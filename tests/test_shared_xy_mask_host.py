"""shared_xy_mask (csrc/ptmi_share.h): which spheres of a linear scene repeat their predecessor's (cx, cy) bits, so that check_hit keeps
the x-y terms of the sphere test (SphereShare::kXY, csrc/ptmi_device.h).  A stand-alone program (tests/cxx/shared_xy_mask_main.cpp, its
own main) is compiled with AddressSanitizer + UndefinedBehaviorSanitizer, the runtime linked statically, and run directly: nothing is
preloaded, nothing sanitized is loaded into Python, no GPU.  It checks the mask of S16's layout, of runs of 1 to 5 at every index of 1 to
9 spheres, of neighbours equal in one coordinate only, of +0 / -0, of NaN patterns, and of 0, 1, 64 and 65 spheres in exactly fitting arrays."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import test_host_sanitized as hs  # noqa: E402


@hs.needs_asan
def test_the_mask_function_is_right_and_clean_under_asan_and_ubsan():
    pkg = graft.load_package()
    out_dir = os.path.join(hs.OUT, "static")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "shared_xy_mask")
    cmd = [hs.CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan",
           "-fno-omit-frame-pointer", "-I", pkg._build.CSRC, os.path.join(ROOT, "tests", "cxx", "shared_xy_mask_main.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([out], capture_output=True, text=True, env=env, timeout=120)
    text = run.stdout + run.stderr
    assert "runtime error" not in text and "AddressSanitizer" not in text and "LeakSanitizer" not in text, text[-4000:]
    assert run.returncode == 0 and "SHARED_XY_MASK_OK" in run.stdout, text[-4000:]


def test_the_build_id_sees_the_header():
    b = graft.load_package()._build
    assert "ptmi_share.h" in b.HEADERS
