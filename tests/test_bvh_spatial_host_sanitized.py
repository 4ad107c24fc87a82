"""ptmi_bvh_layout_spatial, the host twin of the spatial sphere build, under AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU:
a stand-alone program (tests/cxx/bvh_spatial_hostsan.cpp, its own main) compiled together with the twin's unit, csrc/ptmi_bvh.cpp --
pure host code that calls no runtime (the HIP headers it sees declare types only) -- with the sanitizers' runtime linked statically, and run directly in the environment as it is:
nothing is preloaded, nothing sanitized is loaded into Python.  The program drives the twin over the counts and families of
tests/test_bvh_spatial_layout.py in exactly fitting buffers, and over its refusals."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import test_host_sanitized as hs  # noqa: E402


@hs.needs_asan
def test_the_spatial_twin_is_clean_under_asan_and_ubsan():
    pkg = graft.load_package()
    out_dir = os.path.join(hs.OUT, "static")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "bvh_spatial_hostsan")
    cmd = [hs.CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libsan", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cxx", "bvh_spatial_hostsan.cpp"), os.path.join(pkg._build.CSRC, "ptmi_bvh.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([out], capture_output=True, text=True, env=env, timeout=600)
    text = run.stdout + run.stderr
    assert "runtime error" not in text and "AddressSanitizer" not in text and "LeakSanitizer" not in text, text[-4000:]
    assert run.returncode == 0 and "BVH_SPATIAL_HOSTSAN_OK" in run.stdout, text[-4000:]
