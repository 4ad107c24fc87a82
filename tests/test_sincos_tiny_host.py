"""The fix-up for |y| < 2^-12 inside the render kernels' fast sin/cos (ptmi::sincos_quadrant_tiny, csrc/ptmi_core.h), on the CPU.  A
stand-alone program (tests/cxx/sincos_tiny_main.cpp, its own main) is compiled with AddressSanitizer + UndefinedBehaviorSanitizer, the
runtime linked statically, contraction off as in the library's build, and run directly: nothing is preloaded, nothing sanitized is loaded
into Python, no GPU.  It compares the per-angle form bitwise with the literal sincos_t<false> for every pattern within 65 536 of +-0,
of +-2^-12 and of the denormal boundary and for every 1 024th pattern below 2^-12 of both signs, and checks the new guards against the
old ones."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import test_host_sanitized as hs  # noqa: E402


@hs.needs_asan
def test_the_tiny_fixup_equals_the_literal_form_under_asan_and_ubsan():
    pkg = graft.load_package()
    b = pkg._build
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(b.hipcc_path()))), "include")
    out_dir = os.path.join(hs.OUT, "static")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "sincos_tiny")
    cmd = [hs.CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libsan", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I", rocm_include, "-I", b.CSRC,
           os.path.join(ROOT, "tests", "cxx", "sincos_tiny_main.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([out], capture_output=True, text=True, env=env, timeout=300)
    text = run.stdout + run.stderr
    print(run.stdout)
    assert "runtime error" not in text and "AddressSanitizer" not in text and "LeakSanitizer" not in text, text[-4000:]
    assert run.returncode == 0 and "SINCOS_TINY_OK" in run.stdout, text[-4000:]
