"""The host side of the nearest-primitive query (csrc/ptmi_nearest.cpp -- the two device entries' refusals and the host twin, ptmi_nearest --
and the launcher of csrc/ptmi_nearest.hip) under AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU: a stand-alone program
(tests/cxx/nearest_hostsan.cpp, its own main) linked against the library with instrumented host code and against the HIP stand-in
(tests/cxx/hip_stub.cpp), and run directly in the environment as it is -- nothing is preloaded, nothing is loaded into Python.  The
sanitizer's runtime is linked STATICALLY into the program, as in tests/test_multi_hit_host_sanitized.py.  The program provokes every
refusal of the two entries on a linear, a BVH and a mesh scene, calls them with and without r_max and locations on aligned and misaligned
arrays, lets every runtime call of the entries fail in turn, and runs the twin: its refusals, known answers, non-finite points, every
family of r_max, and a batch large enough for its worker threads."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import test_host_sanitized as hs  # noqa: E402


@hs.needs_asan
def test_the_nearest_entries_and_the_twin_are_clean_at_every_refusal_and_failure_point():
    pkg = graft.load_package()
    out_dir = os.path.join(hs.OUT, "static")
    stub = hs.build_stub(out=os.path.join(out_dir, "libhipstub_plain.so"), sanitize=None)
    flags = [f for f in hs.HOST_SANITIZE if f != "-shared-libasan"]          # instrumented host code, no runtime of its own
    lib = pkg._build.build_lib(out=os.path.join(out_dir, "libptmi_sanitized_static.so"), extra_flags=flags)
    out = os.path.join(out_dir, "nearest_hostsan")
    cmd = [hs.CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cxx", "nearest_hostsan.cpp"), "-o", out,
           stub, lib, "-Wl,-rpath," + out_dir]                # (the stand-in BEFORE the library: its hip* symbols win)
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([out], capture_output=True, text=True, env=env, timeout=600)
    text = run.stdout + run.stderr
    assert "runtime error" not in text and "AddressSanitizer" not in text and "HIPSTUB:" not in text, text[-4000:]
    assert run.returncode == 0 and "NEAREST_HOSTSAN_OK" in run.stdout, text[-4000:]
