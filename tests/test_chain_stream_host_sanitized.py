"""The chained closure (csrc/ptmi_chain.cpp) and the stream form's host loop (csrc/ptmi_stream_call.cpp) under AddressSanitizer +
UndefinedBehaviorSanitizer, without a GPU: a stand-alone program (tests/cxx/chain_stream_hostsan.cpp, its own main) linked against the
library with instrumented host code and against the HIP stand-in (tests/cxx/hip_stub.cpp), and run directly in the environment as it is --
nothing is preloaded, nothing is loaded into Python.  The sanitizer's runtime is linked STATICALLY into the program, as
tests/test_bvh_update_host_sanitized.py does it.

`plain`: one fixed scenario through every branch of the chain's block hand-out and of the stream form's overflow levels and redos; after every
ABI call the program prints what the call did to the runtime (calls per kind, live device blocks, ptmi_chain_info, the launches and memsets in
order).  tests/golden/chain_stream_calls.txt is that record of the commit before the two units were cut out of ptmi_api.cpp: the success path
makes the same runtime calls, line for line.  `walk`: every runtime call of the chain calls and of one redone stream-form call fails in turn."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import test_host_sanitized as hs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "chain_stream_calls.txt")


def build_program(root=ROOT, pkg=None, out_dir=None, program="chain_stream_hostsan"):
    """tests/cxx/<program>.cpp against the library of the checkout at `root` (the golden record is made from the parent commit's)."""
    pkg = pkg or graft.load_package()
    out_dir = out_dir or os.path.join(hs.OUT, "static")
    stub = hs.build_stub(out=os.path.join(out_dir, "libhipstub_plain.so"), sanitize=None)
    flags = [f for f in hs.HOST_SANITIZE if f != "-shared-libasan"]          # instrumented host code, no runtime of its own
    lib = pkg._build.build_lib(out=os.path.join(out_dir, "libptmi_sanitized_static.so"), extra_flags=flags)
    out = os.path.join(out_dir, program)
    cmd = [hs.CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(root, "include"),
           "-I", os.path.join(root, "haskell-path-tracer_amd", "csrc"),
           os.path.join(ROOT, "tests", "cxx", program + ".cpp"), "-o", out,
           stub, lib, "-Wl,-rpath," + out_dir]                # (the stand-in BEFORE the library: its hip* symbols win)
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    return out


def run_program(program, mode):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([program, mode], capture_output=True, text=True, env=env, timeout=600)
    text = run.stdout + run.stderr
    assert "runtime error" not in text and "AddressSanitizer" not in text and "HIPSTUB:" not in text, text[-4000:]
    assert run.returncode == 0 and "CHAIN_STREAM_HOSTSAN_OK" in run.stdout, text[-4000:]
    return run.stdout


@hs.needs_asan
def test_the_chain_and_the_stream_form_make_the_recorded_runtime_calls_and_survive_every_failure():
    program = build_program()
    got = run_program(program, "plain").splitlines()
    with open(GOLDEN) as fh:
        want = fh.read().splitlines()
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "line %d: %r, recorded %r" % (i + 1, a, b)
    assert len(got) == len(want), "%d lines, %d recorded" % (len(got), len(want))
    # The walk fails every runtime call in turn, so it has at least as many failure points as the record counts calls (the six numbers after
    # `calls`) for the chain calls up to the one that injects a failure of its own -- the walk runs those exactly as recorded -- and for the
    # stream-form call that is redone once.
    calls = lambda line: sum(int(v) for v in line.split(" calls ")[1].split(" live ")[0].split())      # noqa: E731
    own = next(i for i, line in enumerate(want) if "the allocation within the budget failing" in line)
    floor = sum(calls(line) for line in want[:own] if " calls " in line) + calls(next(line for line in want if line.startswith("children dropped")))
    walked = run_program(program, "walk")
    points = int(re.search(r"walk: (\d+) failure points", walked).group(1))
    assert floor >= 80 and points >= floor, (points, floor)
