"""The quadrant-by-comparison sin/cos of the render kernels (ptmi::sincos_quadrant, csrc/ptmi_core.h), on the CPU: the stand-alone host
program tools/verify_sincos_quadrant.cpp re-derives the four thresholds from reduce_fast's literal text (every binary32 with |y| < 4,
the quadrant must be monotone) and refuses to pass unless they are the header's constants, checks what sincos_quadrant_covers accepts,
and compares the form bitwise with the literal sincos_t<false> for every 4096th covered pattern and for all within 65 536 ulps of
+-T1, +-T2, +-2^-12 and +-0.  The sweep over every covered pattern is the tool's --full mode (and, on the device,
tools/verify_sincos_quadrant.hip: profiles/verify_sincos_quadrant.txt)."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_thresholds_rederived_and_core_equals_the_literal_form(pkg, tmp_path):
    b = pkg._build
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(b.hipcc_path()))), "include")
    exe = str(tmp_path / "verify_sincos_quadrant")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
           "-I", rocm_include, "-I", b.CSRC, os.path.join(ROOT, "tools", "verify_sincos_quadrant.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    env = dict(os.environ, OMP_NUM_THREADS=str(max(1, min(16, os.cpu_count() or 1))))
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    print(res.stdout)
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["thresholds_equal_header"] and out["quadrant_monotone"], out
    assert (out["T1p"], out["T2p"], out["T1n"], out["T2n"]) == ("0x3f490fdb", "0x4016cbe4", "0xbf490fdd", "0xc016cbe5")
    assert out["cover_errors"] == 0 and out["mismatches"] == 0, out
    # every 4096th covered pattern of both signs (2^-12 .. T2: 0x696cbe4 patterns a side) and the windows' covered parts
    assert out["checked"] >= 2 * (0x696cbe4 >> 12) + 4 * 65536
    assert res.returncode == 0 and out["ok"]
