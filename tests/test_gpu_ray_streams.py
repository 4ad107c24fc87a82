"""Render Streams along a caller's own rays on the device: ptmi_trace_streams_device and ptmi_trace_streams_indexed_device through
Context.trace_streams with torch tensors, on the context's stream -- the depth-first walk of every sample's ray tree, GLASS included, for
rays a camera did not make, held to the contract's plain-C reference bit for bit, colours by words.

The torch part runs in ONE child process (tests/ray_streams_driver.py), where torch brings the runtime up before the library is loaded, as
in bench.py -- the convention of tests/test_gpu_ray_paths.py; it is a fresh process and nothing is exec'd.  The child makes the scenes of
tests/ray_streams_inputs.py, one per kernel with and without GLASS, and the drop scene, with the batches tests/test_ray_streams_inputs.py
holds to reaching every shape of the walk, and prints one line per case; each test below reads its own line.  The child runs under one
time limit; a runtime error ends it, and the cases behind it count as not run (a failure).

The cases are those of the driver's docstrings:
  1 colour, seed and d_lost == the reference: every scene, 1 and 3 spp, caps 2, 3, 12 and 65536, a zero start colour and one with -0.0, NaN
    and inf; an explicit PTMI_SEED_KEEP_ACCUMULATOR on the scenes without glass as well
  2 n = 0, 1, 63, 64, 65, 257; every array aligned and 4 bytes off; guard words around colour, seeds, d_lost and the workspace
  3 a camera's primary rays + path_seeds + a zero colour == init_output + render(STREAMS, PTMI_FORM_PIXEL) on seven planes, one scene per kind
    with and without GLASS, both seed rules; d_lost == the statistics' truncated and dropped deltas
  4 3 spp in one call == three calls of 1 spp
  5 through ray_order's permutation the plain words; through a live-style list with -1 padding the named rays alone
  6 the drop scene: dropped > 0, the reference's count
  7 a render's planes, the statistics and the next render are what they are without the calls; a set_scene right behind a call
  8 the refusals through the raw handle, nothing written; d_work NULL accepted without GLASS"""
import os
import subprocess
import sys
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ray_streams_driver as driver  # noqa: E402

pytestmark = pytest.mark.gpu
LIMIT = 420                                  # seconds for the child: process start, torch, nine scenes, the references, eight cases


@pytest.fixture(scope="module")
def outcome(pkg, ora, tmp_path_factory):
    """{case: None if it passed, else why not} from one run of the child"""
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, os.path.join(HERE, "ray_streams_driver.py"), str(tmp_path_factory.mktemp("ray_streams"))],
                         capture_output=True, text=True, timeout=LIMIT)
    print(res.stdout)
    print("ray_streams_driver: %.1f s, exit %d" % (time.perf_counter() - t0, res.returncode))
    tail = (res.stdout + res.stderr)[-3000:]
    found = {}
    for line in res.stdout.splitlines():
        if line.startswith("ok "):
            found[line[3:]] = None
        elif line.startswith("FAILED "):
            name, _, why = line[7:].partition(": ")
            found[name] = why
    return {name: found.get(name, "not run: the child ended with %d before it\n%s" % (res.returncode, tail)) for name in driver.CASES}


@pytest.mark.parametrize("case", driver.CASES)
def test_streams_along_a_callers_rays(outcome, case):
    assert outcome[case] is None, outcome[case]
