"""The nearest-primitive query over a caller's own points on the device: ptmi_nearest_device and ptmi_nearest_indexed_device through
Context.nearest with torch tensors, on the context's stream.

The torch part runs in ONE child process (tests/nearest_driver.py), where torch brings the runtime up before the library is loaded -- the
convention of tests/test_gpu_multi_hit.py; it is a fresh process and nothing is exec'd.  The child makes tests/ray_query_driver.py's five
scene kinds with 4 096 points each, checks on the host twin alone that every comparison has answers of every primitive kind, negative
distances, answers an aimed r_max moves and points the walk does not serve, and prints one line per case; each test below reads its own
line.  The child runs under one time limit; a runtime error ends it, and the cases behind it count as not run (a failure).

The cases are those of the driver's docstrings:
  1 (dist, idx, point) == the host twin bit for bit on every scene kind, r_max absent and aimed at the winner's key
  2 n = 0, 1, 63, 64, 65, 257, 4 096; every array 16-byte aligned and 4 bytes off; guard words
  3 the indexed entry: ray_order's order over [p, 0 0 1], a list with m < n, entries outside [0, n); unnamed rows untouched
  4 on torch's non-default stream, read after that stream alone is synchronised
  5 after update_spheres / set_bvh_spheres / update_mesh_vertices (also one collapsing kept triangles) / set_mesh_triangles from device
    tensors: a context set afresh, the twin
  6 the refusals, through the raw library handle; nothing written
  7 a render between two queries equals a render without them on all seven planes, statistics included
  8 scene data that is not finite, on a linear scene: the twin's answers, no NaN or inf reported
The twin itself is held to exact geometry by tests/test_nearest_exact.py, the walk beyond these scenes -- other builders' trees, refitted
trees, scales, offsets -- to the twin by tests/test_nearest_traversal.py."""
import os
import subprocess
import sys
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nearest_driver as driver  # noqa: E402

pytestmark = pytest.mark.gpu
LIMIT = 300                                  # seconds for the child: process start, torch, six scenes, the twin's answers, eight cases


@pytest.fixture(scope="module")
def outcome(pkg, tmp_path_factory):
    """{case: None if it passed, else why not} from one run of the child"""
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, os.path.join(HERE, "nearest_driver.py"), str(tmp_path_factory.mktemp("nearest"))],
                         capture_output=True, text=True, timeout=LIMIT)
    print(res.stdout)
    print("nearest_driver: %.1f s, exit %d" % (time.perf_counter() - t0, res.returncode))
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
def test_nearest_on_the_device(outcome, case):
    assert outcome[case] is None, outcome[case]
