"""The k nearest hits along a caller's own rays on the device: ptmi_trace_rays_multi_device and ptmi_trace_rays_multi_indexed_device
through Context.trace_rays_multi with torch tensors, on the context's stream.

The torch part runs in ONE child process (tests/multi_hit_driver.py), where torch brings the runtime up before the library is loaded --
the convention of tests/test_gpu_ray_query.py; it is a fresh process and nothing is exec'd.  The child makes that test's five scene kinds,
each extended by a stack (tests/multi_hit_rays.py: a row of 24 spheres, for the mesh scene also 24 quads, every eighth duplicated; 512 of
the 4 096 rays run down it, 384 cross it and 128 pass beside it), checks on the specification alone (tests/cxx/multi_hit_reference.c, by
enumeration) that every comparison has enough rays with more than k hits, with fewer, with none, with ties and outside what the walk
serves, and prints one line per case; each test below reads its own line.  The child runs under one time limit; a runtime error ends it,
and the cases behind it count as not run (a failure).

The cases are those of the driver's docstrings:
  1 (t, idx, count) == the specification on every scene kind, k = 1, 2, 3, 4, 5, 8, 15, 16, t_max absent and from every family aimed at
    the 1st, the k-th and the (k+1)-th hit
  2 n = 0, 1, 63, 64, 65, 257, 4 096; every array 16-byte aligned and 4 bytes off; guard words; unused slots exactly (0, -1)
  3 column 0 at k = 1 is trace_rays, count > 0 at k = 1 is occluded, over the rays without a NaN key
  4 every listed t is the point queries' distance to that primitive, on the linear scenes
  5 the indexed entry: ray_order's order, a live list with m < n, entries outside [0, n); unnamed rows untouched
  6 on torch's non-default stream, read after that stream alone is synchronised
  7 after update_spheres / set_mesh_triangles from device tensors, against a context set afresh and the specification
  8 the refusals, through the raw library handle; nothing written
  9 a render between two queries equals a render without them on all seven planes, statistics included
 10 scene data that is not finite: the specification's answers, no NaN or inf listed
t is compared as a number, idx and count exactly (multi_hit_rays.rows_differ says why: the oracle's sphere distance is +0 where the
device's is -0 for a ray that starts on the sphere); against device functions (cases 3, 4, 7) bit for bit.  The walk beyond these scenes
-- other builders' trees, refitted trees, scales, offsets -- is held to the specification by tests/test_multi_hit_traversal.py."""
import os
import subprocess
import sys
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import multi_hit_driver as driver  # noqa: E402

pytestmark = pytest.mark.gpu
LIMIT = 420                                  # seconds for the child: process start, torch, seven scenes, the references, ten cases


@pytest.fixture(scope="module")
def outcome(pkg, ora, tmp_path_factory):
    """{case: None if it passed, else why not} from one run of the child"""
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, os.path.join(HERE, "multi_hit_driver.py"), str(tmp_path_factory.mktemp("multi_hit"))],
                         capture_output=True, text=True, timeout=LIMIT)
    print(res.stdout)
    print("multi_hit_driver: %.1f s, exit %d" % (time.perf_counter() - t0, res.returncode))
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
def test_multi_hit_on_the_device(outcome, case):
    assert outcome[case] is None, outcome[case]
