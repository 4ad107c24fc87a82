"""A coherent order for a caller's rays and the ray queries through an index, on the device: ptmi_ray_order_device,
ptmi_trace_rays_indexed_device and ptmi_occluded_indexed_device through Context.ray_order and the index= keyword of Context.trace_rays /
Context.occluded with torch tensors, on the context's stream.

The torch part runs in ONE child process (tests/ray_order_driver.py) under one time limit, as tests/test_gpu_ray_query.py's does; it is a
fresh process and nothing is exec'd.  The child makes that test's five scenes with their 4 096 adversarial rays each (every set ends in
three non-finite rays and one zero-direction ray), takes the plain entries' answers once, and prints one line per case; each test below
reads its own line.  A runtime error ends the child, and the cases behind it count as not run (a failure).

The cases are those of the driver's docstrings:
  1 the device order equals the host twin ptmi_ray_order entry for entry at n = 0, 1, 63, 64, 65, 4 095, 4 096, 4 097 and 12 293 (4 096 is
    the sort's tile) on prefixes of tests/ray_order_inputs.py's sets tiled to length, on 4 097 identical rays and on a set with no placed
    ray; the order between guard words, guard bytes behind ptmi_ray_order_bytes(n) bytes of workspace, none written.  The host twin is
    held to the written formula by tests/test_ray_order_layout.py
  2 on all five scene kinds, indexed trace (t, idx, hit record) and indexed occlusion (the t_max families of tests/t_max_families.py)
    equal the plain entries bit for bit (a NaN for a NaN) through the device order, its reverse and a seeded random permutation; outputs
    the binding allocates hold the miss record and 0 where no entry names a ray
  3 m = 0, 1, 63, 64, 65, 257 of n = 4 096 with duplicates, -1, n, INT32_MIN and INT32_MAX in the index; outputs prefilled with a sentinel
    between guards; rays, hit records and the index on both alignments: exactly the named positions hold the plain entries' words
  4 order, indexed trace and indexed occlusion back to back on torch's non-default stream behind a filler, read after that stream alone
    is synchronised
  5 every row of the header's refusal lists through the raw library handle, outputs and workspace untouched; PTMI_ESTATE for the indexed
    queries before a scene, PTMI_OK for the order
  6 a 64 x 48 render with order and indexed queries in between equals one without them on all seven planes (one BVH, one mesh scene)"""
import os
import subprocess
import sys
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ray_order_driver as driver  # noqa: E402

pytestmark = pytest.mark.gpu
LIMIT = 420                                  # seconds for the child: process start, torch, five scenes, the oracle's folds, six cases


@pytest.fixture(scope="module")
def outcome(pkg, ora, tmp_path_factory):
    """{case: None if it passed, else why not} from one run of the child"""
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, os.path.join(HERE, "ray_order_driver.py"), str(tmp_path_factory.mktemp("ray_order"))],
                         capture_output=True, text=True, timeout=LIMIT)
    print(res.stdout)
    print("ray_order_driver: %.1f s, exit %d" % (time.perf_counter() - t0, res.returncode))
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
def test_ray_order_and_indexed_queries_on_the_device(outcome, case):
    assert outcome[case] is None, outcome[case]
