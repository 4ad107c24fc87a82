"""The hierarchy's padding and pruning are conservative, shown on the CPU: tests/cxx/bvh_traverse.c walks the layout ptmi_bvh_layout
exports exactly as the device's check_hit_bvh does (same admission, margins, slab test, pruning), testing spheres with the oracle's
ora_distance_to_sphere -- whose arithmetic the device's sphere test matches -- and must pick the hit the linear fold of ora_check_hit
picks (t bit for bit, the primitive, Just / Nothing) on a million seeded rays, adversarial ones included (tests/bvh_rays.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import bvh_rays  # noqa: E402
import oracle as ora  # noqa: E402

binding = graft.load_package().binding


@pytest.fixture(scope="module")
def trav(tmp_path_factory):
    return bvh_rays.traverse_lib(tmp_path_factory.mktemp("bvh"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run_both(lib, spheres, planes, rays):
    s = np.ascontiguousarray(spheres, ora.SPHERE_DTYPE)
    p = np.ascontiguousarray(planes, ora.PLANE_DTYPE)
    nodes, order = binding.bvh_layout(s)
    field = s["position"].astype(np.float32)
    lo, hi = np.ascontiguousarray(field.min(0)), np.ascontiguousarray(field.max(0))
    n = len(rays)
    res = []
    for fn in ("lin", "bvh"):
        t, idx, just = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        if fn == "lin":
            lib.lin_check_hit(_p(s), len(s), _p(p), len(p), _p(rays), n, _p(t), _p(idx), _p(just))
            tests = None
        else:
            tests = lib.bvh_check_hit(_p(nodes), _p(order), _p(lo), _p(hi), _p(s), len(s), _p(p), len(p), _p(rays), n, _p(t), _p(idx), _p(just))
        res.append((t, idx, just, tests))
    return res


def assert_same(lin, bvh):
    (t0, i0, j0, _), (t1, i1, j1, _) = lin, bvh
    assert not np.any(j1 == -2), "the traversal stack would overflow"
    bad = np.flatnonzero((t0.view(np.uint32) != t1.view(np.uint32)) | (i0 != i1) | (j0 != j1))
    assert bad.size == 0, "%d of %d rays differ, e.g. ray %d: linear (%r, %d, %d) bvh (%r, %d, %d)" % (
        bad.size, len(t0), bad[0], t0[bad[0]], i0[bad[0]], j0[bad[0]], t1[bad[0]], i1[bad[0]], j1[bad[0]])


def test_the_fold_with_its_index_is_ora_check_hit(trav):
    spheres, planes = bvh_rays.adversarial_scene(300, seed=3)
    rays = bvh_rays.adversarial_rays(spheres, 1600, seed=3)
    (t, idx, just, _), _ = run_both(trav, spheres, planes, rays)
    for k in range(len(rays)):
        h = ora.check_hit(spheres, planes, rays[k, :3], rays[k, 3:])
        assert (h is not None) == bool(just[k]), k
        if just[k]:
            i = int(idx[k])
            want = ora.hit_sphere(rays[k, :3], rays[k, 3:], t[k], spheres[i]) if i < len(spheres) else \
                ora.hit_plane(rays[k, :3], rays[k, 3:], t[k], planes[i - len(spheres)])
            assert h[0].tobytes() == want[0].tobytes() and h[1].tobytes() == want[1].tobytes(), k


def test_bvh_picks_the_linear_folds_hit_on_a_million_adversarial_rays(trav):
    spheres, planes = bvh_rays.adversarial_scene(1500, seed=1)
    rays = bvh_rays.adversarial_rays(spheres, 1_000_000, seed=1)
    lin, bvh = run_both(trav, spheres, planes, rays)
    assert_same(lin, bvh)
    hits = int(lin[2].sum())
    assert hits > 200_000, hits                                   # the rays do meet the scene


def test_the_hierarchy_prunes_on_a_sphere_field(trav):
    spheres, planes = bvh_rays.world.sphere_field(20000, seed=2)
    rng = np.random.default_rng(2)
    c = spheres["position"]
    o = c.min(0) + (c.max(0) - c.min(0)) * rng.random((50_000, 3))
    d = rng.normal(size=(50_000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays = np.ascontiguousarray(np.hstack([o, d]).astype(np.float32))
    lin, bvh = run_both(trav, spheres, planes, rays)
    assert_same(lin, bvh)
    assert bvh[3] < 0.01 * len(rays) * len(spheres), bvh[3] / len(rays)     # under 1 % of the linear fold's sphere tests


@pytest.mark.parametrize("n, seed", [(1, 5), (4, 6), (5, 7), (40, 8), (20000, 9)])
def test_bvh_picks_the_linear_folds_hit_at_other_sizes(trav, n, seed):
    spheres, planes = bvh_rays.adversarial_scene(n, seed=seed)
    rays = bvh_rays.adversarial_rays(spheres, 40_000 if n < 10000 else 200_000, seed=seed)
    assert_same(*run_both(trav, spheres, planes, rays))
