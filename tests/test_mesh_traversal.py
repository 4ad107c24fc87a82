"""The triangle hierarchy's padding and pruning are conservative, shown on the CPU: tests/cxx/mesh_traverse.c walks the layout
ptmi_mesh_layout exports as the device's check_hit_mesh does (same admission, margin, slab test, pruning, tie rule) and must pick the
hit the literal fold over spheres ++ planes ++ triangles picks (t bit for bit, the primitive, Just / Nothing) on seeded adversarial rays
(tests/mesh_rays.py): 10^6 rays on about 1.3k and on about 83k triangles.  The count of rays that hit a triangle is checked too, so that the
comparison cannot pass vacuously."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_rays  # noqa: E402


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return mesh_rays.traverse_lib(tmp_path_factory.mktemp("mesh"))


def assert_same(got, want, what):
    (t0, i0, j0), (t1, i1, j1) = got, want
    assert not np.any(j0 == -2), "the traversal stack would overflow"
    bad = np.flatnonzero((t0.view(np.uint32) != t1.view(np.uint32)) | (i0 != i1) | (j0 != j1))
    assert bad.size == 0, "%s: %d of %d rays differ, e.g. ray %d: walk (%r, %d, %d) fold (%r, %d, %d)" % (
        what, bad.size, len(t0), bad[0], t0[bad[0]], i0[bad[0]], j0[bad[0]], t1[bad[0]], i1[bad[0]], j1[bad[0]])


@pytest.mark.parametrize("subdivisions, n_rays", [(3, 1_000_000), (6, 1_000_000)])
def test_the_walk_picks_the_linear_folds_hit(lib, subdivisions, n_rays):
    s, t, p = mesh_rays.adversarial_scene(subdivisions, seed=subdivisions)
    rays = mesh_rays.adversarial_rays(t, n_rays, seed=subdivisions)
    want = mesh_rays.linear_fold(lib, s, t, p, rays)
    got, tests = mesh_rays.walk(lib, s, t, p, rays)
    assert_same(got, want, "%d triangles" % len(t))
    first = len(s) + len(p)
    on_triangles = int(np.sum(want[2].astype(bool) & (want[1] >= first + 13)))          # the icosphere and its duplicates
    assert on_triangles > n_rays // 10, on_triangles
    assert int(np.sum(want[2].astype(bool) & (want[1] >= first))) > n_rays // 5
    if subdivisions == 6:
        assert len(t) >= 50_000
        assert tests < n_rays * len(t) // 100                        # the hierarchy prunes


def test_ties_between_a_triangle_and_a_plane_keep_the_plane(lib):
    s, t, p = mesh_rays.adversarial_scene(2, seed=3)
    k = 13
    cen = ((t["v0"][k] + t["v1"][k] + t["v2"][k]) / np.float32(3.0)).astype(np.float32)
    n = np.float32(p["direction"][0])
    rays = np.zeros((1000, 6), np.float32)
    rng = np.random.default_rng(1)
    rays[:, :3] = cen + (3.0 + rng.random((1000, 1))) * n + 0.05 * rng.normal(size=(1000, 3))
    rays[:, 3:] = mesh_rays._unit(cen - rays[:, :3])
    want = mesh_rays.linear_fold(lib, s, t, p, rays)
    got, _ = mesh_rays.walk(lib, s, t, p, rays)
    assert_same(got, want, "plane / triangle ties")
    assert np.sum(want[1] == len(s)) > 500                   # the plane (index ns) wins the ties with its own triangle
