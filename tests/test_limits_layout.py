"""The host builders at their limits (no device): ptmi_bvh_layout, ptmi_bvh_layout_morton and ptmi_bvh_layout_spatial over
PTMI_MAX_BVH_SPHERES spheres, ptmi_mesh_layout and ptmi_mesh_layout_morton over PTMI_MAX_MESH_TRIANGLES triangles, on the scenes of
tests/limit_scenes.py.  The structure of every tree -- node count, leaf references (whose first position, shifted by 8, comes up to 2^30 only
here), the leaves a partition of the order, the order a permutation, the depth, every box around its primitives -- checked vectorised in
float64; then the CPU traversals (tests/cxx/bvh_traverse.c, tests/cxx/mesh_traverse.c) over those trees on 20 000 rays from inside the
room, which must pick what the core scene's literal fold picks, the index mapped.  Also the sphere count at which the spatial tree has a
level of more than 65 792 nodes (tests/test_gpu_limits.py builds it on the device);
run with -s, the tests print the time every host twin takes."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bvh_rays  # noqa: E402
import limit_scenes as limits  # noqa: E402
import mesh_rays  # noqa: E402
import oracle as ora  # noqa: E402

binding, world = limits.binding, limits.world
N_SPHERES, N_TRIANGLES = binding.MAX_BVH_SPHERES, binding.MAX_MESH_TRIANGLES
N_RAYS = 20_000
WIDE_LEVEL, SPATIAL_WIDE_COUNT = limits.WIDE_LEVEL, limits.SPATIAL_WIDE_COUNT


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


level_counts = limits.level_counts


def check_tree(nodes, order, n, lo, hi, node_bound, what):
    """lo, hi: the box of every primitive by original index (float64).  -> the level counts"""
    assert 1 <= len(nodes) <= node_bound, "%s: %d nodes, the bound is %d" % (what, len(nodes), node_bound)
    assert len(order) == n and np.array_equal(np.bincount(order, minlength=n), np.ones(n, np.int64)), "%s: the order is no permutation" % what
    counts = level_counts(nodes)
    assert len(counts) <= binding.BVH_MAX_DEPTH, "%s: inner nodes on %d levels" % (what, len(counts))
    ref = nodes["ref"].astype(np.int64)
    assert np.all(ref < len(nodes))
    node, child = np.nonzero(ref < -1)
    v = -1 - ref[node, child]
    first, count = v >> 8, v & 255
    assert np.all((count >= 1) & (count <= binding.BVH_LEAF_MAX)), "%s: a leaf of %d" % (what, count.max())
    assert np.all((first >= 0) & (first + count <= n))
    by = np.argsort(first, kind="stable")
    node, child, first, count = node[by], child[by], first[by], count[by]
    assert first[0] == 0 and np.array_equal(first[1:], (first + count)[:-1]) and first[-1] + count[-1] == n, "%s: the leaves do not partition the order" % what
    # every leaf box holds its primitives, every inner child's box the boxes of that node's children
    blo = nodes["center"].astype(np.float64) - nodes["half"].astype(np.float64)
    bhi = nodes["center"].astype(np.float64) + nodes["half"].astype(np.float64)
    leaf_of = np.repeat(np.arange(len(first)), count)                       # (position of the order -> its leaf: they are contiguous)
    prim = order[np.arange(n)]
    bad = np.flatnonzero(np.any(blo[node, child][leaf_of] > lo[prim], 1) | np.any(bhi[node, child][leaf_of] < hi[prim], 1))
    assert bad.size == 0, "%s: %d primitives reach out of their leaf's box, first at position %d" % (what, bad.size, bad[0])
    k, c = np.nonzero(ref >= 0)
    kid = ref[k, c]
    for cc in range(2):
        full = ref[kid, cc] != -1
        bad = np.flatnonzero(full & (np.any(blo[k, c] > blo[kid, cc], 1) | np.any(bhi[k, c] < bhi[kid, cc], 1)))
        assert bad.size == 0, "%s: %d child boxes reach out of their parent's" % (what, bad.size)
    return counts


def sphere_boxes(s):
    c, r = s["position"].astype(np.float64), np.abs(s["radius"].astype(np.float64))[:, None]
    return c - r, c + r


def triangle_boxes(t):
    v = np.stack([t[k].astype(np.float64) for k in ("v0", "v1", "v2")], 1)
    return v.min(1), v.max(1)


def same_hits(got, want, what):
    for a, b, name in zip(got, want, ("t", "idx", "just")):
        bad = np.flatnonzero(np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32))
        assert bad.size == 0, "%s: %s differs for %d of %d rays, first %d: %r against %r" % (what, name, bad.size, len(a), bad[0], a[bad[0]], b[bad[0]])


@pytest.fixture(scope="module")
def trav(tmp_path_factory):
    return bvh_rays.traverse_lib(tmp_path_factory.mktemp("limitbvh"))


@pytest.fixture(scope="module")
def mtrav(tmp_path_factory):
    return mesh_rays.traverse_lib(tmp_path_factory.mktemp("limitmesh"))


@pytest.fixture(scope="module")
def sphere_scene():
    full, core, index = limits.spheres(N_SPHERES, "last")
    limits.premise_holds(full, index)
    return full, core, index, limits.planes()


@pytest.fixture(scope="module")
def triangle_scene():
    full, core, index = limits.triangles(N_TRIANGLES, "last")
    return full, core, index


@pytest.fixture(scope="module")
def sphere_want(trav, sphere_scene):
    """the core scene's fold on the rays, the index mapped to the full scene"""
    full, core, index, p = sphere_scene
    rays = limits.sphere_rays(core, N_RAYS, seed=41)
    t, idx, just = bvh_rays.linear_fold(trav, core, p, rays)
    return rays, (t, limits.map_index(idx, (len(core), len(p)), (len(full), len(p)), index), just)


@pytest.mark.parametrize("builder", ["bvh_layout", "bvh_layout_morton", "bvh_layout_spatial"])
def test_a_sphere_tree_at_the_limit_is_sound_and_its_walk_picks_the_core_folds_hit(trav, sphere_scene, sphere_want, builder):
    full, core, index, p = sphere_scene
    n = len(full)
    assert n == binding.MAX_BVH_SPHERES
    start = time.time()
    nodes, order = getattr(binding, builder)(full)
    print("%s at %d spheres: %.2f s" % (builder, n, time.time() - start))
    # equal counts halve down to 4 or fewer: a leaf holds at least 2 of more than 4 spheres; a spatial split may peel off 1
    bound = n // 2 if builder != "bvh_layout_spatial" else n - 1
    counts = check_tree(nodes, order, n, *sphere_boxes(full), bound, builder)
    print("%s: %d nodes on %d levels, the widest %d" % (builder, len(nodes), len(counts), max(counts)))
    ref = nodes["ref"].astype(np.int64)
    assert ((-1 - ref[ref < -1]) >> 8).max() >= n - binding.BVH_LEAF_MAX     # the last leaf's first position: all 22 bits, shifted by 8
    pos = full["position"].astype(np.float32)
    lo, hi = np.ascontiguousarray(pos.min(0)), np.ascontiguousarray(pos.max(0))
    rays, want = sphere_want
    pick = limits.walked_rays(rays, lo, hi)                                 # (the unserved rays are folded literally over 2^22 spheres: 64 of them)
    assert len(pick) > len(rays) * 3 // 4
    rays, want = np.ascontiguousarray(rays[pick]), tuple(a[pick] for a in want)
    s, pl = np.ascontiguousarray(full, ora.SPHERE_DTYPE), np.ascontiguousarray(p, ora.PLANE_DTYPE)
    t, idx, just = np.zeros(len(rays), np.float32), np.zeros(len(rays), np.int32), np.zeros(len(rays), np.int32)
    start = time.time()
    trav.bvh_check_hit(_p(nodes), _p(order), _p(lo), _p(hi), _p(s), n, _p(pl), len(pl), _p(rays), len(rays), _p(t), _p(idx), _p(just))
    print("the walk of %d rays: %.2f s" % (len(rays), time.time() - start))
    assert not np.any(just == -2), "the traversal stack would overflow"
    same_hits((t, idx, just), want, builder)
    top = int(np.sum((just == 1) & (idx >= n - len(core)) & (idx < n)))
    on_planes = int(np.sum((just == 1) & (idx >= n)))
    print("%d rays hit the top-index spheres, %d a plane" % (top, on_planes))
    assert top > 1000 and on_planes > 1000


@pytest.mark.parametrize("builder", ["mesh_layout", "mesh_layout_morton"])
def test_a_triangle_tree_at_the_limit_is_sound_and_its_walk_picks_the_core_folds_hit(mtrav, sphere_scene, triangle_scene, builder):
    """The CPU walk takes spheres and planes by the literal fold, so it is given the core spheres; the triangle hierarchy is the full
    one.  Indices are counted as the full scene of 2^22 spheres counts them (limit_scenes.map_index)."""
    s_full, s_core, s_index, p = sphere_scene
    full, core, index = triangle_scene
    n = len(full)
    assert n == binding.MAX_MESH_TRIANGLES
    limits.premise_holds(s_full, s_index, full, index)
    start = time.time()
    nodes, order = getattr(binding, builder)(full)
    print("%s at %d triangles: %.2f s" % (builder, n, time.time() - start))
    counts = check_tree(nodes, order, n, *triangle_boxes(full), n // 2, builder)
    print("%s: %d nodes on %d levels, the widest %d" % (builder, len(nodes), len(counts), max(counts)))
    ref = nodes["ref"].astype(np.int64)
    assert ((-1 - ref[ref < -1]) >> 8).max() >= n - binding.BVH_LEAF_MAX
    rays = limits.mesh_rays_for(s_core, core, N_RAYS, seed=43)
    sizes = ((len(s_core), len(p)), (len(s_full), len(p)))
    t, idx, just = mesh_rays.linear_fold(mtrav, s_core, core, p, rays)
    want = (t, limits.map_index(idx, *sizes, s_index, index), just)
    # the walk over the full tree: the core spheres, the planes, every triangle; its triangle k is the full scene's triangle k
    rec = mesh_rays.records(mtrav, full)
    allv = np.concatenate([full["v0"], full["v1"], full["v2"]]).astype(np.float32)
    lo, hi = np.ascontiguousarray(allv.min(0)), np.ascontiguousarray(allv.max(0))
    sc, pl = np.ascontiguousarray(s_core, ora.SPHERE_DTYPE), np.ascontiguousarray(p, ora.PLANE_DTYPE)
    pick = limits.walked_rays(rays, lo, hi)                                 # (the unserved rays are folded literally over 2^22 triangles: 64 of them)
    assert len(pick) > len(rays) * 3 // 4
    rays, want = np.ascontiguousarray(rays[pick]), tuple(a[pick] for a in want)
    m = len(rays)
    t, idx, just = np.zeros(m, np.float32), np.zeros(m, np.int32), np.zeros(m, np.int32)
    start = time.time()
    mtrav.mesh_walk_check_hit(_p(nodes), _p(order), len(order), _p(lo), _p(hi), _p(sc), len(sc), _p(pl), len(pl), _p(rec), len(rec),
                              _p(rays), m, _p(t), _p(idx), _p(just))
    print("the walk of %d rays: %.2f s" % (m, time.time() - start))
    assert not np.any(just == -2), "the traversal stack would overflow"
    walked = idx.astype(np.int64)
    tri = walked >= len(sc) + len(pl)
    walked[tri] += len(s_full) - len(sc)                                     # a triangle's index behind 2^22 spheres
    sph = (walked >= 0) & (walked < len(sc))
    walked[sph] = s_index[walked[sph]]
    pln = ~tri & ~sph & (walked >= 0)
    walked[pln] += len(s_full) - len(sc)
    same_hits((t, walked.astype(np.int32), just), want, builder)
    high = int(np.sum((just == 1) & (walked >= 1 << 23)))
    print("%d rays hit triangles whose fold index is 2^23 or more" % high)
    assert high > 500


def test_the_premise_on_the_data_itself_the_full_literal_fold_on_256_rays(mtrav, sphere_scene, triangle_scene):
    """2^22 spheres ++ 64 planes ++ 2^22 triangles folded literally: what the core scene's fold picks, the index mapped"""
    s_full, s_core, s_index, p = sphere_scene
    full, core, index = triangle_scene
    rays = limits.mesh_rays_for(s_core, core, 256, seed=44)
    t, idx, just = mesh_rays.linear_fold(mtrav, s_core, core, p, rays)
    want = (t, limits.map_index(idx, (len(s_core), len(p)), (len(s_full), len(p)), s_index, index), just)
    same_hits(limits.mesh_fold_in_slices(mtrav, s_full, full, p, rays), want, "the full fold")
    assert int(np.sum(want[1] >= len(s_full) + len(p))) > 5 and int(np.sum((want[1] >= 0) & (want[1] < len(s_full)))) > 20


def test_a_spatial_tree_has_a_level_the_numbering_kernel_walks_twice():
    full, _, _ = limits.spheres(SPATIAL_WIDE_COUNT, "last")
    nodes, _ = binding.bvh_layout_spatial(full)
    assert max(level_counts(nodes)) >= WIDE_LEVEL
