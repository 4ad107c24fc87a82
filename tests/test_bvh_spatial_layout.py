"""ptmi_bvh_layout_spatial, the specification and host twin of ptmi_set_bvh_spheres' SPATIAL device build (PTMI_OPT_BVH_DEVICE_BUILD),
without a GPU: its references and leaf order equal a numpy restatement of the header's text (tests/bvh_spatial_scenes.py) at every count
and on every family -- all centres equal, flat in one and in two axes, duplicate keys, the chain on which the depth guard acts; the
order is a permutation, children come after their parent, levels are contiguous id ranges in ascending range start; ptmi_bvh_refit_layout
leaves the nodes byte-identical, and so does moving away and back; the CPU walk over it picks the linear fold's hit; its surface-area
cost is within 1.10 x of ptmi_bvh_layout's; refusals are ptmi_bvh_layout_morton's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bvh_rays  # noqa: E402
import bvh_spatial_scenes as spatial  # noqa: E402
import bvh_update_scenes as scenes  # noqa: E402
from test_bvh_refit_layout import check_invariants, extent, moved, walk_equals_fold  # noqa: E402

binding = scenes.binding
world = scenes.world
FAMILIES = spatial.families()
COUNTS = (1, 4, 5, 9, 64, 1020, 20000)


def spans_of(nodes, n):
    """[b, e) of every node, from the references alone (the leaves partition the leaf order in sequence)"""
    count = np.zeros(len(nodes), np.int64)
    ref = nodes["ref"]
    for i in range(len(nodes) - 1, -1, -1):
        count[i] = sum(int(count[r]) if r >= 0 else ((-1 - int(r)) & 255 if r != -1 else 0) for r in ref[i])
    begin = np.zeros(len(nodes), np.int64)
    for i in range(len(nodes)):
        at = int(begin[i])
        for r in ref[i]:
            if r >= 0:
                begin[r] = at
                at += int(count[r])
            elif r != -1:
                assert (-1 - int(r)) >> 8 == at, "a leaf out of sequence"
                at += (-1 - int(r)) & 255
    assert count[0] == n
    return begin, begin + count


def check_layout(s):
    nodes, order = binding.bvh_layout_spatial(s)
    again = binding.bvh_layout_spatial(s.copy())
    assert nodes.tobytes() == again[0].tobytes() and np.array_equal(order, again[1])
    n = len(s)
    ref, want_order, level_first, _ = spatial.restate(s)
    assert np.array_equal(order, want_order)
    assert np.array_equal(np.sort(order), np.arange(n))                       # a permutation: every sphere kept
    assert nodes["ref"].shape == ref.shape and np.array_equal(nodes["ref"], ref)
    # structure, from the nodes alone
    inner = nodes["ref"][nodes["ref"] >= 0]
    assert np.array_equal(np.sort(inner), np.arange(1, len(nodes)))           # every node but the root referred to once
    assert np.all((nodes["ref"] < 0) | (nodes["ref"] > np.arange(len(nodes))[:, None]))       # children have larger ids than their parent
    level = spatial.levels_of(nodes)
    assert np.all(np.diff(level) >= 0) and level.max() < binding.BVH_MAX_DEPTH     # levels are contiguous id ranges, none below level 23
    assert [int(np.searchsorted(level, lv)) for lv in range(int(level.max()) + 2)] == level_first
    begin, end = spans_of(nodes, n)
    for lv in range(int(level.max()) + 1):
        assert np.all(np.diff(begin[level == lv]) > 0)                        # ... in ascending range start
    leaves = nodes["ref"][(nodes["ref"] < -1)]
    assert not len(leaves) or ((-1 - leaves) & 255).max() <= binding.BVH_LEAF_MAX
    assert binding.bvh_refit_layout(s, nodes, order).tobytes() == nodes.tobytes()
    return nodes, order


@pytest.mark.parametrize("n", COUNTS)
def test_the_spatial_layout_is_the_restatement_at_every_count(n):
    s, _ = scenes.field(n, seed=24)
    nodes, order = check_layout(s)
    if n <= 1020:
        check_invariants(s, nodes, order)


def test_the_field_of_the_measurements_too():
    check_layout(world.sphere_field(1020, seed=24)[0])


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_the_spatial_layout_is_the_restatement_on_every_family(name):
    s, _ = FAMILIES[name]
    nodes, order = check_layout(s)
    check_invariants(s, nodes, order)


def test_an_empty_scene_gives_the_empty_root_and_a_null_scene_is_refused():
    nodes, order = binding.bvh_layout_spatial(np.zeros(0, binding.SPHERE_DTYPE))
    want = binding.bvh_layout_morton(np.zeros(0, binding.SPHERE_DTYPE))
    assert nodes.tobytes() == want[0].tobytes() and len(order) == 0
    lib = binding.load_library()
    assert lib.ptmi_bvh_layout_spatial(None, 0, None, 0, None) == lib.ptmi_bvh_layout_morton(None, 0, None, 0, None) == binding.PTMI_EINVAL


def test_small_scenes_are_todays_trees():
    for n in (1, 4):
        s, _ = scenes.field(n, seed=3)
        a, b = binding.bvh_layout_spatial(s), binding.bvh_layout_morton(s)
        assert np.array_equal(a[0]["ref"], b[0]["ref"]) and len(a[0]) == 1 and a[0]["ref"][0, 1] == -1


def test_the_chain_needs_the_guard_and_the_guard_holds():
    """every split of the chain peels a cell or a few off: without the guard the recursion passes level 24; with it no inner node lies
    below level 23 and no leaf holds more than 4, and some nodes did take the equal-count split"""
    s, _ = FAMILIES["chain"]
    _, _, unguarded, _ = spatial.restate(s, guard=False)
    assert len(unguarded) - 1 > binding.BVH_MAX_DEPTH, len(unguarded) - 1          # (levels of inner nodes)
    ref, _, guarded, fallbacks = spatial.restate(s)
    nodes, _ = binding.bvh_layout_spatial(s)
    level = spatial.levels_of(nodes)
    assert len(guarded) - 1 == level.max() + 1 <= binding.BVH_MAX_DEPTH
    assert level.max() == binding.BVH_MAX_DEPTH - 1                                # the guard acted at the limit, not before
    assert ((-1 - nodes["ref"][nodes["ref"] < -1]) & 255).max() <= binding.BVH_LEAF_MAX
    assert fallbacks > 0


def test_coincident_spheres_are_ordered_by_their_index():
    s, _ = FAMILIES["coincident"]
    _, order = binding.bvh_layout_spatial(s)
    key = spatial.spatial_keys(s)
    assert len(np.unique(key)) < len(s) // 2
    same = key[order][1:] == key[order][:-1]
    assert same.any() and np.all(order[1:][same] > order[:-1][same])


def test_a_short_axis_uses_the_low_part_of_its_bits():
    s = scenes.field(1020, seed=24)[0]
    s["position"][:, 1] *= np.float32(1.0 / 16.0)                               # a flat field: y is a tenth of the longest axis
    ext = np.ptp(s["position"], axis=0).astype(np.float64)
    assert ext[1] < ext.max() / 8
    y_bits = int(np.bitwise_or.reduce(spatial.spatial_keys(s)) & np.uint64(0x12492492492))      # bits 3 i + 1
    assert 0 < y_bits < 1 << (3 * 11 + 1)                                       # no y bit above i = 10: q_y <= 16384 / 8


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_moving_away_and_back_gives_the_same_bytes(name):
    s, _ = FAMILIES[name]
    nodes, order = binding.bvh_layout_spatial(s)
    s2 = moved(s, 0.25 * extent(s), "noise", 6)
    away = binding.bvh_refit_layout(s2, nodes, order)
    check_invariants(s2, away, order)
    assert binding.bvh_refit_layout(s, away, order).tobytes() == nodes.tobytes()


def test_refusals_are_the_morton_twins_and_write_nothing():
    s, _ = FAMILIES["adversarial"]
    lib = binding.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for what in ("position", "radius^2", "colour", "tag", "capacity", "too many"):
        bad, cap, n = s.copy(), len(s), len(s)
        if what == "position":
            bad["position"][5, 0] = np.inf
        elif what == "radius^2":
            bad["radius"][5] = -1e30
        elif what == "colour":
            bad["color"][5, 1] = np.nan
        elif what == "tag":
            bad["brdf_tag"][5] = -1
        elif what == "capacity":
            cap = 3
        else:
            n = binding.MAX_BVH_SPHERES + 1                                     # (refused before a sphere is read)
        got = []
        for fn in (lib.ptmi_bvh_layout_spatial, lib.ptmi_bvh_layout_morton):
            nodes = np.full(len(s), 7, np.uint8).repeat(64).view(binding.BVH_NODE_DTYPE)
            order = np.full(len(s), -7, np.int32)
            before = nodes.tobytes()
            got.append(fn(P(bad), n, P(nodes), cap, P(order)))
            assert nodes.tobytes() == before and np.all(order == -7), what
        assert got[0] == got[1] < 0, (what, got)
    one = np.zeros(1, binding.BVH_NODE_DTYPE)
    for args in ((None, 3, None, 0, None), (None, -1, P(one), 1, None), (P(s), len(s), P(one), -1, P(np.zeros(len(s), np.int32)))):
        assert lib.ptmi_bvh_layout_spatial(*args) == lib.ptmi_bvh_layout_morton(*args) < 0


@pytest.fixture(scope="module")
def trav(tmp_path_factory):
    return bvh_rays.traverse_lib(tmp_path_factory.mktemp("bvhspatial"))


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_the_cpu_walk_over_the_spatial_layout_is_the_linear_fold(trav, name):
    s, p = FAMILIES[name]
    nodes, order = binding.bvh_layout_spatial(s)
    rays = bvh_rays.adversarial_rays(s, 100_000, seed=9)
    hits = walk_equals_fold(trav, s, p, nodes, order, rays)
    assert hits > 10_000, hits


@pytest.mark.parametrize("n", [1020, 100_000])
def test_the_spatial_tree_costs_what_the_hosts_median_tree_costs(n):
    """The reason for the build.  cost = sum over non-empty child boxes of area x w (2 for an inner child, the sphere count for a leaf)
    over the area of the union of the root's two boxes; the spatial tree's is at most 1.10 x ptmi_bvh_layout's.
    Measured (padded boxes, as stored): n = 1 020: spatial 58.25 (x 0.993), median 58.68, equal-count 103.36 (x 1.762);
    n = 100 000: spatial 227.49 (x 0.987), median 230.49, equal-count 662.05 (x 2.872)."""
    s = world.sphere_field(n, seed=24)[0]
    ours = spatial.cost(binding.bvh_layout_spatial(s)[0])
    median = spatial.cost(binding.bvh_layout(s)[0])
    today = spatial.cost(binding.bvh_layout_morton(s)[0])
    print("n = %d: cost of the spatial tree %.2f, of ptmi_bvh_layout's %.2f (x %.3f), of the equal-count tree %.2f (x %.3f)"
          % (n, ours, median, ours / median, today, today / median))
    assert ours <= 1.10 * median, (ours, median)
