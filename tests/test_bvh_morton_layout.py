"""ptmi_bvh_layout_morton, the specification and host twin of ptmi_set_bvh_spheres' device build, without a GPU: deterministic; the leaf
order sorted by (Morton key of the centre within the f32 box of all centres, index) with the key recomputed here in numpy float64; every
sphere kept (radius 0 too); the topology that of the count, within PTMI_BVH_MAX_DEPTH; ptmi_bvh_refit_layout leaves it byte-identical;
refusals write nothing; the CPU walk (tests/cxx/bvh_traverse.c) over it picks the linear fold's hit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bvh_rays  # noqa: E402
import bvh_update_scenes as scenes  # noqa: E402
from test_bvh_refit_layout import check_invariants, walk_equals_fold  # noqa: E402

binding = scenes.binding
FAMILIES = scenes.families()


def morton_keys(s):
    """ptmi_mesh_morton.h's key of (c, c, c) in numpy float64, each operation rounded on its own"""
    c = s["position"].astype(np.float32)
    if not len(c):
        return np.zeros(0, np.uint64)
    lo, hi = c.min(0).astype(np.float64), c.max(0).astype(np.float64)
    c = c.astype(np.float64)
    key = np.zeros(len(s), np.uint64)
    for a in range(3):
        if hi[a] == lo[a]:
            q = np.zeros(len(s), np.int64)
        else:
            num = (((c[:, a] + c[:, a]) + c[:, a]) - 3.0 * lo[a]) * 16384.0
            den = 3.0 * (hi[a] - lo[a])
            q = np.minimum(16383, np.floor(num / den).astype(np.int64))
        for i in range(14):
            key |= ((q >> i) & 1).astype(np.uint64) << np.uint64(3 * i + (2 - a))
    return key


def depth(nodes):
    level = np.zeros(len(nodes), np.int64)
    for i, nd in enumerate(nodes):
        for ref in nd["ref"]:
            if ref >= 0:
                level[ref] = level[i] + 1
    return int(level.max()) if len(nodes) else 0


def check_layout(s):
    nodes, order = binding.bvh_layout_morton(s)
    again = binding.bvh_layout_morton(s.copy())
    assert nodes.tobytes() == again[0].tobytes() and np.array_equal(order, again[1])
    n = len(s)
    assert np.array_equal(np.sort(order), np.arange(n))                       # every sphere kept
    key = morton_keys(s)
    assert np.array_equal(order, np.lexsort((np.arange(n), key)).astype(np.int32))
    assert depth(nodes) < binding.BVH_MAX_DEPTH
    # the topology: leaves partition the leaf order in sequence, splits at b + n / 2, children after their parent
    def spans(node_id, b, e):
        m = e - b
        mid = b + m // 2 if m > binding.BVH_LEAF_MAX else e
        for ref, (cb, ce) in zip(nodes[node_id]["ref"], ((b, mid), (mid, e))):
            if ce - cb > binding.BVH_LEAF_MAX:
                assert ref > node_id
                spans(int(ref), cb, ce)
            else:
                assert ref == (-1 if ce == cb else -1 - ((cb << 8) | (ce - cb)))
    spans(0, 0, n)
    assert binding.bvh_refit_layout(s, nodes, order).tobytes() == nodes.tobytes()
    return nodes, order


@pytest.mark.parametrize("n", scenes.COUNTS)
def test_the_morton_layout_at_every_count(n):
    s, _ = scenes.field(n, seed=n + 1)
    nodes, order = check_layout(s)
    if n <= 4097:
        check_invariants(s, nodes, order)


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_the_morton_layout_of_every_family(name):
    s, _ = FAMILIES[name]
    nodes, order = check_layout(s)
    check_invariants(s, nodes, order)


def test_coincident_spheres_are_ordered_by_their_index():
    s, _ = scenes.coincident(1000, 4)
    _, order = binding.bvh_layout_morton(s)
    key = morton_keys(s)
    assert len(np.unique(key)) < len(s) // 2
    same = key[order][1:] == key[order][:-1]
    assert same.any() and np.all(order[1:][same] > order[:-1][same])


def test_refusals_write_nothing():
    s, _ = FAMILIES["adversarial"]
    lib = binding.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for what, code in (("position", binding.PTMI_EINVAL), ("radius^2", binding.PTMI_EINVAL), ("colour", binding.PTMI_EINVAL), ("tag", binding.PTMI_EINVAL),
                       ("capacity", binding.PTMI_ELIMIT)):
        bad = s.copy()
        cap = len(s)
        if what == "position":
            bad["position"][5, 0] = np.inf
        elif what == "radius^2":
            bad["radius"][5] = -1e30
        elif what == "colour":
            bad["color"][5, 1] = np.nan
        elif what == "tag":
            bad["brdf_tag"][5] = -1
        else:
            cap = 3
        nodes = np.full(len(s), 7, np.uint8).repeat(64).view(binding.BVH_NODE_DTYPE)
        order = np.full(len(s), -7, np.int32)
        before = nodes.tobytes()
        assert lib.ptmi_bvh_layout_morton(P(bad), len(bad), P(nodes), cap, P(order)) == code, what
        assert nodes.tobytes() == before and np.all(order == -7), what
    assert lib.ptmi_bvh_layout_morton(None, 3, None, 0, None) == binding.PTMI_EINVAL
    assert lib.ptmi_bvh_layout_morton(None, -1, P(np.zeros(1, binding.BVH_NODE_DTYPE)), 1, None) == binding.PTMI_EINVAL


@pytest.fixture(scope="module")
def trav(tmp_path_factory):
    return bvh_rays.traverse_lib(tmp_path_factory.mktemp("bvhmorton"))


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_the_cpu_walk_over_the_morton_layout_is_the_linear_fold(trav, name):
    s, p = FAMILIES[name]
    nodes, order = binding.bvh_layout_morton(s)
    rays = bvh_rays.adversarial_rays(s, 100_000, seed=9)
    hits = walk_equals_fold(trav, s, p, nodes, order, rays)
    assert hits > 10_000, hits
