"""ptmi_bvh_layout (host code, no device): the hierarchy ptmi_set_scene_bvh builds.  Every sphere in exactly one leaf, boxes nested
and padded as include/ptmi.h says, the depth within PTMI_BVH_MAX_DEPTH, the output a pure function of the input, and the documented
refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
binding, world = pkg.binding, pkg.world


def walk(nodes):
    """-> [(node, level)], [(first, count, box lo, box hi, level)] of the leaves"""
    inner, leaves, todo = [], [], [(0, 0)]
    while todo:
        k, level = todo.pop()
        inner.append((k, level))
        nd = nodes[k]
        for c in range(2):
            ref = int(nd["ref"][c])
            lo = nd["center"][c].astype(np.float64) - nd["half"][c].astype(np.float64)
            hi = nd["center"][c].astype(np.float64) + nd["half"][c].astype(np.float64)
            if ref >= 0:
                todo.append((ref, level + 1))
            elif ref != -1:
                v = -1 - ref
                leaves.append((v >> 8, v & 255, lo, hi, level))
    return inner, leaves


def child_box(nd, c):
    return nd["center"][c].astype(np.float64) - nd["half"][c].astype(np.float64), nd["center"][c].astype(np.float64) + nd["half"][c].astype(np.float64)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 17, 1000, 50000])
def test_every_sphere_sits_in_exactly_one_leaf_and_the_boxes_nest(n):
    spheres, _ = world.sphere_field(n, seed=n)
    nodes, order = binding.bvh_layout(spheres)
    assert len(nodes) <= max(1, n)
    assert sorted(order.tolist()) == list(range(n))
    inner, leaves = walk(nodes)
    assert sorted(k for k, _ in inner) == list(range(len(nodes)))            # every node reached once
    covered = np.zeros(n, np.int32)
    for first, count, lo, hi, level in leaves:
        assert 1 <= count <= pkg.binding.BVH_LEAF_MAX
        for i in order[first:first + count]:
            covered[i] += 1
            s = spheres[i]
            r = abs(float(s["radius"]))
            pad = r * (1 + 2.0 ** -8) + 2.0 ** -20 * max(np.abs(s["position"].astype(np.float64)).max(), r)
            assert np.all(lo <= s["position"] - pad) and np.all(s["position"] + pad <= hi), (i, lo, hi)
    assert np.all(covered == 1)
    for k, _ in inner:                                                   # a child's box holds its children's boxes
        for c in range(2):
            ref = int(nodes[k]["ref"][c])
            if ref >= 0:
                lo, hi = child_box(nodes[k], c)
                for cc in range(2):
                    if int(nodes[ref]["ref"][cc]) != -1:
                        clo, chi = child_box(nodes[ref], cc)
                        assert np.all(lo <= clo) and np.all(chi <= hi)
    for k, _ in inner:                                                   # inv_2r: 1 / (2 smallest radius) under the child, never below it
        for c in range(2):
            ref = int(nodes[k]["ref"][c])
            if ref == -1:
                continue
            idx = [int(order[f + j]) for f, cnt, *_ in collect(nodes, k, c) for j in range(cnt)]
            r_min = min(abs(float(spheres[i]["radius"])) for i in idx)
            assert nodes[k]["inv_2r"][c] >= 1.0 / (2.0 * r_min) if r_min > 0 else np.isinf(nodes[k]["inv_2r"][c])
        if n > 1000:
            break


def collect(nodes, k, c):
    ref = int(nodes[k]["ref"][c])
    if ref < 0:
        v = -1 - ref
        return [(v >> 8, v & 255)]
    return collect(nodes, ref, 0) + collect(nodes, ref, 1)


def test_depth_stays_within_the_header_bound():
    for n in (5, 1000, 1 << 18):
        spheres, _ = world.sphere_field(n, seed=1)
        nodes, _ = binding.bvh_layout(spheres)
        inner, leaves = walk(nodes)
        deepest = max(level for _, level in inner)
        assert deepest < binding.BVH_MAX_DEPTH
        assert deepest <= int(np.ceil(np.log2(max(1.0, n / 4.0))))          # median splits: a balanced tree
    # all spheres at one point: the splits still halve (ties by index)
    same = np.repeat(world.sphere_field(1, seed=2)[0], 5000)
    nodes, order = binding.bvh_layout(same)
    assert max(level for _, level in walk(nodes)[0]) < binding.BVH_MAX_DEPTH
    assert sorted(order.tolist()) == list(range(5000))


def test_the_layout_is_deterministic():
    spheres, _ = world.sphere_field(30000, seed=4)
    a = binding.bvh_layout(spheres)
    b = binding.bvh_layout(spheres.copy())
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


def test_empty_and_tiny_layouts():
    nodes, order = binding.bvh_layout(np.zeros(0, world.SPHERE_DTYPE))
    assert len(nodes) == 1 and list(nodes[0]["ref"]) == [-1, -1] and order.size == 0
    nodes, order = binding.bvh_layout(world.sphere_field(3, seed=1)[0])
    assert len(nodes) == 1 and int(nodes[0]["ref"][1]) == -1 and -1 - int(nodes[0]["ref"][0]) == 3


def _raw(spheres, nodes_cap):
    lib = binding.load_library()
    s = np.ascontiguousarray(spheres, world.SPHERE_DTYPE)
    nodes = np.zeros(max(1, nodes_cap), binding.BVH_NODE_DTYPE)
    order = np.zeros(max(1, s.size), np.int32)
    return lib.ptmi_bvh_layout(s.ctypes.data_as(C.c_void_p) if s.size else None, s.size, nodes.ctypes.data_as(C.c_void_p), nodes_cap,
                               order.ctypes.data_as(C.c_void_p))


def test_refusals():
    spheres, _ = world.sphere_field(100, seed=1)
    assert _raw(spheres, 100) > 0
    assert _raw(spheres, 2) == binding.PTMI_ELIMIT                          # the nodes do not fit
    for field, value in (("position", np.nan), ("position", np.inf), ("radius", np.nan), ("radius", -np.inf), ("radius", 2e19)):
        bad = spheres.copy()
        if field == "position":
            bad["position"][17, 1] = value
        else:
            bad["radius"][17] = value                                        # (2e19: radius^2 overflows)
        assert _raw(bad, 100) == binding.PTMI_EINVAL, (field, value)
        with pytest.raises(binding.PtmiError) as e:
            binding.bvh_layout(bad)
        assert e.value.code == binding.PTMI_EINVAL
    lib = binding.load_library()
    assert lib.ptmi_bvh_layout(None, 5, None, 5, None) == binding.PTMI_EINVAL
    many = np.zeros(binding.MAX_BVH_SPHERES + 1, world.SPHERE_DTYPE)
    assert _raw(many, 8) == binding.PTMI_ELIMIT
