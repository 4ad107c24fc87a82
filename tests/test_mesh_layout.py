"""ptmi_mesh_layout (host code, no device): the triangle hierarchy ptmi_set_scene_mesh builds -- every triangle of non-zero area in
exactly one leaf, boxes nested and padded as DESIGN.md 5.8 says, the depth within PTMI_BVH_MAX_DEPTH, the output a pure function of
the input, the refusals -- and world.load_obj."""
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
    inner, leaves, todo = [], [], [(0, 0)]
    while todo:
        k, level = todo.pop()
        inner.append((k, level))
        for c in range(2):
            ref = int(nodes[k]["ref"][c])
            lo = nodes[k]["center"][c].astype(np.float64) - nodes[k]["half"][c].astype(np.float64)
            hi = nodes[k]["center"][c].astype(np.float64) + nodes[k]["half"][c].astype(np.float64)
            if ref >= 0:
                todo.append((ref, level + 1))
                for cc in range(2):
                    if int(nodes[ref]["ref"][cc]) != -1:
                        clo = nodes[ref]["center"][cc].astype(np.float64) - nodes[ref]["half"][cc].astype(np.float64)
                        chi = nodes[ref]["center"][cc].astype(np.float64) + nodes[ref]["half"][cc].astype(np.float64)
                        assert np.all(lo <= clo) and np.all(chi <= hi)
            elif ref != -1:
                v = -1 - ref
                leaves.append((v >> 8, v & 255, lo, hi, level))
    return inner, leaves


@pytest.mark.parametrize("subdivisions", [0, 2, 5])
def test_every_triangle_sits_in_exactly_one_leaf_and_the_boxes_nest(subdivisions):
    _, t, _ = world.mesh_room(subdivisions)
    flat = t[[20, 21]].copy()
    flat["v2"] = flat["v0"]                                    # zero area: in no leaf
    t = np.concatenate([t, flat])
    nodes, order = binding.mesh_layout(t)
    assert sorted(order.tolist()) == list(range(len(t) - 2))
    inner, leaves = walk(nodes)
    assert sorted(k for k, _ in inner) == list(range(len(nodes)))
    covered = np.zeros(len(t), np.int32)
    for first, count, lo, hi, level in leaves:
        assert 1 <= count <= binding.BVH_LEAF_MAX
        for i in order[first:first + count]:
            covered[i] += 1
            v = np.stack([t["v0"][i], t["v1"][i], t["v2"][i]]).astype(np.float64)
            pad = 2.0 ** -16 * (np.abs(v).max() + (v.max(0) - v.min(0)).max())
            assert np.all(lo <= v.min(0) - pad) and np.all(v.max(0) + pad <= hi), (i, lo, hi)
    assert np.all(covered[:-2] == 1) and np.all(covered[-2:] == 0)
    assert np.all(nodes["inv_2r"] == 0)


def test_depth_stays_within_the_header_bound():
    for sub in (3, 7):
        _, t, _ = world.mesh_room(sub)
        nodes, _ = binding.mesh_layout(t)
        deepest = max(level for _, level in walk(nodes)[0])
        assert deepest < binding.BVH_MAX_DEPTH
        assert deepest <= int(np.ceil(np.log2(len(t) / 4.0)))          # median splits: balanced
    # at 2^22 triangles a balanced tree has ceil(log2(2^22 / 4)) = 20 levels of inner nodes, within PTMI_BVH_MAX_DEPTH
    assert int(np.ceil(np.log2(binding.MAX_MESH_TRIANGLES / binding.BVH_LEAF_MAX))) < binding.BVH_MAX_DEPTH
    same = np.repeat(world.mesh_room(0)[1][13:14], 5000)             # one triangle 5000 times: the splits still halve (ties by index)
    nodes, order = binding.mesh_layout(same)
    assert max(level for _, level in walk(nodes)[0]) < binding.BVH_MAX_DEPTH and sorted(order.tolist()) == list(range(5000))


def test_the_layout_is_deterministic():
    _, t, _ = world.mesh_room(5, seed=4)
    a, b = binding.mesh_layout(t), binding.mesh_layout(t.copy())
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


def test_refusals():
    _, t, _ = world.mesh_room(1)
    for field, value in (("v0", np.nan), ("v1", np.inf), ("v2", -np.inf), ("color", np.nan), ("illuminance", np.inf),
                         ("brdf_param", np.nan), ("v1", 3e19)):
        bad = t.copy()
        if field in ("v0", "v1", "v2", "color"):
            bad[field][13, 1] = value
        else:
            bad[field][13] = value
        with pytest.raises(binding.PtmiError) as e:
            binding.mesh_layout(bad)
        assert e.value.code == binding.PTMI_EINVAL, (field, value)
    with pytest.raises(binding.PtmiError) as e:
        binding.mesh_layout(np.zeros(binding.MAX_MESH_TRIANGLES + 1, world.TRIANGLE_DTYPE))
    assert e.value.code == binding.PTMI_ELIMIT
    nodes, order = binding.mesh_layout(np.zeros(3, world.TRIANGLE_DTYPE))            # all of zero area: accepted, nothing in the tree
    assert len(order) == 0 and list(nodes[0]["ref"]) == [-1, -1]


def test_load_obj_reads_vertices_and_faces_only(tmp_path):
    text = "\n".join(["# a unit quad and a triangle", "o thing", "mtllib x.mtl", "v 0 0 0", "v 1 0 0", "v 1 1 0", "v 0 1 0",
                      "vn 0 0 1", "vt 0 0", "usemtl m", "s off", "f 1/1/1 2/1/1 3/1/1 4/1/1", "v 0 0 2", "f -5 -4 -1", "g group", "l 1 2"])
    path = tmp_path / "m.obj"
    path.write_text(text + "\n")
    mat = ((0.5, 0.6, 0.7), 2.0, world.GLOSSY, 0.8)
    for src in (str(path), text + "\n"):
        t = world.load_obj(src, mat)
        assert t.dtype == world.TRIANGLE_DTYPE and len(t) == 3
        assert t["v0"].tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, 0]]
        assert t["v1"].tolist() == [[1, 0, 0], [1, 1, 0], [1, 0, 0]]             # the quad fanned: (1 2 3), (1 3 4)
        assert t["v2"].tolist() == [[1, 1, 0], [0, 1, 0], [0, 0, 2]]             # -1: the last vertex read
        assert np.all(t["color"] == np.float32([0.5, 0.6, 0.7])) and np.all(t["brdf_tag"] == world.GLOSSY)
    with pytest.raises(ValueError):
        world.load_obj("v 0 0 0\nf 1 2 3\n", mat)
