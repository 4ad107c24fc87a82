"""ptmi_mesh_layout_morton, the specification and host twin of the hierarchy ptmi_set_mesh_triangles builds on the device (no GPU
needed): for every family of triangles below its output is (i) accepted by ptmi_mesh_refit_layout and left byte-identical by it -- the
boxes are the refit's; (ii) a leaf order that is a permutation of exactly the triangles of non-zero area; (iii) ascending by (key,
index), the key recomputed here in numpy float64; (iv) as deep, and of as many nodes, as ptmi_mesh_layout's hierarchy; (v) walked on the
CPU (tests/cxx/mesh_traverse.c) to the literal fold's hit on tests/mesh_rays.py's rays; (vi) refused where ptmi_mesh_layout refuses, with
its codes; (vii) the same bytes twice."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_rays  # noqa: E402

pkg = mesh_rays.pkg
B, W = pkg.binding, pkg.world
N_RAYS = 20_000


def _flat(t, where):
    f = t[where].copy()
    f["v2"] = f["v1"]
    return f


def _first(k):
    s, t, p = mesh_rays.adversarial_scene(3, seed=1)
    return s, t[13:13 + k].copy(), p, t[13:13 + 300]


def _room():
    s, t, p = W.mesh_room(3)
    return s, t, p, t


def _coincident():
    s, t, p = mesh_rays.adversarial_scene(2, seed=2)
    t = np.repeat(t[20:21], 300)
    return s, t, p, t


def _only(scene):
    s, t, p = scene
    return s, t, p, t


def _zero_areas():
    s, t, p = W.mesh_room(2)
    t = np.concatenate([_flat(t, [3, 4]), t[:150], _flat(t, [40, 41, 42]), t[150:], _flat(t, [7])])
    return s, t, p, t


def _far_room():
    s, t, p = mesh_rays.transformed(W.mesh_room(3), 2.0 ** 12, mesh_rays.OFFSETS[2])
    return s, t, p, t


FAMILIES = dict([("k%d" % k, (lambda k=k: _first(k))) for k in (0, 1, 4, 5, 8, 9, 255, 256, 257)] +
                [("room", _room), ("coincident300", _coincident), ("planar_grid", lambda: _only(mesh_rays.planar_grid())),
                 ("coincident_grids", lambda: _only(mesh_rays.coincident_grids())), ("zero_areas", _zero_areas), ("far_room", _far_room)])


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return mesh_rays.traverse_lib(tmp_path_factory.mktemp("morton"))


def has_area(t):
    """nn > 0 by the library's f32 operations (ptmi_mesh_box.h: triangle_normal)"""
    v0, v1, v2 = (t[k].astype(np.float32) for k in ("v0", "v1", "v2"))
    e1, e2 = v1 - v0, v2 - v0
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    return ((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]) > 0


def morton_keys(t, kept):
    """The key of every kept triangle, in float64 as csrc/ptmi_mesh_morton.h states it -> uint64 per triangle (0 for the others)"""
    keys = np.zeros(len(t), np.uint64)
    if not len(kept):
        return keys
    v = np.stack([t[k][kept].astype(np.float32) for k in ("v0", "v1", "v2")], 1)             # [k, 3 vertices, 3 axes]
    lo, hi = v.min((0, 1)).astype(np.float64), v.max((0, 1)).astype(np.float64)
    vd = v.astype(np.float64)
    s = (vd[:, 0] + vd[:, 1]) + vd[:, 2]
    key = np.zeros(len(kept), np.uint64)
    for a in range(3):
        if hi[a] == lo[a]:
            continue
        q = np.minimum(16383, np.floor((s[:, a] - 3.0 * lo[a]) * 16384.0 / (3.0 * (hi[a] - lo[a]))).astype(np.int64)).astype(np.uint64)
        for i in range(14):
            key |= ((q >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i + 2 - a)
    keys[kept] = key
    return keys


def depth(nodes):
    level = np.zeros(len(nodes), np.int64)
    for i, nd in enumerate(nodes):                                                   # children have larger ids than their parent
        for r in nd["ref"]:
            if r >= 0:
                assert r > i
                level[r] = level[i] + 1
    return int(level.max())


def walk(lib, s, tri, p, rays, nodes, order):
    """mesh_rays.walk over a given hierarchy"""
    import oracle as ora
    s, p = np.ascontiguousarray(s, ora.SPHERE_DTYPE), np.ascontiguousarray(p, ora.PLANE_DTYPE)
    rec = mesh_rays.records(lib, tri)
    kept = tri[order]
    allv = np.concatenate([kept["v0"], kept["v1"], kept["v2"]]).astype(np.float32) if len(order) else np.zeros((1, 3), np.float32)
    lo, hi = np.ascontiguousarray(allv.min(0)), np.ascontiguousarray(allv.max(0))
    nodes, order = np.ascontiguousarray(nodes), np.ascontiguousarray(order if len(order) else np.zeros(1, np.int32))
    n = len(rays)
    t, idx, just = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    _p = mesh_rays._p
    lib.mesh_walk_check_hit(_p(nodes), _p(order), len(kept), _p(lo), _p(hi), _p(s), len(s), _p(p), len(p), _p(rec), len(rec), _p(rays), n, _p(t), _p(idx),
                            _p(just))
    return t, idx, just


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_morton_layout_is_a_refit_hierarchy_in_key_order_that_the_walk_serves(lib, family):
    s, t, p, aim = FAMILIES[family]()
    t = np.ascontiguousarray(t, W.TRIANGLE_DTYPE)
    nodes, order = B.mesh_layout_morton(t)
    again = B.mesh_layout_morton(t)
    assert nodes.tobytes() == again[0].tobytes() and order.tobytes() == again[1].tobytes()                     # (vii)
    assert B.mesh_refit_layout(t, nodes, order).tobytes() == nodes.tobytes()                                  # (i)
    kept = np.flatnonzero(has_area(t))
    assert np.array_equal(np.sort(order), kept)                                                               # (ii)
    keys = morton_keys(t, kept)[order]
    ascending = (keys[1:] > keys[:-1]) | ((keys[1:] == keys[:-1]) & (order[1:] > order[:-1]))
    assert np.all(ascending), "position %d" % int(np.flatnonzero(~ascending)[0])                              # (iii)
    want_nodes, _ = B.mesh_layout(t)
    assert len(nodes) == len(want_nodes) and depth(nodes) == depth(want_nodes)                                # (iv)
    box, length = mesh_rays.scene_box(aim)
    rays = mesh_rays.adversarial_rays(aim, N_RAYS, seed=len(t), box=box, length=length)
    want = mesh_rays.linear_fold(lib, s, t, p, rays)
    got = walk(lib, s, t, p, rays, nodes, order)
    assert not np.any(got[2] == -2), "the traversal stack would overflow"
    bad = np.flatnonzero((got[0].view(np.uint32) != want[0].view(np.uint32)) | (got[1] != want[1]) | (got[2] != want[2]))
    assert bad.size == 0, "%d of %d rays differ, e.g. ray %d" % (bad.size, len(rays), bad[0])                 # (v)
    if len(kept) > 100:
        assert int(np.sum(want[2].astype(bool) & (want[1] >= len(s) + len(p)))) > N_RAYS // 20                # (not vacuously)


def test_all_keys_equal_order_by_index_and_a_flat_axis_counts_for_nothing():
    _, t, _, _ = FAMILIES["coincident300"]()
    assert np.array_equal(B.mesh_layout_morton(t)[1], np.arange(300))
    _, t, _ = mesh_rays.planar_grid()
    kept = np.arange(len(t))
    assert np.all(morton_keys(t, kept) & np.uint64(0x12492492492) == 0)                                      # no y bit (bits 3 i + 1)


def _raw(fn, t, capacity, with_order=True):
    t = np.ascontiguousarray(t, W.TRIANGLE_DTYPE)
    nodes, order, kept = np.zeros(max(1, capacity), B.BVH_NODE_DTYPE), np.zeros(max(1, len(t)), np.int32), C.c_int(-7)
    rc = fn(B._ptr(t) if len(t) else None, len(t), B._ptr(nodes), capacity, B._ptr(order) if with_order else None, C.byref(kept))
    return rc, kept.value


def test_refusals_and_return_codes_are_ptmi_mesh_layouts():
    lib = B.load_library()
    _, t, _ = W.mesh_room(2)
    cases = []
    for field, value in (("v1", np.nan), ("v0", np.inf), ("color", np.inf), ("illuminance", np.nan), ("brdf_param", -np.inf), ("v2", 3e38)):
        bad = t.copy()
        if bad[field].ndim == 2:
            bad[field][77, 1] = value
            if field == "v2":
                bad["v0"][77, 1] = -3e38                                             # finite vertices, an edge that is not
        else:
            bad[field][77] = value
        cases.append((bad, len(bad), True))
    cases += [(t, len(B.mesh_layout(t)[0]) - 1, True), (t, 0, True), (t, len(t), False), (t[:0], 1, False), (t[:0], 0, False), (t, len(t), True)]
    for tri, capacity, with_order in cases:
        got, want = _raw(lib.ptmi_mesh_layout_morton, tri, capacity, with_order), _raw(lib.ptmi_mesh_layout, tri, capacity, with_order)
        assert got == want, (got, want, capacity, with_order)
    assert _raw(lib.ptmi_mesh_layout_morton, cases[0][0], len(t))[0] == B.PTMI_EINVAL
    assert _raw(lib.ptmi_mesh_layout_morton, t, 3)[0] == B.PTMI_ELIMIT
    assert lib.ptmi_mesh_layout_morton(None, -1, None, 0, None, None) == lib.ptmi_mesh_layout(None, -1, None, 0, None, None) == B.PTMI_EINVAL
