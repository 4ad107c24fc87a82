"""ptmi_bvh_refit_layout, the host twin of ptmi_update_spheres' refit, and the one definition of the sphere boxes behind it
(csrc/ptmi_bvh_box.h), without a GPU.

ptmi_bvh_layout still returns the bytes it returned before the box arithmetic moved into the shared header: the sha256 digests of
(nodes, order) for six seeded scenes are recorded in tests/golden/bvh_layout_digests.json.  Recipe, run once with the library of the
commit BEFORE the header existed:
    for name, s in bvh_update_scenes.golden_scenes().items():
        nodes, order = binding.bvh_layout(s)
        out[name] = {"n_spheres": len(s), "n_nodes": len(nodes), "sha256": bvh_update_scenes.layout_digest(nodes, order)}
The refit of unchanged spheres gives ptmi_bvh_layout's nodes back byte for byte, and so does moving away and back; after a move every
sphere's padded box lies inside its leaf child's box, boxes nest exactly and inv_2r is the rounded-up value of the smallest radius
below; refusals write nothing; the CPU walk (tests/cxx/bvh_traverse.c) over the refitted layout picks the linear fold's hit."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bvh_rays  # noqa: E402
import bvh_update_scenes as scenes  # noqa: E402
import oracle as ora  # noqa: E402

binding = scenes.binding
W = scenes.world
FAMILIES = scenes.families()


def moved(s, amount, kind, seed=0):
    return W.with_sphere_geometry(s, W.displaced_spheres(W.sphere_geometry(s), amount, kind, seed))


def extent(s):
    return float(np.ptp(s["position"], axis=0).max()) if len(s) > 1 else 1.0


def round_up(v):
    """(float32)v, or its upper neighbour when that lies below v"""
    f = np.asarray(v, np.float64).astype(np.float32)
    low = f.astype(np.float64) < v
    return np.where(low, np.nextafter(f, np.float32(np.inf)), f)


def pad_of(s):
    r = np.abs(s["radius"].astype(np.float64))
    m = np.maximum(np.abs(s["position"].astype(np.float64)).max(axis=1), r)
    return r * (1.0 + 1.0 / 256.0) + (1.0 / 1048576.0) * m


def check_invariants(s, nodes, order):
    """every padded sphere inside its leaf child's box; an inner child's box exactly the union of the node's two stored boxes; inv_2r"""
    pad = pad_of(s)
    c = s["position"].astype(np.float64)
    r_below = {}
    for node_id in range(len(nodes) - 1, -1, -1):
        nd = nodes[node_id]
        mins = []
        for k in range(2):
            ref = int(nd["ref"][k])
            cen, half = nd["center"][k].astype(np.float64), nd["half"][k].astype(np.float64)
            if ref == -1:
                assert np.all(cen == 0) and np.all(half == -1) and nd["inv_2r"][k] == 0
                continue
            if ref >= 0:
                sub = nodes[ref]
                live = [j for j in range(2) if sub["ref"][j] != -1]
                lo = np.min([sub["center"][j].astype(np.float64) - sub["half"][j].astype(np.float64) for j in live], axis=0)
                hi = np.max([sub["center"][j].astype(np.float64) + sub["half"][j].astype(np.float64) for j in live], axis=0)
                r_min = r_below[ref]
            else:
                v = -1 - ref
                idx = order[(v >> 8):(v >> 8) + (v & 255)]
                lo, hi = (c[idx] - pad[idx, None]).min(axis=0), (c[idx] + pad[idx, None]).max(axis=0)
                r_min = float(np.abs(s["radius"][idx].astype(np.float64)).min())
            want_c = (0.5 * (lo + hi)).astype(np.float32)
            want_h = round_up(np.maximum(hi - want_c.astype(np.float64), want_c.astype(np.float64) - lo))
            assert nd["center"][k].tobytes() == want_c.tobytes() and nd["half"][k].tobytes() == want_h.astype(np.float32).tobytes(), (node_id, k)
            assert np.all(cen - half <= lo) and np.all(cen + half >= hi), (node_id, k)
            with np.errstate(divide="ignore"):
                want_inv = round_up(np.float64(1.0) / (2.0 * np.float64(r_min))) if r_min > 0 else np.float32(np.inf)
            assert np.float32(nd["inv_2r"][k]).tobytes() == np.float32(want_inv).tobytes(), (node_id, k, r_min)
            mins.append(r_min)
        r_below[node_id] = min(mins) if mins else np.inf


def test_bvh_layout_returns_the_bytes_it_returned_before_the_shared_header():
    with open(os.path.join(ROOT, "tests", "golden", "bvh_layout_digests.json")) as fh:
        gold = json.load(fh)
    made = scenes.golden_scenes()
    assert sorted(made) == sorted(gold) and len(gold) == 6
    for name, s in made.items():
        nodes, order = binding.bvh_layout(s)
        assert (len(s), len(nodes)) == (gold[name]["n_spheres"], gold[name]["n_nodes"]), name
        assert scenes.layout_digest(nodes, order) == gold[name]["sha256"], name


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_unchanged_spheres_and_away_and_back_give_the_layout_back(name):
    s, _ = FAMILIES[name]
    nodes, order = binding.bvh_layout(s)
    assert binding.bvh_refit_layout(s, nodes, order).tobytes() == nodes.tobytes()
    away = binding.bvh_refit_layout(moved(s, extent(s), "noise", 1), nodes, order)
    assert away.tobytes() != nodes.tobytes()
    assert np.array_equal(away["ref"], nodes["ref"])
    assert binding.bvh_refit_layout(s, away, order).tobytes() == nodes.tobytes()


@pytest.mark.parametrize("n", scenes.COUNTS)
def test_every_count_refits_to_its_own_layout(n):
    s, _ = scenes.field(n, seed=n)
    nodes, order = binding.bvh_layout(s)
    assert binding.bvh_refit_layout(s, nodes, order).tobytes() == nodes.tobytes()
    s2 = moved(s, 2.0, "noise", 2)
    assert binding.bvh_refit_layout(s, binding.bvh_refit_layout(s2, nodes, order), order).tobytes() == nodes.tobytes()


@pytest.mark.parametrize("name", sorted(FAMILIES))
@pytest.mark.parametrize("kind", ["wave", "noise"])
def test_after_a_move_boxes_hold_their_spheres_and_nest_exactly(name, kind):
    s, _ = FAMILIES[name]
    nodes, order = binding.bvh_layout(s)
    s2 = moved(s, 0.5 if kind == "wave" else extent(s), kind, 3)
    check_invariants(s2, binding.bvh_refit_layout(s2, nodes, order), order)
    check_invariants(s, nodes, order)


def test_refusals_write_nothing():
    s, _ = FAMILIES["adversarial"]
    nodes, order = binding.bvh_layout(s)
    lib = binding.load_library()

    def call(sph, nd, n_nodes, od):
        sph = np.ascontiguousarray(sph, binding.SPHERE_DTYPE)
        od = np.ascontiguousarray(od, np.int32)
        return lib.ptmi_bvh_refit_layout(sph.ctypes.data_as(C.c_void_p), len(sph), nd.ctypes.data_as(C.c_void_p), n_nodes, od.ctypes.data_as(C.c_void_p))

    s2 = moved(s, 1.0, "noise", 4)
    for what in ("nan", "inf radius", "radius^2", "short nodes", "twice in the order", "wrong count"):
        bad, work, od, n_nodes = s2.copy(), nodes.copy(), order.copy(), len(nodes)
        if what == "nan":
            bad["position"][17, 1] = np.nan
        elif what == "inf radius":
            bad["radius"][3] = np.inf
        elif what == "radius^2":
            bad["radius"][3] = 1e30
        elif what == "short nodes":
            n_nodes -= 1
        elif what == "twice in the order":
            od[5] = od[6]
        else:
            bad = bad[:-1]
        assert call(bad, work, n_nodes, od) == binding.PTMI_EINVAL, what
        assert work.tobytes() == nodes.tobytes(), what
    work = nodes.copy()
    assert call(s2, work, len(nodes), order) == binding.PTMI_OK and work.tobytes() != nodes.tobytes()


@pytest.fixture(scope="module")
def trav(tmp_path_factory):
    return bvh_rays.traverse_lib(tmp_path_factory.mktemp("bvhrefit"))


def walk_equals_fold(lib, s, p, nodes, order, rays):
    s = np.ascontiguousarray(s, ora.SPHERE_DTYPE)
    p = np.ascontiguousarray(p, ora.PLANE_DTYPE)
    nodes, order = np.ascontiguousarray(nodes), np.ascontiguousarray(order, np.int32)
    lo, hi = np.ascontiguousarray(s["position"].min(0)), np.ascontiguousarray(s["position"].max(0))
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = len(rays)
    t, idx, just = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib.bvh_check_hit(P(nodes), P(order), P(lo), P(hi), P(s), len(s), P(p), len(p), P(rays), n, P(t), P(idx), P(just))
    t0, i0, j0 = bvh_rays.linear_fold(lib, s, p, rays)
    assert not np.any(just == -2), "the traversal stack would overflow"
    bad = np.flatnonzero((t0.view(np.uint32) != t.view(np.uint32)) | (i0 != idx) | (j0 != just))
    assert bad.size == 0, "%d of %d rays differ, first %d" % (bad.size, n, bad[0])
    return int(j0.astype(bool).sum())


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_the_cpu_walk_over_the_refitted_layout_is_the_linear_fold(trav, name):
    s, p = FAMILIES[name]
    nodes, order = binding.bvh_layout(s)
    s2 = moved(s, 0.25 * extent(s), "noise", 6)
    rays = bvh_rays.adversarial_rays(s2, 100_000, seed=8)
    hits = walk_equals_fold(trav, s2, p, binding.bvh_refit_layout(s2, nodes, order), order, rays)
    assert hits > 10_000, hits
