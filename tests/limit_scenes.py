"""Scenes at the limits (PTMI_MAX_BVH_SPHERES, PTMI_MAX_MESH_TRIANGLES) for which a small scene is a bit-exact reference
(tests/test_limits_layout.py on the CPU, tests/test_gpu_limits.py on the device).

The core: world.mirror_box()'s closed room of six inward-facing perfect mirrors around initial_camera(), a few dozen spheres inside it
(Matte, Glossy, some GLASS, every fifth a light) and, for mesh scenes, a small icosphere (every fourth triangle GLASS); 64 planes, the
58 beyond the room's outside it and facing away.  The ballast: every other sphere or triangle, in a wide layer outside the room whose
nearest point is farther from the room's box than twice the room's diagonal.

The premise: a ray that starts inside the room meets a wall within one diagonal (a mirror's bounce is the exact reflection and a
sphere's or a triangle's starts where the ray was, so the renderer's rays never leave), the ballast is strictly farther, so it neither
wins nor ties, and the fold's order among the core primitives is the same.  Hence a render of the full scene equals the oracle's render
of the core scene bit for bit, and checkHit on the full scene is the core scene's fold with the index mapped (map_index).
premise_holds asserts the distances on the data; the large tests run the full literal fold on 256 rays besides."""
import numpy as np

import __graft_entry__ as graft

pkg = graft.load_package()
world, binding = pkg.world, pkg.binding

ROOM_LO, ROOM_HI = np.array([-6.0, -4.0, -14.0]), np.array([8.0, 4.0, 2.0])          # world.mirror_box()'s walls
DIAGONAL = float(np.linalg.norm(ROOM_HI - ROOM_LO))
CLEARANCE = 2.0 * DIAGONAL
N_PLANES = binding.MAX_BVH_PLANES
ROOM_PLANE_AT = (3, 17, 30, 41, 52, 63)                                              # where the six walls sit among the 64 planes
N_CORE_SPHERES = 40
ICO_CENTRE, ICO_RADIUS = np.array([2.5, -0.5, -9.5]), 1.3
# bvh_spatial_number_kernel sums the workgroups before it 256 at a time: a second trip needs a level of more than 256 * 257 nodes.  The
# spatial tree of spheres(SPATIAL_WIDE_COUNT) has one (tests/test_limits_layout.py finds it on the CPU; found by trying 2^20 first).
WIDE_LEVEL, SPATIAL_WIDE_COUNT = 256 * 257 + 1, 1 << 20


def planes():
    """64 planes: mirror_box()'s six walls at ROOM_PLANE_AT -- perfect mirrors still, of a colour that halves the throughput at every bounce, so
    that a Streams lineage ends after a few dozen steps, not several hundred -- the others outside the room, their normals pointing away
    from it (a ray from inside meets their back or runs away from them: never a hit)"""
    _, room = world.mirror_box()
    assert np.array_equal(room["position"].sum(0) + 0.0, ROOM_LO + ROOM_HI)
    p = np.zeros(N_PLANES, world.PLANE_DTYPE)
    pads = [j for j in range(N_PLANES) if j not in ROOM_PLANE_AT]
    for k, j in enumerate(pads):
        axis, side = k % 3, 1.0 if (k // 3) % 2 else -1.0
        pos, nrm = np.zeros(3), np.zeros(3)
        pos[axis] = (ROOM_HI if side > 0 else ROOM_LO)[axis] + side * (3.0 + k)
        nrm[axis] = side
        p[j] = world.plane(pos, nrm, (0.2 + 0.01 * k, 0.5, 0.7), 1.0 + k, world.MATTE if k % 2 else world.GLOSSY, 0.75)
    room["color"] = [(3.0, 2.8, 2.6), (2.6, 2.8, 3.0), (2.8, 3.0, 2.6), (3.0, 2.6, 2.8), (2.6, 3.0, 2.8), (2.8, 2.6, 3.0)]
    room["illuminance"] = 0.25                                          # (every path gathers light at every wall: no pixel stays black)
    p[list(ROOM_PLANE_AT)] = room
    return p


def core_spheres(glass=True, seed=0):
    """N_CORE_SPHERES spheres inside the room, none around the camera: Matte and Glossy, every fourth GLASS (Glossy when glass is false: render
    Inline and the Streams chain refuse GLASS), every fifth a light"""
    rng = np.random.default_rng(seed + 7000)
    cam = world.initial_camera()["position"].astype(np.float64)
    s = np.zeros(N_CORE_SPHERES, world.SPHERE_DTYPE)
    k = 0
    while k < len(s):
        r = 0.3 + 0.7 * rng.random()
        c = ROOM_LO + r + 0.2 + (ROOM_HI - ROOM_LO - 2.0 * (r + 0.2)) * rng.random(3)
        if np.linalg.norm(c - cam) < r + 1.0 or np.linalg.norm(c - ICO_CENTRE) < r + ICO_RADIUS + 0.2:
            continue
        s["position"][k], s["radius"][k] = c, r
        k += 1
    s["color"] = 0.2 + 0.75 * rng.random((len(s), 3))
    i = np.arange(len(s))
    s["illuminance"] = np.where(i % 5 == 1, 20.0, 0.0)
    s["brdf_tag"] = np.where(i % 2 == 0, world.GLOSSY, world.MATTE)
    s["brdf_param"] = np.where(i % 2 == 0, 0.8, 0.9)
    g = i % 4 == 3
    if glass:
        s["brdf_tag"][g], s["brdf_param"][g], s["color"][g] = world.GLASS, 1.5, (0.95, 0.95, 0.95)
    return s


def core_triangles(glass=True):
    """world.icosphere(2) inside the room (320 triangles), the farthest from the camera first -- the last 64, which alone have a fold index
    of 2^23 or more behind 2^22 spheres, 64 planes and the ballast triangles, are the ones the camera sees -- every fourth GLASS (Glossy
    when glass is false)"""
    v, f = world.icosphere(2)
    t = world.triangles_of(v * ICO_RADIUS + ICO_CENTRE, f, ((0.85, 0.75, 0.4), 0.0, world.GLOSSY, 0.8))
    centroid = (t["v0"].astype(np.float64) + t["v1"] + t["v2"]) / 3.0
    t = t[np.argsort(-np.linalg.norm(centroid - world.initial_camera()["position"], axis=1), kind="stable")].copy()
    t["brdf_tag"][1::2] = world.MATTE
    g = np.arange(len(t)) % 4 == 3
    if glass:
        t["brdf_tag"][g], t["brdf_param"][g], t["color"][g] = world.GLASS, 1.5, (0.95, 0.95, 0.95)
    return t


def _layer(rng, n, z_near, towards):
    """n centres in a layer as dense as world.sphere_field's (0.5 per unit volume, as wide and deep as it needs to be) that starts at
    z_near and extends in the direction `towards` (+1 or -1) of z"""
    w = float(np.sqrt(max(n, 1) / (0.5 * 17.6)))
    c = np.empty((n, 3), np.float32)
    c[:, 0] = 1.0 + (rng.random(n, dtype=np.float32) - 0.5) * w
    c[:, 1] = -2.8 + rng.random(n, dtype=np.float32) * 17.6
    c[:, 2] = z_near + towards * rng.random(n, dtype=np.float32) * w
    return c


def ballast_spheres(n, seed=0):
    """n spheres of sphere_field's radii and materials in a layer behind the room (z below the room's by CLEARANCE and more)"""
    rng = np.random.default_rng(seed + 7001)
    s = np.zeros(n, world.SPHERE_DTYPE)
    s["position"] = _layer(rng, n, ROOM_LO[2] - CLEARANCE - 2.0, -1.0)
    s["radius"] = 0.1 + 0.35 * rng.random(n, dtype=np.float32)
    s["color"] = 0.2 + 0.75 * rng.random((n, 3), dtype=np.float32)
    s["illuminance"] = np.where(rng.random(n, dtype=np.float32) < 0.02, 300.0, 0.0)
    glossy = rng.random(n, dtype=np.float32) < 0.3
    s["brdf_tag"] = np.where(glossy, world.GLOSSY, world.MATTE)
    s["brdf_param"] = np.where(glossy, 0.8, 0.75).astype(np.float32)
    return s


def ballast_triangles(n, seed=0):
    """n small triangles (sides up to 0.6) in a layer in front of the room (z above the room's by CLEARANCE and more), none of zero area"""
    rng = np.random.default_rng(seed + 7002)
    t = np.zeros(n, world.TRIANGLE_DTYPE)
    c = _layer(rng, n, ROOM_HI[2] + CLEARANCE + 2.0, 1.0)
    e1 = (rng.random((n, 3), dtype=np.float32) - 0.5) * np.float32(0.6)
    e2 = (rng.random((n, 3), dtype=np.float32) - 0.5) * np.float32(0.6)
    e2[:, 1] += np.where(np.abs(e1[:, 0]) > 0.01, 0.0, 0.3).astype(np.float32)
    t["v0"], t["v1"], t["v2"] = c, c + e1, c + e2
    area = np.linalg.norm(np.cross(t["v1"].astype(np.float64) - t["v0"], t["v2"].astype(np.float64) - t["v0"]), axis=1)
    flat = area < 1e-4                                                  # (a handful in 2^22: given a fixed shape)
    t["v1"][flat] = t["v0"][flat] + np.float32([0.25, 0.0, 0.0])
    t["v2"][flat] = t["v0"][flat] + np.float32([0.0, 0.25, 0.0])
    t["color"] = 0.2 + 0.75 * rng.random((n, 3), dtype=np.float32)
    t["illuminance"] = np.where(rng.random(n, dtype=np.float32) < 0.02, 300.0, 0.0)
    t["brdf_tag"] = np.where(rng.random(n, dtype=np.float32) < 0.3, world.GLOSSY, world.MATTE)
    t["brdf_param"] = 0.8
    return t


def _ordered(core, ballast, ordering):
    """-> (full, core, index map): "last" -- the core records are the last ones; "ends" -- half of them first, half last"""
    k = {"last": 0, "ends": len(core) // 2}[ordering]
    full = np.concatenate([core[:k], ballast, core[k:]])
    index = np.concatenate([np.arange(k), len(ballast) + np.arange(k, len(core))]).astype(np.int64)
    assert np.array_equal(full[index], core)
    return full, core, index


def spheres(total, ordering="last", glass=True, seed=0, n_core=N_CORE_SPHERES):
    """`total` spheres, n_core of them the (first) core spheres -> (full, core, index of every core sphere in full)"""
    core = core_spheres(glass, seed)[:n_core]
    return _ordered(core, ballast_spheres(total - len(core), seed), ordering)


def triangles(total, ordering="last", glass=True, seed=0):
    """`total` triangles, 320 of them the core icosphere -> (full, core, index of every core triangle in full)"""
    core = core_triangles(glass)
    return _ordered(core, ballast_triangles(total - len(core), seed), ordering)


def _beyond(points, radius):
    """the distance (float64) from the room's box to the nearest point of balls around `points`"""
    p = np.asarray(points, np.float64)
    gap = np.maximum(np.maximum(ROOM_LO - p, p - ROOM_HI), 0.0)
    return np.sqrt((gap * gap).sum(-1)) - radius


def premise_holds(s_full, s_index, t_full=None, t_index=None):
    """Asserts, in float64 on the data: every core primitive lies inside the room, every other one farther from the room's box than twice
    its diagonal and well within 2^40 of it, the camera is inside, and the ballast is spread out (no tight cluster)."""
    cam = world.initial_camera()["position"].astype(np.float64)
    assert np.all(ROOM_LO < cam) and np.all(cam < ROOM_HI)
    for full, index, what in ((s_full, s_index, "s"), (t_full, t_index, "t")):
        if full is None:
            continue
        core = np.zeros(len(full), bool)
        core[index] = True
        if what == "s":
            c, r = full["position"].astype(np.float64), np.abs(full["radius"].astype(np.float64))
            inside = np.all(c - r[:, None] > ROOM_LO, 1) & np.all(c + r[:, None] < ROOM_HI, 1)
            far, reach, centre = _beyond(c, r), np.abs(c).max(1) + r, c
        else:
            v = np.stack([full[k].astype(np.float64) for k in ("v0", "v1", "v2")], 1)
            inside = np.all(v > ROOM_LO, (1, 2)) & np.all(v < ROOM_HI, (1, 2))
            far, reach, centre = _beyond(v, 0.0).min(1), np.abs(v).max((1, 2)), v[:, 0]
        assert np.all(inside[core]), "a core primitive reaches out of the room"
        assert np.all(far[~core] > CLEARANCE), "ballast within twice the room's diagonal"
        assert np.all(reach < 2.0 ** 20), "a primitive far beyond what the walk serves"
        b = centre[~core]
        if len(b) > 1000:                                               # spread out: the layer is wider than 100 room diagonals' worth of
            assert np.ptp(b, axis=0).max() > np.sqrt(len(b) / 8.8) * 0.9   # sphere_field's density, and every tenth of it is populated
            assert np.all(np.histogram(b[:, 0], 10)[0] > len(b) // 20)
    return True


def map_index(idx, core_counts, full_counts, s_index, t_index=None):
    """a core scene's fold index (spheres ++ planes ++ triangles) -> the full scene's; -1 (a miss) stays.  counts: (spheres, planes)"""
    idx = np.asarray(idx, np.int64)
    (ns, npl), (fs, _) = core_counts, full_counts
    out = idx.copy()
    is_s = (idx >= 0) & (idx < ns)
    out[is_s] = s_index[idx[is_s]]
    is_p = (idx >= ns) & (idx < ns + npl)
    out[is_p] = idx[is_p] - ns + fs
    is_t = idx >= ns + npl
    if is_t.any():
        out[is_t] = fs + npl + t_index[idx[is_t] - ns - npl]
    return out.astype(np.int32)


def into_the_room(rays, margin=0.05):
    """the rays with every finite origin clamped into the room (a margin inside its walls); directions and non-finite origins kept"""
    r = np.array(rays, np.float32, copy=True)
    o = r[:, :3]
    ok = np.all(np.isfinite(o), 1)
    o[ok] = np.clip(o[ok], (ROOM_LO + margin).astype(np.float32), (ROOM_HI - margin).astype(np.float32))
    return np.ascontiguousarray(r)


def sphere_rays(core, n, seed=0):
    """bvh_rays.adversarial_rays aimed at the core spheres, from inside the room"""
    import bvh_rays
    return into_the_room(bvh_rays.adversarial_rays(core, n, seed))


def mesh_rays_for(core_s, core_t, n, seed=0):
    """half sphere_rays; a quarter mesh_rays.adversarial_rays aimed at the core triangles, a quarter at the last 64 of them, with origins
    drawn from the room"""
    import mesh_rays
    box = tuple((float(ROOM_LO[a]), float(ROOM_HI[a] - ROOM_LO[a])) for a in range(3))
    k = n - n // 2
    a = mesh_rays.adversarial_rays(core_t, k - k // 2, seed, box=box, length=ICO_RADIUS)
    b = mesh_rays.adversarial_rays(core_t[-64:], k // 2, seed + 1, box=box, length=ICO_RADIUS)
    return np.ascontiguousarray(np.concatenate([sphere_rays(core_s, n // 2, seed), into_the_room(a), into_the_room(b)]))


def camera_rays_at(triangles):
    """rays from initial_camera()'s position at the centroids of `triangles`"""
    cam = world.initial_camera()["position"].astype(np.float64)
    c = (triangles["v0"].astype(np.float64) + triangles["v1"] + triangles["v2"]) / 3.0 - cam
    d = c / np.linalg.norm(c, axis=1, keepdims=True)
    return np.ascontiguousarray(np.hstack([np.repeat(cam[None], len(d), 0), d]).astype(np.float32))


def level_counts(nodes):
    """the node count of every level of a hierarchy, the root's first; every node must be reached exactly once"""
    ref = nodes["ref"]
    seen = np.zeros(len(nodes), np.int32)
    frontier, counts = np.zeros(1, np.int64), []
    while len(frontier):
        counts.append(len(frontier))
        np.add.at(seen, frontier, 1)
        children = ref[frontier].reshape(-1)
        frontier = children[children >= 0].astype(np.int64)
        assert len(counts) <= len(nodes)
    assert np.all(seen == 1), "a node is reached %s" % ("twice" if seen.max() > 1 else "never")
    return counts


def served(rays, lo, hi):
    """Which rays the walks serve from a hierarchy whose primitives' box is lo .. hi (the others take the literal fold over every primitive,
    whatever the tree): the admission test of check_hit_bvh and check_hit_mesh in f32 -> bool per ray.  Used to CHOOSE rays only."""
    r = np.asarray(rays, np.float32)
    o, d = r[:, :3], r[:, 3:]
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    with np.errstate(all="ignore"):
        eta = np.abs(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) - np.float32(1.0))
        P2 = np.zeros(len(r), np.float32)
        for a in range(3):
            pa = np.maximum(np.abs(lo[a] - o[:, a]), np.abs(hi[a] - o[:, a]))
            P2 = P2 + pa * pa
        P = np.sqrt(P2) * (np.float32(1.0) + np.float32(2.0 ** -20))
    return np.all(np.isfinite(r), 1) & (eta <= np.float32(2.0 ** -12)) & (P <= np.float32(2.0 ** 40))


def walked_rays(rays, lo, hi, unserved=64):
    """the indices of the rays a CPU walk over a tree of millions is given: every served ray, and `unserved` of the others (each of
    those costs a literal fold over every primitive)"""
    ok = served(rays, lo, hi)
    return np.sort(np.concatenate([np.flatnonzero(ok), np.flatnonzero(~ok)[:unserved]]))


def in_slices(fold, rays, slices=16):
    """fold(rays) -> (t, idx, just) over a few hundred rays, `slices` calls at once on threads of their own: the C folds hand out 256
    consecutive rays to a thread, so one call over 256 rays runs on one"""
    from concurrent.futures import ThreadPoolExecutor
    parts = [np.ascontiguousarray(a) for a in np.array_split(np.asarray(rays, np.float32), slices) if len(a)]
    with ThreadPoolExecutor(len(parts)) as pool:
        res = list(pool.map(fold, parts))
    return tuple(np.concatenate([r[k] for r in res]) for k in range(3))


def mesh_fold_in_slices(lib, spheres, triangles, planes, rays, slices=16):
    """mesh_rays.linear_fold (the literal fold over spheres ++ planes ++ triangles, lib: mesh_rays.traverse_lib) with the triangles'
    records made once, in_slices"""
    import ctypes as C
    import mesh_rays
    import oracle as ora
    s = np.ascontiguousarray(spheres, ora.SPHERE_DTYPE)
    p = np.ascontiguousarray(planes, ora.PLANE_DTYPE)
    rec = mesh_rays.records(lib, triangles)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def fold(r):
        t, idx, just = np.zeros(len(r), np.float32), np.zeros(len(r), np.int32), np.zeros(len(r), np.int32)
        lib.mesh_lin_check_hit(P(s), len(s), P(p), len(p), P(rec), len(rec), P(r), len(r), P(t), P(idx), P(just))
        return t, idx, just
    return in_slices(fold, rays, slices)
