"""Scenes, cameras, cases and the comparison shared by tests/test_render_exact.py (the oracle held to tests/exact_render.py) and
tests/test_gpu_render_exact.py (the device held to it).  Every primitive has a colour of its own and a non-zero illuminance, so a pixel's
colour tells which primitives its path met and every BRDF factor along it.  The reference of a case is computed once and kept."""
import functools
import os
import sys

import numpy as np

import __graft_entry__ as graft

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_render as X  # noqa: E402
import mesh_rays  # noqa: E402

pkg = graft.load_package()
world = pkg.world
SEED0 = 0x5EED1234
CAP_SHARE = {"short": 0.10, "long": 0.25}             # undecided pixels: limit <= 4; limit 15 and Streams
SIZES = ((64, 48), (37, 23))


def recoloured(scene):
    """The scene with colour k and illuminance k of its own for primitive k (the geometry and the BRDFs stay)"""
    out = []
    k = 0
    for part in scene:
        part = part.copy()
        for i in range(len(part)):
            part["color"][i] = (0.35 + 0.6 * ((k * 7) % 11) / 10.0, 0.35 + 0.6 * ((k * 5) % 13) / 12.0, 0.35 + 0.6 * ((k * 3) % 7) / 6.0)
            part["illuminance"][i] = 0.5 + 0.75 * ((k * 4) % 9)
            k += 1
        out.append(part)
    return tuple(out)


def mirror_rooms():
    """world.mirror_box() with Glossy p of 0, 0.3 and 1 on its three pairs of walls"""
    s, p = recoloured(world.mirror_box())
    p["brdf_param"] = [0.0, 0.0, 0.3, 0.3, 1.0, 1.0]
    p["color"] *= 6.2 / p["color"].max(1, keepdims=True)
    return s, p


def dim_room():
    """A closed Matte room around initial_camera() with albedo <= 0.05: a bounce keeps at most 0.05 (1 / pi) / (2 pi) = 0.0025 of the
    throughput, whose square passes nearZero's 1e-6 after three bounces, so Streams paths end by nearZero within a few steps.  Sphere 1
    coincides with sphere 0 under another colour: an exact tie, which the fold's `<=` gives to sphere 0.  The last plane lies 0.0012 above the
    floor and faces it: rays from the room pass through its back, and a ray that leaves the floor starts 0.002 cos above the floor --
    beyond that plane or under it, which is where `epsilon` shows (a shift of an origin along its own ray moves no other hit)."""
    M = world.MATTE
    spheres = np.array([world.sphere((1.0, -1.0, -9.0), 1.25, (0.05, 0.03, 0.02), 3.0, M, 1.0),
                        world.sphere((1.0, -1.0, -9.0), 1.25, (0.01, 0.04, 0.05), 9.0, M, 1.0),
                        world.sphere((-2.5, 0.5, -7.0), 0.75, (0.03, 0.05, 0.03), 5.0, M, 0.9)], dtype=world.SPHERE_DTYPE)
    walls = [((0.0, -4.0, 0.0), (0.0, 1.0, 0.0)), ((0.0, 4.0, 0.0), (0.0, -1.0, 0.0)), ((-6.0, 0.0, 0.0), (1.0, 0.0, 0.0)),
             ((8.0, 0.0, 0.0), (-1.0, 0.0, 0.0)), ((0.0, 0.0, -14.0), (0.0, 0.0, 1.0)), ((0.0, 0.0, 2.0), (0.0, 0.0, -1.0)),
             ((0.0, -4.0 + 0.0012, 0.0), (0.0, -1.0, 0.0))]
    planes = np.array([world.plane(pos, nor, (0.05 - 0.005 * k, 0.02 + 0.005 * k, 0.035), 1.0 + k, M, 1.0) for k, (pos, nor) in enumerate(walls)],
                      dtype=world.PLANE_DTYPE)
    return spheres, planes


def mesh_room(glass):
    """mesh_rays.closed_room (the room, its icosphere, duplicates, zero areas) recoloured; the icosphere is Glossy, and with `glass` every
    fourth of its triangles GLASS"""
    s, t, p = mesh_rays.closed_room(1)
    (t,) = recoloured((t,))
    if glass:
        k = np.arange(13, len(t), 4)
        t["brdf_tag"][k], t["brdf_param"][k] = world.GLASS, 1.5
    return s, p, t


@functools.lru_cache(None)
def scene(name):
    """-> (spheres, planes, triangles or None)"""
    if name == "main":
        return recoloured(world.main_scene()) + (None,)
    if name == "scene16":
        return recoloured(world.scene16()) + (None,)
    if name == "glass":
        return world.glass_scene() + (None,)
    if name == "glass_low":                            # an index of refraction below 1: eta > 1, so grazing rays are totally reflected
        s, p = world.glass_scene()
        s = s.copy()
        s["brdf_param"][[0, 7]] = 0.6
        return s, p, None
    if name == "mirror":
        return mirror_rooms() + (None,)
    if name == "dim":
        return dim_room() + (None,)
    if name == "mesh":
        return mesh_room(False)
    if name == "mesh_glass":
        return mesh_room(True)
    raise KeyError(name)


CAMERAS = {"initial": lambda: world.initial_camera(),
           "turned60": lambda: world.camera((1.0, -1.6, -4.8), (0.3, -0.7, 1.1), 60),       # three distinct non-zero angles: a swapped axis shows
           "turned90": lambda: world.camera((1.0, -1.6, -4.8), (0.3, -0.7, 1.1), 90)}


def start_planes(w, h):
    """conftest.initial_planes: zero colour and the oracle's deterministic seeds (data: any generator state serves the reference)"""
    from conftest import initial_planes
    ora = graft.load_oracle()
    ora.build()
    return initial_planes(ora, w, h, SEED0)


@functools.lru_cache(None)
def reference(scene_name, camera, w, h, mode, limit, spp):
    s, p, t = scene(scene_name)
    ref = X.render(X.Scene(s, p, t), CAMERAS[camera](), w, h, mode, limit, spp, start_planes(w, h)[3:])
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def compare(ref, got, start, mode, limit, spp, what, verbose=True):
    """The seven planes `got` of the code under test against the reference `ref` (exact_render.render's dict):
      decided pixels: the four generator planes equal the reference's; |colour - reference| <= bound per channel
      undecided pixels: finite colours; the counter moved by a count the algorithm allows
      and the undecided share is within its cap.  -> figures (largest error / bound, undecided share)"""
    dec = ref["decided"]
    share = 1.0 - float(dec.mean())
    cap = CAP_SHARE["short" if (mode == X.INLINE and limit <= 4) else "long"]
    colour = np.stack([np.asarray(g, np.float64).reshape(-1) for g in got[:3]], 1) - \
        np.stack([np.asarray(g, np.float64).reshape(-1) for g in start[:3]], 1)
    err, bound = np.abs(colour - ref["colour"]), ref["bound"]
    with np.errstate(all="ignore"):
        ratio = np.where(err <= bound, np.where(bound > 0, err / bound, 0.0), np.inf)
    ratio = np.where(np.isfinite(colour), ratio, np.inf)
    worst = float(ratio[dec].max()) if dec.any() else 0.0
    if verbose:
        print("%s: undecided %.1f %% (cap %.0f %%), largest error / bound over %d decided pixels %.3g" % (what, 100 * share, 100 * cap, int(dec.sum()), worst))
    assert share <= cap, "%s: %.1f %% of the pixels are undecided, the cap is %.0f %%" % (what, 100 * share, 100 * cap)
    assert ref["truncated"] == 0 or mode in (X.TREE, X.INLINE), "%s: the reference's cap cut %d rays" % (what, ref["truncated"])
    for name, g, r in zip(("sfc_a", "sfc_b", "sfc_c", "sfc_counter"), got[3:], ref["seeds"]):
        bad = np.flatnonzero((np.asarray(g).reshape(-1) != r) & dec)
        assert bad.size == 0, "%s: plane %s differs from the reference at %d decided pixels, first %d" % (what, name, bad.size, bad[0])
    bad = np.flatnonzero((ratio > 1.0).any(1) & dec)
    assert bad.size == 0, "%s: %d decided pixels are outside their bound, e.g. pixel %d: got %r, reference %r, bound %r, hits %r" % (
        what, bad.size, bad[0], colour[bad[0]].tolist(), ref["colour"][bad[0]].tolist(), bound[bad[0]].tolist(), ref["hits"][bad[0]].tolist())
    assert np.all(np.isfinite(colour[~dec])), "%s: an undecided pixel is not finite" % what
    moved = X.counter_moves_allowed(mode, limit, spp, start[6], got[6])
    assert np.all(moved[~dec]), "%s: an undecided pixel's counter moved by a count the algorithm does not allow" % what
    return {"ratio": worst, "undecided": share}


def assert_not_vacuous(ref, what, needs):
    """At least 40 decided pixels of the case show each property in `needs` (the whole suite's counts: test_render_exact.py)"""
    for name in needs:
        n = int((ref["stats"][name] & ref["decided"]).sum())
        assert n >= 40, "%s: only %d decided pixels with %s" % (what, n, name)
