"""Scenes, sphere counts and data families shared by the tests of moving and replacing a BVH scene's spheres
(tests/test_bvh_refit_layout.py, test_bvh_morton_layout.py on the CPU, test_gpu_bvh_update.py on the device)."""
import hashlib

import numpy as np

import bvh_rays

pkg = bvh_rays.pkg
world = pkg.world
binding = pkg.binding

# the smallest counts at which each piece can go wrong: the empty tree, a root with one leaf, the first split, the block edge of the
# records and level kernels, one sort tile and several, 18 tiles and 15 levels
COUNTS = (0, 1, 4, 5, 8, 9, 255, 256, 257, 4096, 4097, 12289, 70001)


def field(n, seed=0):
    """exactly n spheres of world.sphere_field (which appends a few of its own), and its planes"""
    s, p = world.sphere_field(max(n, 1), seed)
    if len(s) < n:
        s = np.concatenate([s, world.sphere_field(n, seed + 1)[0]])
    return np.ascontiguousarray(s[:n]), p


def coincident(n, seed=0):
    """n spheres on n // 3 + 1 distinct centres: equal keys, where the index decides"""
    s, p = field(n, seed)
    s["position"] = s["position"][np.arange(n) % (n // 3 + 1)]
    return s, p


def flat(n, axis, seed=0):
    """every centre equal on one axis: hi == lo there"""
    s, p = field(n, seed)
    s["position"][:, axis] = np.float32(1.5)
    return s, p


def odd_radii(n, seed=0):
    """a tenth of the radii 0, a tenth negative"""
    s, p = field(n, seed)
    s["radius"][::10] = 0.0
    s["radius"][5::10] *= -1.0
    return s, p


def far_small(n, seed=0):
    """centres at 1e7 with radii of 1e-3"""
    s, p = field(n, seed)
    s["position"] = (s["position"].astype(np.float64) + 1e7).astype(np.float32)
    s["radius"] = np.float32(1e-3)
    return s, p


def families(n=600, seed=0):
    """name -> (spheres, planes): bvh_rays' scenes and the families above"""
    adv = bvh_rays.adversarial_scene(n, seed)
    return {
        "adversarial": adv,
        "multiscale": bvh_rays.multiscale_field(n, seed),
        "transformed": bvh_rays.transformed(adv, 2.0 ** 12, (3e5, 1e5, -7e5)),
        "coincident": coincident(n, seed),
        "flat_x": flat(n, 0, seed),
        "flat_z": flat(n, 2, seed),
        "odd_radii": odd_radii(n, seed),
        "far_small": far_small(n, seed),
    }


def golden_scenes():
    """the six seeded scenes of tests/golden/bvh_layout_digests.json"""
    return {
        "adversarial_3000_s0": bvh_rays.adversarial_scene(3000, 0)[0],
        "adversarial_257_s3": bvh_rays.adversarial_scene(257, 3)[0],
        "multiscale_3000_s1": bvh_rays.multiscale_field(3000, 1)[0],
        "field_70001_s2": field(70001, 2)[0],
        "coincident_1000_s4": coincident(1000, 4)[0],
        "odd_radii_5_s5": odd_radii(5, 5)[0],
    }


def layout_digest(nodes, order):
    return hashlib.sha256(np.ascontiguousarray(nodes).tobytes() + np.ascontiguousarray(order, np.int32).tobytes()).hexdigest()


def wave(g, amount, phase=0.0):
    """a smooth displacement of [n, 4] geometry: every centre moves by up to `amount` along y, radii stay"""
    out = np.array(g, np.float32, copy=True)
    out[:, 1] += (amount * np.sin(out[:, 0].astype(np.float64) * 0.7 + phase)).astype(np.float32)
    return out
