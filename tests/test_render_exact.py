"""The oracle (oracle/pt_oracle.c; tests/cxx/mesh_reference.c for triangles) held to tests/exact_render.py, the float64 restatement of
the reference's text: per decided pixel the generator planes are the reference's exactly and the colour is within the reference's own
error bound; the undecided share is capped, every case shows what it is there to show, and thirteen misreadings of the text, each put
into a copy of the oracle, are caught.  (tests/test_gpu_render_exact.py holds the device to the same reference.)"""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_render as X  # noqa: E402
import mesh_rays  # noqa: E402
import render_cases as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = max(1, min(16, os.cpu_count() or 1))
STREAM_CAP = 1 << 16                    # the reference has no cap (Trace.hs:166-170); exact_render gets 64 and reports what it cuts
TREE_CAP = 6

# (scene, camera, size index, mode, limit, samples, what the case is there to show)
CASES = [
    ("main", "turned60", 0, X.INLINE, 0, 1, ()),
    ("main", "turned90", 1, X.INLINE, 1, 1, ("sphere", "plane", "matte", "glossy")),
    ("main", "turned60", 0, X.INLINE, 2, 2, ("sphere", "plane", "matte", "glossy")),
    ("main", "turned60", 1, X.INLINE, 4, 1, ("three_hits", "near_zero_end")),
    ("main", "turned90", 0, X.INLINE, 4, 2, ("three_hits", "near_zero_end", "miss_end")),
    ("main", "turned60", 0, X.INLINE, 15, 2, ("three_hits", "near_zero_end")),
    ("scene16", "turned60", 0, X.INLINE, 4, 2, ("three_hits", "sphere", "plane")),
    ("scene16", "turned90", 1, X.INLINE, 15, 1, ("sphere", "plane")),
    ("mirror", "initial", 0, X.INLINE, 4, 1, ("three_hits", "glossy", "plane")),
    ("mirror", "turned60", 1, X.INLINE, 2, 2, ("glossy", "plane")),
    ("dim", "initial", 0, X.INLINE, 4, 2, ("near_zero_end", "matte")),
    ("dim", "turned90", 0, X.STREAMS_FROM_RESULT, 64, 2, ("near_zero_end", "three_hits")),
    ("dim", "initial", 1, X.STREAMS_KEEP, 64, 2, ("near_zero_end",)),
    ("main", "turned60", 0, X.STREAMS_FROM_RESULT, 64, 1, ("near_zero_end",)),
    ("main", "turned90", 1, X.STREAMS_KEEP, 64, 2, ("near_zero_end",)),
    ("glass", "initial", 0, X.TREE, TREE_CAP, 1, ("glass_both",)),
    ("glass", "turned90", 1, X.TREE, TREE_CAP, 1, ("glass_both",)),
    ("mesh", "initial", 0, X.INLINE, 4, 2, ("triangle", "glossy")),
    ("mesh", "turned90", 1, X.INLINE, 15, 1, ("triangle",)),
    ("mesh", "initial", 1, X.STREAMS_FROM_RESULT, 64, 1, ("triangle",)),
    ("mesh_glass", "initial", 0, X.TREE, TREE_CAP, 2, ("triangle", "glass_both")),
    ("glass_low", "initial", 0, X.TREE, TREE_CAP, 1, ("glass_both", "tir")),
]
IDS = ["%s-%s-%dx%d-%s-l%d-s%d" % (c[0], c[1], *R.SIZES[c[2]], c[3], c[4], c[5]) for c in CASES]


@pytest.fixture(scope="module")
def mesh_lib(tmp_path_factory):
    return mesh_rays.reference_lib(tmp_path_factory.mktemp("render_exact_mesh"))


def oracle_render(ora, case, start, mesh_lib=None, calls=1):
    """The oracle's seven planes for a case, `calls` calls of samples / calls each"""
    name, camera, size, mode, limit, spp, _ = case
    w, h = R.SIZES[size]
    s, p, t = R.scene(name)
    cam = R.CAMERAS[camera]()

    def run(o):
        planes = start
        for _ in range(calls):
            n = spp // calls
            if mode == X.INLINE:
                planes = o.render_inline(s, p, cam, w, h, limit, n, planes, n_threads=THREADS)[0]
            elif mode == X.TREE:
                planes = o.render_streams_tree(s, p, cam, w, h, limit, n, planes, n_threads=THREADS)[0]
            else:
                rule = o.SEED_FROM_RESULT if mode == X.STREAMS_FROM_RESULT else o.SEED_KEEP_ACCUMULATOR
                planes, _, truncated = o.render_streams(s, p, cam, w, h, STREAM_CAP, n, planes, seed_rule=rule, want_truncated=True, n_threads=THREADS)
                assert truncated == 0
        return planes
    if t is None:
        return run(ora)
    with mesh_rays.MeshOracle(mesh_lib, t) as mo:
        return run(mo)


def check(ora, case, mesh_lib=None, calls=1, verbose=True):
    name, camera, size, mode, limit, spp, needs = case
    w, h = R.SIZES[size]
    start = R.start_planes(w, h)
    ref = R.reference(name, camera, w, h, mode, limit, spp)
    what = "%s, %s, %d x %d, %s, limit %d, %d samples in %d calls" % (name, camera, w, h, mode, limit, spp, calls)
    R.assert_not_vacuous(ref, what, needs)
    return R.compare(ref, oracle_render(ora, case, start, mesh_lib, calls), start, mode, limit, spp, what, verbose)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_oracle_is_within_the_references_bound(ora, mesh_lib, case):
    check(ora, case, mesh_lib)


@pytest.mark.parametrize("case", [CASES[2], CASES[11], CASES[20]], ids=[IDS[2], IDS[11], IDS[20]])
def test_two_calls_are_one_call_of_two_samples(ora, mesh_lib, case):
    """The second call starts from the planes the first left: the carried seed and the f32 colour"""
    check(ora, case, mesh_lib, calls=2)


NEEDED = {"three_hits": "a path of three hits or more", "matte": "a Matte bounce", "glossy": "a Glossy bounce",
          "glass_both": "a GLASS split with both children hitting something", "tir": "a total internal reflection", "sphere": "a hit on a sphere",
          "plane": "a hit on a plane", "triangle": "a hit on a triangle", "near_zero_end": "a sample ended by nearZero", "miss_end": "a sample ended by a miss"}


def test_the_generator_is_the_oracles(ora):
    """exact_render's reading of the generator (A1, A2, A4) against the oracle's on a few words: the seeding (render()'s start planes are
    data, so nothing else exercises sfc32_seed), the step and random @Float"""
    words = np.array([[0, 0, 0], [1, 2, 3], [0xFFFFFFFF, 0x80000000, 0x7FFFFFFF], [0x5EED1234, 0x9E3779B9, 0xDEADBEEF]], np.uint32)
    got = X.sfc32_seed(words[:, 0], words[:, 1], words[:, 2])
    for k, w in enumerate(words):
        state = ora.sfc32_seed3(*w)
        assert tuple(int(x[k]) for x in got) == tuple(state), w
        raw, flt, end = ora.sfc32_stream(state, 40)
        mine = tuple(x[k:k + 1] for x in got)
        for i in range(40):
            out, stepped = X.sfc32_step(mine)
            x, mine = X.random_float(mine)
            assert int(out[0]) == int(raw[i]) and x[0] == np.float64(flt[i]), (w, i)
            assert all(np.array_equal(a, b) for a, b in zip(stepped, mine))
        assert tuple(int(x[0]) for x in mine) == tuple(end)


def test_the_cases_together_are_not_vacuous_and_stay_inside_the_caps():
    """The reference alone: every cap holds for its classification, and over all cases at least 200 decided pixels show each property"""
    total = dict.fromkeys(NEEDED, 0)
    for name, camera, size, mode, limit, spp, _ in CASES:
        w, h = R.SIZES[size]
        ref = R.reference(name, camera, w, h, mode, limit, spp)
        share = 1.0 - ref["decided"].mean()
        assert share <= R.CAP_SHARE["short" if (mode == X.INLINE and limit <= 4) else "long"], (name, camera, mode, limit, share)
        for k in total:
            total[k] += int((ref["stats"][k] & ref["decided"]).sum())
    print("decided pixels with each property, all cases:", total)
    for k, n in total.items():
        assert n >= 200, "only %d decided pixels with %s" % (n, NEEDED[k])


# ---- discrimination: misreadings of the text, each put into a copy of the oracle ---------------------------------------------------------
MUTANTS = {
    "two Euler angles swapped": ("float roll = angles.x, pitch = angles.y, yaw = angles.z;", "float roll = angles.y, pitch = angles.x, yaw = angles.z;", 1, "colour"),
    "epsilon halved": ("ORA_EPSILON = 0.002f;", "ORA_EPSILON = 0.001f;", 10, "colour"),
    "nextRayProb 1 / pi": ("float next_ray_prob = 1.0f / (ORA_PI * 2.0f);", "float next_ray_prob = 1.0f / ORA_PI;", 2, "planes"),
    "a draw not mapped to [-1, 1]": ("r.x = (ora_random_float(s) * 2.0f) - 1.0f;", "r.x = ora_random_float(s);", 2, "planes"),
    "the fold's <= made <": ("else if (!(acc_key <= key)) { acc = h; acc_key = key; }   /* cond", "else if (!(acc_key < key)) { acc = h; acc_key = key; }   /* cond", 10, "planes"),
    "screenY's offset dropped": ("raster_y / size_y * 2.0f + 1.0f;", "raster_y / size_y * 2.0f;", 1, "colour"),
    "topOffset's aspect division dropped": ("ora_v3 top = v3_div(v3_cross(c_dir, right), screen_aspect);", "ora_v3 top = v3_cross(c_dir, right); (void)screen_aspect;", 1, "colour"),
    "Glossy's 1 - p made p": ("v3_scale_l(1.0f - p, rotation_vector)", "v3_scale_l(p, rotation_vector)", 2, "planes"),
    "Matte's dot taken against the ray": ("brdf = p / ORA_PI * v3_dot(next, i_normal);", "brdf = p / ORA_PI * v3_dot(next, ray.direction);", 2, "planes"),
    "emittance added after the throughput update": (
        "result = v3_add(result, v3_mul(emittance, throughput));\n            throughput = v3_mul(throughput, tmod);",
        "throughput = v3_mul(throughput, tmod);\n            result = v3_add(result, v3_mul(emittance, throughput));", 2, "colour"),
    "GLASS's eta inverted": ("float eta = 1.0f / ior;", "float eta = ior;", 15, "colour"),
    "child 1 given child 0's seed": ("(void)ora_random_float(&seed);\n    out[1].seed = seed;", "out[1].seed = seed;", 16, "colour"),
    "updateSeed skipped": ("(void)ora_random_float(&pixel_seed);      /* updateSeed */", "/* updateSeed */", 12, "planes"),
}


# What compare() says of a mutant.  The generator planes are compared first, and Inline's and FROM_RESULT's carry out the state the last
# live bounce left: a misreading that moves where some path ENDS (a draw's direction, or a throughput that passes nearZero a bounce sooner or
# later) shows there.  One that leaves every path's length alone -- another primitive hit first in a closed scene at limit 1, the order of
# two updates, the tree's children under the keep-accumulator rule -- shows in the colour.
FAILS = {"colour": r"decided pixels are outside their bound", "planes": r"plane sfc_\w+ differs from the reference at \d+ decided pixels"}


class _Mutant:
    """The oracle module's wrappers over another build of pt_oracle.c (as mesh_rays.MeshOracle points them at the mesh reference)"""

    def __init__(self, ora, path):
        self.ora, self.lib = ora, C.CDLL(path)
        base = ora.lib()
        for name in ("ora_render_inline_ex", "ora_render_streams_ex", "ora_render_streams_tree"):
            fn, want = getattr(self.lib, name), getattr(base, name)
            fn.restype, fn.argtypes = want.restype, want.argtypes

    def __enter__(self):
        self.saved = self.ora.lib
        self.ora.lib = lambda: self.lib
        return self.ora

    def __exit__(self, *exc):
        self.ora.lib = self.saved
        return False


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_misreading_of_the_text_is_caught(ora, tmp_path, name):
    old, new, case, how = MUTANTS[name]
    for f in ("pt_oracle.c", "pt_oracle.h", "Makefile"):
        shutil.copy(os.path.join(ROOT, "oracle", f), tmp_path)
    src = tmp_path / "pt_oracle.c"
    text = src.read_text()
    assert text.count(old) == 1, "the substitution for %r matches %d times" % (name, text.count(old))
    src.write_text(text.replace(old, new))
    lib = str(tmp_path / "libptoracle.so")
    res = subprocess.run(["make", "-s", "-C", str(tmp_path), "-f", str(tmp_path / "Makefile"), lib], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    check(ora, CASES[case])                                  # the unchanged oracle passes this case ...
    with _Mutant(ora, lib) as mutant:                        # ... and the mutant fails the comparison itself, in the way its misreading must
        with pytest.raises(AssertionError, match=FAILS[how]) as e:
            check(mutant, CASES[case], verbose=False)
    print("%s: %s" % (name, str(e.value)[:200]))
