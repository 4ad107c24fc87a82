"""The device held to tests/exact_render.py, the float64 restatement of the reference's text, through the C ABI: one case per kernel
family, so that none is covered only by way of the oracle.  Scenes, cameras, sizes, assertions and caps are tests/test_render_exact.py's
(tests/render_cases.py); each reference is computed once."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_render as X  # noqa: E402
import render_cases as R  # noqa: E402

pytestmark = pytest.mark.gpu
TREE_CAP = 6
RULES = {X.STREAMS_KEEP: "SEED_KEEP_ACCUMULATOR", X.STREAMS_FROM_RESULT: "SEED_FROM_RESULT", X.TREE: "SEED_KEEP_ACCUMULATOR"}


def set_scene(c, name, how="linear"):
    s, p, t = R.scene(name)
    if t is not None:
        c.set_scene_mesh(s, t, p)
    elif how == "bvh":
        c.set_scene_bvh(s, p)
    else:
        c.set_scene(s, p)


def device_planes(c, pkg, name, camera, w, h, mode, limit, spp, start, how="linear", calls=1):
    """The context's seven planes after `calls` calls of spp / calls samples from `start` (the scene is set by `how`)"""
    B = pkg.binding
    if how is not None:
        set_scene(c, name, how)
    c.resize(w, h)
    c.upload_state(*start)
    cam = R.CAMERAS[camera]()
    if mode == X.INLINE:
        for _ in range(calls):
            c.render(cam, limit, spp // calls, pkg.INLINE)
        return c.download_state()
    c.set_option(B.OPT_STREAMS_SEED_RULE, getattr(B, RULES[mode]))
    if mode == X.TREE:
        c.set_option(B.OPT_STREAM_STEP_CAP, limit)
    try:
        for _ in range(calls):
            c.render(cam, 15, spp // calls, pkg.STREAMS)
        return c.download_state()
    finally:
        c.set_option(B.OPT_STREAMS_SEED_RULE, B.SEED_AUTO)
        c.set_option(B.OPT_STREAM_STEP_CAP, 1 << 16)


def held(got, start, name, camera, w, h, mode, limit, spp, what):
    ref = R.reference(name, camera, w, h, mode, limit, spp)
    return R.compare(ref, got, start, mode, limit, spp, "device, " + what + ": %s, %s, %d x %d, %s, limit %d, %d samples" % (name, camera, w, h, mode, limit, spp))


INLINE_2_SAMPLES, INLINE_1_SAMPLE = ("main", "turned60", 64, 48, 4, 2), ("scene16", "turned90", 37, 23, 15, 1)


@pytest.mark.parametrize("variant, chunks, case", [(13, 1, INLINE_2_SAMPLES), (13, 1, INLINE_1_SAMPLE), (13, 4, INLINE_2_SAMPLES),
                                                   (17, 1, INLINE_2_SAMPLES), (17, 1, INLINE_1_SAMPLE), (17, 4, INLINE_2_SAMPLES)])
def test_inline_on_a_linear_scene_lds_and_scalar_loads(pkg, variant, chunks, case):
    """8 x 8 tiles with the scene in LDS (13) and through scalar loads (17), in one launch and with PTMI_OPT_SPP_CHUNKS 4.  No case here
    has more than 2 samples, and the launcher gives no copy of the tile grid less than one sample: with 4 chunks asked for, the 2-sample
    case runs as two chained copies of one sample each (the hand-over of the planes between copies is what it shows); a 1-sample case
    would be the launch of 1 chunk again, so it is not run with chunks."""
    name, camera, w, h, limit, spp = case
    start = R.start_planes(w, h)
    with pkg.Context(0) as c:
        c.set_variant(variant)
        c.set_option(pkg.binding.OPT_SPP_CHUNKS, chunks)
        got = device_planes(c, pkg, name, camera, w, h, X.INLINE, limit, spp, start)
    held(got, start, name, camera, w, h, X.INLINE, limit, spp, "variant %d, %d chunks" % (variant, chunks))


@pytest.mark.parametrize("case", [("main", "turned90", 37, 23, 1, 1), ("mirror", "initial", 64, 48, 4, 1), ("dim", "initial", 64, 48, 4, 2),
                                  ("main", "turned60", 64, 48, 0, 1)])
def test_inline_by_the_automatic_choice(ctx, pkg, case):
    name, camera, w, h, limit, spp = case
    start = R.start_planes(w, h)
    held(device_planes(ctx, pkg, name, camera, w, h, X.INLINE, limit, spp, start), start, name, camera, w, h, X.INLINE, limit, spp, "auto")


def test_two_calls_are_one_call_of_two_samples(ctx, pkg):
    w, h = 64, 48
    start = R.start_planes(w, h)
    got = device_planes(ctx, pkg, "main", "turned60", w, h, X.INLINE, 2, 2, start, calls=2)
    held(got, start, "main", "turned60", w, h, X.INLINE, 2, 2, "two calls")


@pytest.mark.parametrize("mode, camera, w, h", [(X.STREAMS_FROM_RESULT, "turned90", 64, 48), (X.STREAMS_KEEP, "initial", 37, 23)])
def test_the_streams_chain_with_both_seed_rules(ctx, pkg, mode, camera, w, h):
    start = R.start_planes(w, h)
    held(device_planes(ctx, pkg, "dim", camera, w, h, mode, 64, 2, start), start, "dim", camera, w, h, mode, 64, 2, "Streams chain")


@pytest.mark.parametrize("name, mode, limit, spp", [("main", X.STREAMS_FROM_RESULT, 64, 1), ("glass", X.TREE, TREE_CAP, 1)])
def test_the_stream_form_with_and_without_glass(pkg, name, mode, limit, spp):
    """PTMI_FORM_STREAM adds a pixel's terms in no defined order: the reference's bound carries the unordered-sum term for its term count"""
    B = pkg.binding
    camera, w, h = ("turned60", 64, 48) if name == "main" else ("initial", 64, 48)
    start = R.start_planes(w, h)
    with pkg.Context(0) as c:
        c.set_option(B.OPT_STREAMS_FORM, B.FORM_STREAM)
        got = device_planes(c, pkg, name, camera, w, h, mode, limit, spp, start)
        assert c.stats()["stream_rays_dropped"] == 0
    held(got, start, name, camera, w, h, mode, limit, spp, "stream form")


@pytest.mark.parametrize("name, camera, w, h", [("glass", "turned90", 37, 23), ("glass_low", "initial", 64, 48)])
def test_the_tree_walk_under_the_step_cap(ctx, pkg, name, camera, w, h):
    start = R.start_planes(w, h)
    held(device_planes(ctx, pkg, name, camera, w, h, X.TREE, TREE_CAP, 1, start), start, name, camera, w, h, X.TREE, TREE_CAP, 1, "tree walk")


@pytest.mark.parametrize("mode, limit, spp, camera", [(X.INLINE, 4, 2, "turned60"), (X.STREAMS_FROM_RESULT, 64, 1, "turned60")])
def test_the_same_scene_through_the_sphere_hierarchy(ctx, pkg, mode, limit, spp, camera):
    name = "scene16" if mode == X.INLINE else "main"
    w, h = 64, 48
    start = R.start_planes(w, h)
    held(device_planes(ctx, pkg, name, camera, w, h, mode, limit, spp, start, how="bvh"), start, name, camera, w, h, mode, limit, spp, "set_scene_bvh")


@pytest.mark.parametrize("name, camera, w, h, mode, limit, spp", [("mesh", "initial", 64, 48, X.INLINE, 4, 2), ("mesh", "initial", 37, 23, X.STREAMS_FROM_RESULT, 64, 1),
                                                                  ("mesh_glass", "initial", 64, 48, X.TREE, TREE_CAP, 2)])
def test_the_mesh_room_as_set_and_after_new_triangles(pkg, name, camera, w, h, mode, limit, spp):
    """set_scene_mesh, and set_mesh_triangles (the hierarchy built on the device) over a scene set with other triangles"""
    start = R.start_planes(w, h)
    s, p, t = R.scene(name)
    with pkg.Context(0) as c:
        got = device_planes(c, pkg, name, camera, w, h, mode, limit, spp, start)
        held(got, start, name, camera, w, h, mode, limit, spp, "set_scene_mesh")
        c.set_scene_mesh(s, t[:13], p)
        c.set_mesh_triangles(t)
        got = device_planes(c, pkg, name, camera, w, h, mode, limit, spp, start, how=None)
        held(got, start, name, camera, w, h, mode, limit, spp, "set_mesh_triangles")


def test_a_chained_closure_call(ctx, pkg):
    name, camera, w, h, limit = "main", "turned60", 64, 48, 2
    start = R.start_planes(w, h)
    set_scene(ctx, name)
    cam = R.CAMERAS[camera]()
    names = ("r", "g", "b", "sa", "sb", "sc", "sctr")
    tok, _ = ctx.render1_chained(cam, limit, w, h, 0, planes_in=start)
    tok2, fetched = ctx.render1_chained(cam, limit, w, h, tok, consume=True, fetch=names)
    ctx.chain_release(tok2)
    held([fetched[k] for k in names], start, name, camera, w, h, X.INLINE, limit, 2, "two chained closure calls")


def test_a_three_part_partition_stitched(pkg):
    name, camera, w, h, limit, spp = "main", "turned60", 64, 48, 4, 2
    start = R.start_planes(w, h)
    stitched = [np.zeros_like(p) for p in start]
    for part in range(3):
        with pkg.Context(0) as c:
            set_scene(c, name)
            c.set_partition(4, 3, part)
            c.resize(w, h)
            rows = c.global_rows()
            c.upload_state(*[p[rows] for p in start])
            c.render(R.CAMERAS[camera](), limit, spp, pkg.INLINE)
            for dst, src in zip(stitched, c.download_state()):
                dst[rows] = src
    held(stitched, start, name, camera, w, h, X.INLINE, limit, spp, "3 parts")


@pytest.mark.parametrize("case", [INLINE_2_SAMPLES, INLINE_1_SAMPLE])
def test_contracted_arithmetic_is_within_the_same_bound(pkg, case):
    """PTMI_ARITH_CONTRACTED: a fused a * b + c rounds once where the bound counts two roundings, so the bound holds as it stands"""
    B = pkg.binding
    name, camera, w, h, limit, spp = case
    start = R.start_planes(w, h)
    with pkg.Context(0) as c:
        c.set_option(B.OPT_ARITHMETIC, B.ARITH_CONTRACTED)
        got = device_planes(c, pkg, name, camera, w, h, X.INLINE, limit, spp, start)
        c.set_option(B.OPT_ARITHMETIC, B.ARITH_EXACT)
        exact = device_planes(c, pkg, name, camera, w, h, X.INLINE, limit, spp, start)
    held(got, start, name, camera, w, h, X.INLINE, limit, spp, "contracted")
    assert any(not np.array_equal(a, b) for a, b in zip(got[:3], exact[:3])), "the contracted kernel ran: its colours are not the exact ones"
