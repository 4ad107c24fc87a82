"""tests/cxx/ray_streams_reference.c -- the contract of ptmi_trace_streams_device in plain C, with its own restatement of glass_children --
held to the oracle's render loops (no GPU): along the primary rays of world.initial_camera() over 64 x 32, from ora_gen_seeds and the
planes' colours, all seven planes match bit for bit and the counters match
  * ora_render_streams_tree (stack 16) on world.glass_scene() at step caps 2, 3, 64 and 65536;
  * ora_render_streams_ex under both seed rules on main_scene and scene16, at caps 3 and 65536."""
import numpy as np
import pytest

import ray_streams_inputs as inputs

W = inputs.W
WIDTH, HEIGHT, SPP = 64, 32, 3
KEEP, FROM_RESULT = 0, 1                                     # ORA_SEED_KEEP_ACCUMULATOR, ORA_SEED_FROM_RESULT


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return inputs.Reference(tmp_path_factory.mktemp("ray_streams"))


@pytest.fixture(scope="module")
def start(ref):
    """(rays, seeds (n, 4), colour (n, 3), the same as seven planes): a start colour that is not zero, so that the adder's order shows"""
    n = WIDTH * HEIGHT
    rays = ref.primaries(W.initial_camera(), WIDTH, HEIGHT)
    seeds = ref.seeds(n)
    color = np.random.default_rng(3).uniform(0.0, 2.0, (n, 3)).astype(np.float32)
    planes = [color[:, k].reshape(HEIGHT, WIDTH).copy() for k in range(3)] + [seeds[:, k].reshape(HEIGHT, WIDTH).copy() for k in range(4)]
    return rays, seeds, color, planes


def same_planes(got_color, got_seeds, planes, what):
    for k, name in enumerate("rgb"):
        assert np.array_equal(got_color[:, k].view(np.uint32), np.asarray(planes[k], np.float32).reshape(-1).view(np.uint32)), "%s: plane %s" % (what, name)
    for k, name in enumerate(("sa", "sb", "sc", "sctr")):
        assert np.array_equal(got_seeds[:, k], np.asarray(planes[3 + k]).reshape(-1).view(np.uint32)), "%s: plane %s" % (what, name)


@pytest.mark.parametrize("cap", [2, 3, 64, 65536])
def test_the_walk_is_the_oracles_tree_walk_on_the_glass_scene(ref, start, cap):
    rays, seeds, color, planes = start
    spheres, planes_of_scene = W.glass_scene()
    want, _, dropped, _, truncated = ref.ora.render_streams_tree(spheres, planes_of_scene, W.initial_camera(), WIDTH, HEIGHT, cap, SPP, planes, stack_depth=16)
    got_color, got_seeds, lost, diag = ref.trace((spheres, None, planes_of_scene), rays, color, seeds, SPP, cap=cap)
    same_planes(got_color, got_seeds, want, "cap %d" % cap)
    assert lost.tolist() == [truncated, dropped]
    assert int(diag["truncated"].sum()) == truncated and int(diag["dropped"].sum()) == dropped
    assert (diag["glass_hits"] > 0).sum() > 100
    assert truncated > 0 if cap <= 3 else cap == 64 or truncated == 0
    assert not np.array_equal(got_color, color)


def test_a_shallow_stack_drops_what_the_oracle_drops(ref, start):
    rays, seeds, color, planes = start
    spheres, planes_of_scene = W.glass_scene()
    want, _, dropped, _, truncated = ref.ora.render_streams_tree(spheres, planes_of_scene, W.initial_camera(), WIDTH, HEIGHT, 65536, 1, planes, stack_depth=1)
    got_color, got_seeds, lost, _ = ref.trace((spheres, None, planes_of_scene), rays, color, seeds, 1, stack_depth=1)
    same_planes(got_color, got_seeds, want, "stack 1")
    assert dropped > 0 and lost.tolist() == [truncated, dropped]


@pytest.mark.parametrize("scene", ["main_scene", "scene16"])
@pytest.mark.parametrize("rule", [KEEP, FROM_RESULT])
@pytest.mark.parametrize("cap", [3, 65536])
def test_without_glass_the_walk_is_the_oracles_chain_under_both_seed_rules(ref, start, scene, rule, cap):
    rays, seeds, color, planes = start
    spheres, planes_of_scene = getattr(W, scene)()
    want, _, truncated = ref.ora.render_streams(spheres, planes_of_scene, W.initial_camera(), WIDTH, HEIGHT, cap, SPP, planes, seed_rule=rule, want_truncated=True)
    got_color, got_seeds, lost, diag = ref.trace((spheres, None, planes_of_scene), rays, color, seeds, SPP, cap=cap, from_result=rule == FROM_RESULT)
    same_planes(got_color, got_seeds, want, "%s, rule %d, cap %d" % (scene, rule, cap))
    assert lost.tolist() == [truncated, 0] and (truncated > 0) == (cap == 3)
    assert (diag["glass_hits"] == 0).all() and (diag["hits"] >= 2 * SPP).sum() > 100


def test_the_seed_rules_differ_and_auto_is_from_result_without_glass(ref, start):
    rays, seeds, color, _ = start
    sc = W.main_scene()
    keep = ref.trace((sc[0], None, sc[1]), rays, color, seeds, 1, from_result=False)
    res = ref.trace((sc[0], None, sc[1]), rays, color, seeds, 1, from_result=True)
    auto = ref.trace((sc[0], None, sc[1]), rays, color, seeds, 1)
    assert np.array_equal(auto[1], res[1]) and (keep[1] != res[1]).any()
    assert np.array_equal(keep[0].view(np.uint32), res[0].view(np.uint32))            # one sample: the same colour
