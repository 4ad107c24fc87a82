"""The batches tests/ray_streams_driver.py sends to ptmi_trace_streams_device, run through the reference alone (no GPU): they must reach what
they are for, or the device test would pass on nothing.  From the reference's per-ray diagnostics, at one sample from a zero colour, at
least 16 rays of every GLASS scene of tests/ray_streams_inputs.py
  * have a glass first hit with 2, with 1 and with 0 of its children hitting (the start record's three shapes);
  * have a glass hit below the first;
  * hold more than kTreeFastLevels = 4 children at once (the scratch levels of the stack);
  * are cut at a step cap of 3 and of 12;
  * have a direction whose length is not 1 and hit glass;
on the drop scene children are dropped; and without GLASS, under PTMI_SEED_FROM_RESULT, there are rays with no hit and rays with two or more,
and the seed a hit leaves differs from the one the other rule keeps."""
import numpy as np
import pytest

import ray_streams_inputs as inputs

AT_LEAST = 16


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return inputs.Reference(tmp_path_factory.mktemp("ray_streams"))


def walk(ref, kind, **kw):
    sc = inputs.scene(kind)
    rays = inputs.batch(kind, sc, ref)
    n = len(rays)
    return rays, ref.seeds(n), ref.trace(sc, rays, np.zeros((n, 3), np.float32), ref.seeds(n), 1, **kw)


@pytest.mark.parametrize("kind", inputs.GLASS)
def test_a_glass_batch_reaches_every_shape_of_the_walk(ref, kind):
    rays, _, (color, _, lost, d) = walk(ref, kind)
    first = d["first_glass"] == 1
    off_length = np.abs((rays[:, 3:].astype(np.float64) ** 2).sum(1) - 1.0) > 2.0 ** -12
    counts = {"first hit glass, 2 children hit": int((first & (d["first_children"] == 2)).sum()),
              "first hit glass, 1 child hits": int((first & (d["first_children"] == 1)).sum()),
              "first hit glass, no child hits": int((first & (d["first_children"] == 0)).sum()),
              "glass below the first hit": int((d["glass_below"] > 0).sum()),
              "a stack past the fast levels": int((d["deepest"] > inputs.FAST_LEVELS).sum()),
              "off-length and glass": int((off_length & (d["glass_hits"] > 0)).sum()),
              "first hit not glass": int(((d["hits"] > 0) & ~first).sum())}
    for cap in (3, 12):
        dc = walk(ref, kind, cap=cap)[2]
        counts["cut at cap %d" % cap] = int((dc[3]["truncated"] > 0).sum())
        assert dc[2][0] == dc[3]["truncated"].sum() > 0
    print(kind, counts)
    for what, count in counts.items():
        assert count >= AT_LEAST, (kind, what, counts)
    assert len(rays) == inputs.N_RAYS and (np.nan_to_num(color, nan=1.0) != 0).any(1).sum() >= len(rays) // 10
    assert lost[0] == 0 and lost[1] == d["dropped"].sum()


def test_the_drop_scene_drops(ref):
    rays, _, (color, _, lost, d) = walk(ref, "drop")
    assert len(rays) == inputs.N_DROP_RAYS
    assert (d["dropped"] > 0).sum() >= AT_LEAST and lost[1] == d["dropped"].sum() > 0 and lost[0] == 0
    assert d["deepest"].max() == inputs.STACK_DEPTH
    assert ((d["first_glass"] == 1) & (d["dropped"] > 0)).sum() >= AT_LEAST          # through the start record, with its slot less
    assert (d["dropped"] == 0).sum() >= AT_LEAST                                      # ... and rays that lose nothing
    assert (color != 0).any(1).all()
    shallow = walk(ref, "drop", stack_depth=4)[2]
    # (the children dropped here are dead -- total reflection leaves them no throughput -- so the colour cannot show a drop: d_lost does)
    assert shallow[2][1] > lost[1] and np.array_equal(shallow[0].view(np.uint32), color.view(np.uint32))


@pytest.mark.parametrize("kind", inputs.PLAIN)
def test_without_glass_the_seed_rule_shows(ref, kind):
    rays, seeds, (color, seeds_out, lost, d) = walk(ref, kind)                        # PTMI_SEED_AUTO: FROM_RESULT
    keep = walk(ref, kind, from_result=False)[2]
    assert (d["glass_hits"] == 0).all() and lost.tolist() == [0, 0]
    assert (d["hits"] == 0).sum() >= 1 and (d["hits"] >= 2).sum() >= len(rays) // 4
    one_hit = d["hits"] <= 1                                                          # the first hit's ray carried the ray's own seed
    assert np.array_equal(seeds_out[one_hit], keep[1][one_hit]) and (seeds_out[~one_hit] != keep[1][~one_hit]).any(1).sum() >= len(rays) // 4
    assert np.array_equal(color.view(np.uint32)[~np.isnan(color)], keep[0].view(np.uint32)[~np.isnan(color)])
    cut = walk(ref, kind, cap=3)[2]
    assert cut[2][0] == cut[3]["truncated"].sum() > 0 and cut[2][1] == 0


def test_the_scenes_are_the_kinds_the_kernels_serve():
    paths = inputs.paths
    for kind in ("main", "glass"):
        s, _, p = inputs.scene(kind)
        assert paths.packed_bytes(s, p) <= paths.MAX_SCENE_LDS
    for kind in ("big", "big_glass"):
        s, _, p = inputs.scene(kind)
        assert paths.packed_bytes(s, p) > paths.MAX_SCENE_LDS
    for kind in inputs.PLAIN:
        s, t, p = inputs.scene(kind)
        assert not (s["brdf_tag"] == inputs.W.GLASS).any() and not (p["brdf_tag"] == inputs.W.GLASS).any()
        assert t is None or not (t["brdf_tag"] == inputs.W.GLASS).any()
    s, t, p = inputs.scene("mesh_glass")
    assert (t["brdf_tag"] == inputs.W.GLASS).sum() >= len(t) // 5 and (s["brdf_tag"] == inputs.W.GLASS).sum() == 2
    s, _, p = inputs.scene("bvh_glass")
    assert (s["brdf_tag"] == inputs.W.GLASS).sum() >= 1000 and len(s) > 3000
