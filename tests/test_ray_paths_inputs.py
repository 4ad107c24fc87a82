"""The batches tests/ray_paths_driver.py sends to ptmi_trace_paths_device, run through the reference alone (no GPU): they must exercise the
loop, or the device test would pass on nothing.  For each of the five scenes of tests/ray_paths_inputs.py, at limit 8 and 2 spp from a
zero colour:
  * at least a quarter of the rays have a sample of 2 or more live bounces (the loop's trace and second shade run);
  * at least a tenth end with a non-zero colour (light is carried back);
  * at least one ray misses outright (no live bounce in any sample: the seed stays, the colour is 0 + colour);
  * at least one path reaches the bounce limit (the certain-freeze exit at the limit) -- at limit 3, which the device test runs too: in
    these scenes a bounce scales the throughput by at most |colour| max(brdf) / (2 pi) < 0.16, so nearZero (|throughput|^2 < 1e-6) freezes
    every path before its eighth bounce, and at limit 8 the other exit is the one that runs (both are counted below);
and the batches hold the off-length family; the camera half and the adversarial rest both have paths of two bounces."""
import numpy as np
import pytest

import ray_paths_inputs as inputs

LIMIT, SHORT_LIMIT, SPP = 8, 3, 2


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return inputs.Reference(tmp_path_factory.mktemp("ray_paths"))


@pytest.mark.parametrize("kind", inputs.KINDS)
def test_the_batch_exercises_the_loop(ref, kind):
    sc = inputs.scene(kind)
    rays = inputs.batch(kind, sc, ref)
    seeds = ref.seeds(inputs.N_RAYS)
    color, seeds_out, lo, hi = ref.trace(sc, rays, np.zeros((inputs.N_RAYS, 3), np.float32), seeds, LIMIT, SPP)
    n = inputs.N_RAYS
    hi3 = ref.trace(sc, rays, np.zeros((inputs.N_RAYS, 3), np.float32), seeds, SHORT_LIMIT, SPP)[3]
    counts = {"two bounces": int((hi >= 2).sum()), "non-zero colour": int((np.nan_to_num(color, nan=1.0) != 0).any(1).sum()),
              "misses": int((hi == 0).sum()), "at limit 3": int((hi3 == SHORT_LIMIT).sum()), "frozen before limit 8": int(((hi > 0) & (hi < LIMIT)).sum())}
    print(kind, counts)
    assert counts["two bounces"] >= n // 4, counts
    assert counts["non-zero colour"] >= (n + 9) // 10, counts
    assert counts["misses"] >= 1 and counts["at limit 3"] >= 1 and counts["frozen before limit 8"] >= 1, counts
    missed = hi == 0
    assert np.array_equal(seeds_out[missed], seeds[missed]) and not seeds_out[~missed].tobytes() == seeds[~missed].tobytes()
    assert (color[missed] == 0).all()
    # the camera half and the adversarial half both contribute paths; the latter holds off-length and non-finite rays
    half = inputs.CAMERA_IMAGE[0] * inputs.CAMERA_IMAGE[1] + inputs.N_PROBES
    assert (hi[:half] >= 2).sum() > 0 and (hi[half:] >= 2).sum() > 0
    d2 = (rays[half:, 3:].astype(np.float64) ** 2).sum(1)
    assert (np.abs(d2 - 1.0) > 2.0 ** -12).sum() >= 20


def test_the_scenes_are_the_kinds_the_kernels_serve():
    """mainScene has no shared-xy run and the bench scene has one (which staged kernel the launcher takes); `big` is the first sphere field
    past the LDS budget"""
    def shares(s):
        xy = np.ascontiguousarray(s["position"][:, :2]).view(np.uint32)
        return any(np.array_equal(xy[i], xy[i - 1]) for i in range(1, len(xy)))
    main, s16, big = (inputs.scene(k) for k in ("main", "s16", "big"))
    assert not shares(main[0]) and shares(s16[0])
    assert inputs.packed_bytes(main[0], main[2]) <= inputs.MAX_SCENE_LDS and inputs.packed_bytes(s16[0], s16[2]) <= inputs.MAX_SCENE_LDS
    assert inputs.packed_bytes(big[0], big[2]) > inputs.MAX_SCENE_LDS >= inputs.packed_bytes(big[0][:-1], big[2])
    assert len(inputs.scene("bvh")[0]) > 3000 and len(inputs.scene("mesh")[1]) > 1000
