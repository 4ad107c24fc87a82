"""The step's reference, run alone (no GPU).  Two things are held here, for each of the five scenes of tests/ray_paths_inputs.py with their
4 096 rays:

  * THE RESTATEMENT IS THE ORACLE'S.  tests/cxx/ray_bounce_reference.c writes prepareRay a second time; k of its steps from throughput 1 and
    radiance 0 must give ray_paths_reference(limit k, 1 spp) -- the oracle's own traceInline -- word for word: 0 + radiance and the seeds,
    for k = 1 .. 8.
  * THE BATCHES EXERCISE THE STEP, or the device test would pass on nothing.  With c(k) the number of rays whose k-th prepareRay is a
    computeRay: c(1), c(2), c(3) lie in [n / 4, n - 1]; c(4) >= 1; c(7) == 0, so the live list empties within 8 steps; and both other
    outcomes -- a miss, a frozen throughput -- occur at some step."""
import numpy as np
import pytest

import ray_bounce_inputs as inputs


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return inputs.Reference(tmp_path_factory.mktemp("ray_bounce"))


@pytest.fixture(scope="module")
def stepped(ref):
    """{kind: (scene, rays, the states after 1 .. 8 steps)}, computed once"""
    out = {}
    for kind in inputs.KINDS:
        sc = inputs.scene(kind)
        rays = inputs.batch(kind, sc, ref)
        out[kind] = (sc, rays, ref.steps(sc, rays))
    return out


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("kind", inputs.KINDS)
def test_k_steps_are_the_oracles_trace_inline(ref, stepped, kind):
    sc, rays, states = stepped[kind]
    n = inputs.N_RAYS
    for k in range(1, inputs.STEPS + 1):
        color, seeds, _, _ = ref.trace(sc, rays, np.zeros((n, 3), np.float32), ref.seeds(n), k, 1)
        _, _, radiance, s, _, _ = states[k - 1]
        with np.errstate(all="ignore"):
            got = (np.float32(0.0) + radiance).astype(np.float32)          # new + old, old = 0
        assert np.array_equal(s, seeds), "%s: seeds after %d steps" % (kind, k)
        same = (words(got) == words(color)) | (np.isnan(got) & np.isnan(color))
        assert same.all(), "%s: %d radiance words differ after %d steps" % (kind, (~same).sum(), k)


@pytest.mark.parametrize("kind", inputs.KINDS)
def test_the_batch_exercises_the_step(stepped, kind):
    _, rays, states = stepped[kind]
    n = inputs.N_RAYS
    outcome = np.stack([s[4] for s in states])                            # (step, ray)
    hits = (outcome == inputs.HIT).sum(1)
    print(kind, "computeRay per step:", hits.tolist(), "misses:", (outcome == inputs.MISSED).sum(1).tolist(),
          "frozen:", (outcome == inputs.FROZEN).sum(1).tolist())
    for k in (1, 2, 3):
        assert n // 4 <= hits[k - 1] <= n - 1, (kind, k, hits.tolist())
    assert hits[3] >= 1, hits.tolist()
    assert hits[6] == 0, hits.tolist()
    assert (outcome == inputs.MISSED).any() and (outcome == inputs.FROZEN).any()
    # what each outcome leaves: a hit moves the seed; a miss or a frozen ray keeps ray, radiance and seed and has throughput 0
    before = (rays, np.ones((n, 3), np.float32), np.zeros((n, 3), np.float32), None)
    for k, state in enumerate(states):
        r, t, rad, s, what, rec = state
        if k:
            still = what != inputs.HIT
            assert np.array_equal(words(r[still]), words(before[0][still])) and np.array_equal(words(rad[still]), words(before[2][still]))
            assert np.array_equal(s[still], before[3][still]) and not words(t[still]).any() and not words(rec[still]).any()
            assert (s[~still] != before[3][~still]).any(1).all()
        before = state
    # a ray whose throughput is zero is frozen from then on: the live list only shrinks
    live = [inputs.live_list(s[1])[1] for s in states]
    assert all(a >= b for a, b in zip(live, live[1:])) and live[-1] == 0, live
    assert [int(c) for c in hits[1:]] == [int(((states[k][4] == inputs.HIT)).sum()) for k in range(1, inputs.STEPS)]


def test_the_numpy_near_zero_is_the_oracles(ref):
    """live_list's nearZero against ora_near_zero_v3 on the values the list is tested at: around the threshold, denormal, infinite, NaN"""
    import ctypes as C
    rng = np.random.default_rng(3)
    t = (rng.normal(size=(4096, 3)) * 10.0 ** rng.uniform(-6, 0, (4096, 1))).astype(np.float32)
    t[:8] = [[1e-3, 0, 0], [0, 1e-3, 0], [np.float32(1e-3), np.float32(1e-6), 0], [np.nan, 0, 0], [np.inf, 0, 0], [1e-40, 1e-40, 1e-40], [-0.0, 0.0, -0.0],
             [0, 0, np.float32(0.0010000002)]]
    lib = C.CDLL(ref.ora.LIB)

    class V3(C.Structure):
        _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]
    lib.ora_near_zero_v3.argtypes, lib.ora_near_zero_v3.restype = [V3], C.c_int
    want = np.array([bool(lib.ora_near_zero_v3(V3(*map(float, row)))) for row in t])
    got = inputs.near_zero(t)
    assert np.array_equal(got, want)
    assert want.any() and not want.all() and not want[3] and not want[4] and want[5] and want[6]
