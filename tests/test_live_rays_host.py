"""ptmi_live_rays, the host twin of ptmi_live_rays_device (no GPU, no context), against a numpy statement of its definition
(tests/ray_bounce_inputs.py: live_list): the candidates -- the index's entries, or 0 .. n - 1 -- that lie in [0, n) and whose throughput is
not nearZero, in candidate order, then -1 up to the candidate count; `count` their number.  Candidate counts 0, 1, 63, 64, 65, 257 and
65 537; an index with out-of-range, -1 and repeated entries; NaN, infinite, denormal and exactly-at-threshold throughputs; the list
written over its own index; every refusal."""
import ctypes as C

import numpy as np
import pytest

import ray_bounce_inputs as inputs

COUNTS = (0, 1, 63, 64, 65, 257, 65537)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
# nearZero is |x x + y y + z z| <= 1e-6 in binary32: the largest float32 whose square rounds to at most float32(1e-6), and the next one
_R = np.float32(1e-3)
while np.float32(_R * _R) <= np.float32(1e-6):
    _R = np.nextafter(_R, np.float32(1))
AT_THRESHOLD, PAST_THRESHOLD = np.nextafter(_R, np.float32(0)), _R


def throughputs(n, seed=1):
    """n throughputs: about half nearZero, with the special values in the first rows (when there is room)"""
    rng = np.random.default_rng(seed)
    t = (rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-5, 0, (n, 1))).astype(np.float32)
    special = np.array([[np.nan, 0, 0], [0, np.inf, 0], [-np.inf, 0, 0], [1e-40, 1e-40, 1e-40], [0, 0, 0], [-0.0, -0.0, -0.0], [AT_THRESHOLD, 0, 0],
                        [0, PAST_THRESHOLD, 0], [0, 0, -AT_THRESHOLD], [1e-39, 0, 1], [np.nan, np.nan, np.nan], [3e38, 3e38, 0]], np.float32)
    k = min(n, len(special))
    t[n - k:] = special[:k]
    return t


def test_the_special_values_are_classified_as_the_definition_says():
    t = throughputs(12)
    assert np.float32(AT_THRESHOLD * AT_THRESHOLD) <= np.float32(1e-6) < np.float32(PAST_THRESHOLD * PAST_THRESHOLD)
    # NaN and infinity are not nearZero (a NaN compares false), denormals and the threshold itself are
    assert inputs.near_zero(t).tolist() == [False, False, False, True, True, True, True, False, True, False, False, False]


@pytest.mark.parametrize("n", COUNTS)
def test_every_ray_a_candidate(pkg, n):
    t = throughputs(n)
    live, count = pkg.binding.live_rays(t)
    want, want_count = inputs.live_list(t)
    assert live.shape == (n,) and count == want_count and np.array_equal(live, want)
    if n >= 63:
        assert 0 < count < n
    # all live and none live
    for fill, expect in ((1.0, n), (0.0, 0)):
        live, count = pkg.binding.live_rays(np.full((n, 3), fill, np.float32))
        assert count == expect and np.array_equal(live, inputs.live_list(np.full((n, 3), fill, np.float32))[0])


@pytest.mark.parametrize("m", COUNTS)
def test_through_an_index_with_foreign_and_repeated_entries(pkg, m):
    n = 300
    t = throughputs(n, seed=2)
    rng = np.random.default_rng(m)
    index = rng.integers(0, n, m).astype(np.int32)                       # repeated entries among them once m > n
    if m >= 63:
        index[[0, 5, 17, 40, 62]] = [-1, n, INT32_MIN, INT32_MAX, index[1]]
    live, count = pkg.binding.live_rays(t, index)
    want, want_count = inputs.live_list(t, index)
    assert count == want_count and np.array_equal(live, want)
    if m >= 63:
        assert 0 < count < m and (live[:count] >= 0).all() and (live[:count] < n).all() and (live[count:] == -1).all()
    # in place: the list written over the index it was made from
    own = index.copy()
    out, count2 = pkg.binding.live_rays(t, own, out=own)
    assert out is own and count2 == want_count and np.array_equal(own, want)
    # an index into no rays at all: every entry is outside [0, 0)
    live, count = pkg.binding.live_rays(np.zeros((0, 3), np.float32), index)
    assert count == 0 and (live == -1).all()


def test_a_padded_list_is_a_fixed_point_and_the_order_is_kept(pkg):
    """the list of a list is the list (the -1 padding is skipped); a permutation's order survives"""
    n = 1000
    t = throughputs(n, seed=4)
    order = np.random.default_rng(9).permutation(n).astype(np.int32)
    live, count = pkg.binding.live_rays(t, order)
    assert np.array_equal(live[:count], order[~inputs.near_zero(t)[order]])
    again, count2 = pkg.binding.live_rays(t, live)
    assert count2 == count and np.array_equal(again, live)


def test_refusals(pkg):
    B = pkg.binding
    lib = B.load_library()
    n = 65
    t = throughputs(n)
    index = np.arange(n, dtype=np.int32)
    live = np.full(n, 77, np.int32)
    count = C.c_int32(77)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    f = lib.ptmi_live_rays
    for rc in (f(p(t), -1, None, 0, p(live), C.byref(count)), f(p(t), n, p(index), -1, p(live), C.byref(count)), f(p(t), n, None, -1, p(live), C.byref(count)),
               f(None, n, None, 0, p(live), C.byref(count)), f(None, n, p(index), n, p(live), C.byref(count)), f(p(t), n, None, 0, None, C.byref(count)),
               f(p(t), n, p(index), n, None, C.byref(count))):
        assert rc == B.PTMI_EINVAL, rc
    big = np.zeros(B.LIVE_RAYS_MAX + 1, np.int32)
    out = np.full(B.LIVE_RAYS_MAX + 1, 77, np.int32)
    assert f(p(t), n, p(big), B.LIVE_RAYS_MAX + 1, p(out), C.byref(count)) == B.PTMI_ELIMIT
    assert f(p(np.zeros((1, 3), np.float32)), B.LIVE_RAYS_MAX + 1, None, 0, p(out), C.byref(count)) == B.PTMI_ELIMIT
    assert (live == 77).all() and (out == 77).all() and count.value == 77, "a refused call wrote"
    # zero candidates: PTMI_OK, nothing touched; a NULL count is allowed
    assert f(None, 0, None, 0, None, None) == B.PTMI_OK and f(p(t), n, p(index), 0, p(live), C.byref(count)) == B.PTMI_OK
    assert (live == 77).all() and count.value == 77
    assert f(p(t), n, None, 0, p(live), None) == B.PTMI_OK and np.array_equal(live, inputs.live_list(t)[0])
    assert f(p(big), 0, p(big), B.LIVE_RAYS_MAX, p(out), C.byref(count)) == B.PTMI_OK and count.value == 0 and (out[:-1] == -1).all() and out[-1] == 77
    # the workspace: 0 for no candidates, 8-byte granular, and at least the candidates themselves
    assert B.live_rays_bytes(0) == 0 and B.live_rays_bytes(-5) == 0
    for c in (1, 64, 65, 257, 65537, B.LIVE_RAYS_MAX):
        assert B.live_rays_bytes(c) % 8 == 0 and 4 * c < B.live_rays_bytes(c) <= 4 * c + c // 32 + 64, c


def test_the_wrapper_refuses_arrays_of_the_wrong_kind(pkg):
    B = pkg.binding
    t = throughputs(10)
    for bad in (t.astype(np.float64), t.reshape(-1), t[:, :2], t[::2]):
        with pytest.raises(ValueError):
            B.live_rays(bad)
    for bad in (np.arange(4, dtype=np.int64), np.zeros((2, 2), np.int32), np.arange(8, dtype=np.int32)[::2]):
        with pytest.raises(ValueError):
            B.live_rays(t, bad)
    with pytest.raises(ValueError):
        B.live_rays(t, out=np.zeros(9, np.int32))
