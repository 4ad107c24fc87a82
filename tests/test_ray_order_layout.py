"""The ray order's key and order on the host (no GPU needed): ptmi_ray_order_keys against a numpy float64 restatement of the formula in
csrc/ptmi_ray_order.h's comment, word for word, and ptmi_ray_order against the keys.  These host twins are what the device order is held
to entry for entry (tests/test_gpu_ray_order.py), so together the device is held to the written formula.

The restatement below is written from the comment, not from the code: a ray is placed when its six words are finite and
s = (|dx| + |dy|) + |dz| > 0; lo / hi are the binary32 box of the placed rays' origins; per axis
qo = hi == lo ? 0 : min(255, floor((o - lo) * 256 / (hi - lo))); u = dx / s, v = dy / s, folded over when dz < 0 with sg(x) = x >= 0 ? 1 : -1;
qu = min(1023, floor((u * 0.5 + 0.5) * 1024)); key = morton3(qo) << 20 | morton2(qu, qv); 1 << 44 for a ray that is not placed.  Every
numpy operation on float64 arrays is one IEEE operation rounded on its own, as the library's (it is compiled without contraction)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ray_order_inputs as inputs  # noqa: E402

NOT_PLACED = np.uint64(1 << 44)


def keys_by_formula(rays):
    r = np.ascontiguousarray(rays, np.float32)
    n = len(r)
    o, d = r[:, :3], r[:, 3:].astype(np.float64)
    with np.errstate(all="ignore"):
        s = (np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2])
        placed = np.isfinite(r).all(1) & (s > 0)
        keys = np.full(n, NOT_PLACED, np.uint64)
        if not placed.any():
            return keys
        lo, hi = o[placed].min(0), o[placed].max(0)            # binary32
        q = np.zeros((n, 3), np.int64)
        for a in range(3):
            if hi[a] == lo[a]:
                continue
            num = (o[:, a].astype(np.float64) - np.float64(lo[a])) * 256.0
            cell = np.floor(num / (np.float64(hi[a]) - np.float64(lo[a])))
            q[placed, a] = np.minimum(255, cell[placed]).astype(np.int64)
        u, v = d[:, 0] / s, d[:, 1] / s
        sg = lambda x: np.where(x >= 0, 1.0, -1.0)  # noqa: E731
        below = r[:, 5] < 0
        fu, fv = (1.0 - np.abs(v)) * sg(u), (1.0 - np.abs(u)) * sg(v)
        u, v = np.where(below, fu, u), np.where(below, fv, v)
        qu = np.zeros(n, np.int64)
        qv = np.zeros(n, np.int64)
        qu[placed] = np.minimum(1023, np.floor((u * 0.5 + 0.5) * 1024.0)[placed]).astype(np.int64)
        qv[placed] = np.minimum(1023, np.floor((v * 0.5 + 0.5) * 1024.0)[placed]).astype(np.int64)
    assert (q >= 0).all() and (qu >= 0).all() and (qv >= 0).all()
    m3 = np.zeros(n, np.uint64)
    m2 = np.zeros(n, np.uint64)
    for i in range(8):
        for a, up in ((0, 2), (1, 1), (2, 0)):
            m3 |= (((q[:, a] >> i) & 1).astype(np.uint64)) << np.uint64(3 * i + up)
    for i in range(10):
        m2 |= (((qu >> i) & 1).astype(np.uint64)) << np.uint64(2 * i + 1)
        m2 |= (((qv >> i) & 1).astype(np.uint64)) << np.uint64(2 * i)
    keys[placed] = ((m3 << np.uint64(20)) | m2)[placed]
    return keys


@pytest.fixture(scope="module")
def sets(pkg):
    return inputs.all_sets(pkg)


SET_NAMES = ["adversarial plain", "adversarial s16", "adversarial runs", "adversarial bvh", "adversarial mesh", "camera", "faces", "axes and diagonals",
             "negative zero", "beyond 2^40"]


def test_the_named_sets_are_the_sets(sets):
    assert sorted(sets) == sorted(SET_NAMES)
    for name in SET_NAMES[:5]:
        r = sets[name]
        assert len(r) == 4096 and not np.isfinite(r[-4:-1]).all(1).any() and (r[-1, 3:] == 0).all()


@pytest.mark.parametrize("name", SET_NAMES)
def test_keys_equal_the_written_formula(pkg, sets, name):
    rays = sets[name]
    got, want = pkg.binding.ray_order_keys(rays), keys_by_formula(rays)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d keys differ, e.g. ray %d %r: %#x, the formula gives %#x" % (name, bad.size, bad[0], rays[bad[0]], got[bad[0]], want[bad[0]])
    placed = got != NOT_PLACED
    assert (got[placed] < NOT_PLACED).all() and placed.sum() > len(rays) // 2
    if name.startswith("adversarial"):
        assert not placed[-4:].any() and len(np.unique(got)) > 1000          # the keys do tell the rays apart


def test_what_the_sets_are_there_for(pkg, sets):
    B = pkg.binding
    cam = B.ray_order_keys(sets["camera"])
    assert (cam >> np.uint64(20) == 0).all() and len(np.unique(cam)) > 2000            # one origin: hi == lo, the direction alone orders
    faces = sets["faces"]
    k = B.ray_order_keys(faces) >> np.uint64(20)
    top = (faces[:, :3] == faces[:, :3].max(0))
    for a, up in ((0, 2), (1, 1), (2, 0)):
        cell = sum((((k >> np.uint64(3 * i + up)) & np.uint64(1)) << np.uint64(i)) for i in range(8))
        assert top[:, a].sum() > 50 and (cell[top[:, a]] == 255).all() and cell.max() == 255 and cell.min() == 0
    # the octahedral map's landmarks: +z the centre, -z the corners, +-x and +-y the edge midpoints, whatever the length
    r = np.zeros((6, 6), np.float32)
    r[:, :3] = [[0, 0, 0], [1, 1, 1], [0, 1, 0], [1, 0, 0], [0, 0, 1], [1, 1, 0]]
    r[np.arange(6), [5, 5, 3, 3, 4, 4]] = [2.0, -0.5, 3.0, -3.0, 1e-20, -1e20]
    low20 = B.ray_order_keys(r) & np.uint64((1 << 20) - 1)

    def cells(key):
        key = int(key)
        return (sum(((key >> (2 * i + 1)) & 1) << i for i in range(10)), sum(((key >> (2 * i)) & 1) << i for i in range(10)))
    assert [cells(x) for x in low20] == [(512, 512), (1023, 1023), (1023, 512), (0, 512), (512, 1023), (512, 0)]
    nz = sets["negative zero"]
    kz = B.ray_order_keys(nz)
    flipped = nz.copy()
    flipped[0::4, 5] = 0.0
    assert np.array_equal(B.ray_order_keys(flipped)[0::4], kz[0::4])                  # dz = -0.0 is not below: the key of dz = +0.0
    assert (np.abs(sets["beyond 2^40"][:, :3]).max(1) > 2.0 ** 40).sum() > 300


def test_a_set_with_no_placed_ray(pkg):
    rays = inputs.unplaced_rays()
    assert pkg.binding.RAY_KEY_NOT_PLACED == NOT_PLACED
    assert (pkg.binding.ray_order_keys(rays) == NOT_PLACED).all() and (keys_by_formula(rays) == NOT_PLACED).all()
    assert np.array_equal(pkg.binding.ray_order(rays), np.arange(len(rays)))
    assert pkg.binding.ray_order_keys(np.zeros((0, 6), np.float32)).shape == (0,) and pkg.binding.ray_order(np.zeros((0, 6), np.float32)).shape == (0,)


@pytest.mark.parametrize("name", SET_NAMES)
def test_the_order_is_a_permutation_ascending_by_key_then_index(pkg, sets, name):
    for n in (len(sets[name]), 4097, 12293):
        rays = inputs.tiled(sets[name], n)
        keys, order = pkg.binding.ray_order_keys(rays), pkg.binding.ray_order(rays)
        assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(n)), name
        assert np.array_equal(order, np.lexsort((np.arange(n), keys))), name
        if name.startswith("adversarial") and n == len(sets[name]):
            assert np.array_equal(order[-4:], np.arange(n - 4, n))                   # what is not placed: behind, in index order


def test_identical_rays_give_the_identity(pkg):
    rays = inputs.identical_rays(4097)
    assert len(np.unique(pkg.binding.ray_order_keys(rays))) == 1
    assert np.array_equal(pkg.binding.ray_order(rays), np.arange(4097))


def test_the_host_twins_refuse_what_the_header_says(pkg):
    lib, B = pkg.load_library(), pkg.binding
    assert lib.ptmi_ray_order(None, -1, None) == B.PTMI_EINVAL and lib.ptmi_ray_order_keys(None, -1, None) == B.PTMI_EINVAL
    assert lib.ptmi_ray_order(None, 3, None) == B.PTMI_EINVAL and lib.ptmi_ray_order_keys(None, 3, None) == B.PTMI_EINVAL
    assert lib.ptmi_ray_order(None, 0, None) == B.PTMI_OK and lib.ptmi_ray_order_keys(None, 0, None) == B.PTMI_OK
    one = np.zeros(6, np.float32)
    out = np.zeros(2, np.uint64)
    p = lambda a: a.ctypes.data  # noqa: E731
    assert lib.ptmi_ray_order(p(one), B.RAY_ORDER_MAX + 1, p(out)) == B.PTMI_ELIMIT
    assert lib.ptmi_ray_order_keys(p(one), B.RAY_ORDER_MAX + 1, p(out)) == B.PTMI_ELIMIT and not out.any()


def test_the_workspace_size(pkg):
    """ptmi_ray_order_bytes: 0 for n <= 0; the sort's scratch (two key and two index arrays, 256 counts per tile of 4 096) and six box
    words, a multiple of 8"""
    B = pkg.binding
    assert B.ray_order_bytes(0) == 0 and B.ray_order_bytes(-7) == 0
    for n in (1, 63, 4096, 4097, 12293, 1 << 22):
        tiles = (n + 4095) // 4096
        assert B.ray_order_bytes(n) == 24 * n + 1024 * tiles + 24 and B.ray_order_bytes(n) % 8 == 0
