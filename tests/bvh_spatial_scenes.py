"""What the tests of the spatial sphere build share (tests/test_bvh_spatial_layout.py on the CPU, test_gpu_bvh_spatial.py on the device):
a numpy restatement of include/ptmi.h's text for ptmi_bvh_layout_spatial -- written from that text, level by level -- the scene families
and the cost of a node array."""
import numpy as np

import bvh_update_scenes as scenes

binding = scenes.binding
LEAF_MAX, MAX_DEPTH = binding.BVH_LEAF_MAX, binding.BVH_MAX_DEPTH


def spatial_keys(s):
    """the 42-bit key of every centre in cubic cells, float64, each operation rounded on its own"""
    c = s["position"].astype(np.float32)
    if not len(c):
        return np.zeros(0, np.uint64)
    lo, hi = c.min(0).astype(np.float64), c.max(0).astype(np.float64)
    den = float((hi - lo).max())
    c = c.astype(np.float64)
    key = np.zeros(len(s), np.uint64)
    for a in range(3):
        if den == 0.0:
            q = np.zeros(len(s), np.int64)
        else:
            q = np.minimum(16383, np.floor(((c[:, a] - lo[a]) * 16384.0) / den).astype(np.int64))
        for i in range(14):
            key |= ((q >> i) & 1).astype(np.uint64) << np.uint64(3 * i + (2 - a))
    return key


def equal_count_levels(k):
    """the inner levels of equal-count splits over k items (an array): 0 up to LEAF_MAX"""
    k = np.array(k, np.int64, copy=True)
    levels = np.zeros_like(k)
    while True:
        big = k > LEAF_MAX
        if not big.any():
            return levels
        k[big] -= k[big] // 2
        levels[big] += 1


def leaf_ref(b, e):
    return np.where(e == b, -1, -1 - ((b << 8) | (e - b)))


def restate(s, guard=True):
    """-> (ref [n_nodes, 2] int32, order int32, level_first: the id of every level's first node and the node count behind, fallbacks: how
    many nodes split at their middle).  guard=False leaves the depth limit out (the recursion the guard exists for)."""
    n = len(s)
    key = spatial_keys(s)
    order = np.lexsort((np.arange(n), key)).astype(np.int32)
    sk = key[order].astype(np.int64)                                  # (42 bits)
    b, e = np.zeros(1, np.int64), np.full(1, n, np.int64)
    refs, level_first, fallbacks, level = [], [0], 0, 0
    while len(b):
        if n <= LEAF_MAX:                                             # the root of a small scene: everything in child 0
            m = e.copy()
        else:
            differ = sk[b] ^ sk[e - 1]
            h = np.frexp(np.maximum(differ, 1).astype(np.float64))[1].astype(np.int64) - 1      # the highest set bit (exact: 42 bits)
            m_bit = np.searchsorted(sk, ((sk[b] >> h) | 1) << h, "left")      # the first key with bit h set: the bits above agree in [b, e)
            take = differ != 0
            if guard:
                take &= level + 1 + equal_count_levels(np.maximum(m_bit - b, e - m_bit)) <= MAX_DEPTH
            m = np.where(take, m_bit, b + (e - b) // 2)
            fallbacks += int((~take).sum())
            assert np.all((b < m) & (m < e))
        cb = np.stack([b, m], 1).reshape(-1)                          # the children in id order: child 0, child 1 of each node in turn
        ce = np.stack([m, e], 1).reshape(-1)
        inner = ce - cb > LEAF_MAX
        next_first = level_first[-1] + len(b)
        ids = next_first + np.cumsum(inner) - 1
        refs.append(np.where(inner, ids, leaf_ref(cb, ce)).reshape(-1, 2))
        level_first.append(next_first)
        b, e = cb[inner], ce[inner]
        level += 1
    return np.concatenate(refs).astype(np.int32), order, level_first, fallbacks


def chain(duplicates=4, cluster=100):
    """A scene on which every spatial split peels one cell off: centres on a geometric series (1, 1/2, 1/4 ... down to the key's
    resolution, 2^-14 of the box) that hugs the diagonal -- per octave three centres, whose x, whose x and y, whose x, y and z have dropped
    to the next octave, so that the three bits of an octave split one after another (ON the diagonal the three bits of an octave agree and
    the series has only 14 splits to give) -- `duplicates` spheres on each, and a cluster of `cluster` spheres in the cell at the small end.
    About 270 spheres; the unguarded recursion is 14 x 3 levels deep before it reaches the cluster."""
    centres = []
    for i in range(14):
        hi_, lo_ = 2.0 ** -i, 2.0 ** -(i + 1)
        centres += [(hi_, hi_, hi_), (lo_, hi_, hi_), (lo_, lo_, hi_)]
    c = np.repeat(np.array(centres, np.float32), duplicates, axis=0)
    rng = np.random.default_rng(5)
    small = (rng.random((cluster, 3)) * 2.0 ** -16).astype(np.float32)
    small[0] = 0.0                                                    # (the box starts at the origin: the cells are 2^-14 wide)
    c = np.concatenate([c, small])
    s, p = scenes.field(len(c), seed=31)
    s["position"] = c
    s["radius"] = (np.maximum(np.abs(c).max(1), 2.0 ** -16) * 0.25).astype(np.float32)
    return s, p


def all_equal(n=300):
    s, p = scenes.field(n, seed=32)
    s["position"] = s["position"][7]
    return s, p


def flat_two(n=300):
    """hi == lo on two axes"""
    s, p = scenes.field(n, seed=33)
    s["position"][:, 0] = np.float32(1.5)
    s["position"][:, 2] = np.float32(-2.25)
    return s, p


def families():
    """name -> (spheres, planes)"""
    return {
        "field": scenes.field(600, seed=30),
        "all_equal": all_equal(),
        "flat_y": scenes.flat(600, 1, seed=34),
        "flat_xz": flat_two(),
        "coincident": scenes.coincident(600, seed=35),
        "chain": chain(),
        "adversarial": scenes.families()["adversarial"],
    }


def levels_of(nodes):
    """the level of every node (children have larger ids than their parent)"""
    ref = nodes["ref"]
    level = np.zeros(len(nodes), np.int64)
    for i in range(len(nodes)):
        for r in ref[i]:
            if r >= 0:
                level[r] = level[i] + 1
    return level


def cost(nodes):
    """the surface-area cost of a node array: the sum over non-empty child boxes of area x w -- w = 2 for an inner child, the sphere count
    for a leaf -- over the area of the union of the root's two boxes"""
    half, center, ref = nodes["half"].astype(np.float64), nodes["center"].astype(np.float64), nodes["ref"].astype(np.int64)
    d = 2.0 * half
    area = 2.0 * (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])
    w = np.where(ref >= 0, 2, (-1 - ref) & 255)
    full = ref != -1
    keep = full[0]
    lo, hi = (center[0] - half[0])[keep].min(0), (center[0] + half[0])[keep].max(0)
    r = hi - lo
    root = 2.0 * (r[0] * r[1] + r[1] * r[2] + r[2] * r[0])
    return float((area * w)[full].sum() / root)
