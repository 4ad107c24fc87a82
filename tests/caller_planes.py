"""Helpers of the caller-owned-planes tests (tests/test_caller_planes_layout.py, tests/test_gpu_caller_planes.py and its child program
tests/caller_planes_driver.py): where seven planes lie inside one buffer of a caller -- each at an alignment of its own, in any order, a
guard band on both sides -- and what ptmi_present computes, restated in numpy.  No torch at module level: the CPU half imports this."""
import numpy as np

GUARD_WORD = 0xA5A5A5A5
ALIGNED = (0, 0, 0, 0, 0, 0, 0)
ODD = (1, 2, 3, 0, 1, 2, 3)                 # elements past a 16-byte boundary: r g b sa sb sc sctr (sa stays aligned)
ORDER = (6, 2, 4, 0, 5, 1, 3)               # the order in memory: sctr first, r in the middle of nowhere, sa last
SEPARATE_ORDER = (3, 6, 0, 5, 2, 4, 1)      # SEPARATE: seven allocations of their own, made in this order
SEPARATE_MISALIGN = (2, 0, 3, 1, 0, 3, 1)
NAMES = "r g b sa sb sc sctr".split()


class Layout:
    """n elements per plane; plane k begins `rel[k]` elements behind the first 16-byte boundary at or after the buffer's base address;
    every element of the buffer's `total` that belongs to no plane is a guard."""

    def __init__(self, n, guard, rel, total):
        self.n, self.guard, self.rel, self.total = int(n), int(guard), tuple(int(v) for v in rel), int(total)

    def offsets(self, base_address):
        """element offset of every plane from the buffer's first element, for a buffer at this (4-byte aligned) address"""
        if base_address % 4:
            raise ValueError("the buffer must be 4-byte aligned")
        shift = ((-base_address) % 16) // 4
        return [shift + r for r in self.rel]

    def guard_mask(self, base_address):
        mask = np.ones(self.total, bool)
        for o in self.offsets(base_address):
            mask[o:o + self.n] = False
        return mask


def arena_layout(n, width, misalign=ODD, order=None):
    """One buffer for len(misalign) planes of n elements: plane k starts 4 * misalign[k] bytes past a 16-byte boundary, the planes lie in
    memory in `order` (a permutation; default: as numbered), and max(256, 2 * width) guard elements lie before and after each.  Pure
    arithmetic: Layout.offsets(base address) gives the element offsets once the buffer exists."""
    k = len(misalign)
    order = list(range(k)) if order is None else list(order)
    if sorted(order) != list(range(k)) or any(not 0 <= m < 4 for m in misalign):
        raise ValueError("order must be a permutation and misalignments lie in 0..3")
    guard = max(256, 2 * int(width))
    rel, cursor = [0] * k, 0
    for plane in order:
        cursor += guard
        start = (cursor + 3) // 4 * 4 + misalign[plane]
        rel[plane] = start
        cursor = start + int(n)
    return Layout(n, guard, rel, cursor + guard + 3)            # (+ 3: the base may lie up to three elements before its boundary)


def _address(buf):
    return buf.data_ptr() if hasattr(buf, "data_ptr") else np.asarray(buf).ctypes.data


def _pattern(total):
    return (np.arange(total, dtype=np.uint32) ^ np.uint32(GUARD_WORD)).astype(np.uint32)


def fill_guards(buf, layout, base_address=None):
    """guard element i <- 0xA5A5A5A5 ^ i.  buf: `layout.total` 32-bit elements, a numpy array or a torch tensor (any 4-byte type)."""
    mask = layout.guard_mask(_address(buf) if base_address is None else base_address)
    pat = _pattern(layout.total)
    if hasattr(buf, "data_ptr"):
        import torch
        whole = torch.from_numpy(pat.view(np.int32)).to(buf.device)
        view = buf.view(torch.int32)
        where = torch.from_numpy(mask).to(buf.device)
        view[where] = whole[where]
    else:
        np.asarray(buf).view(np.uint32)[mask] = pat[mask]


def guards_intact(buf, layout, base_address=None):
    """-> the indices (ascending) of the guard elements that no longer hold their word; empty when all do"""
    mask = layout.guard_mask(_address(buf) if base_address is None else base_address)
    host = buf.detach().cpu().numpy() if hasattr(buf, "data_ptr") else np.asarray(buf)
    return np.flatnonzero(mask & (host.reshape(-1).view(np.uint32) != _pattern(layout.total)))


# ---- present ----------------------------------------------------------------------------------------------------------------------------
def present_reference(r, g, b, iterations):
    """app/Main.hs:351 (zipWith3 V3 r g b), fs.glsl:12 (texture.rgb / u_iterations) and the framebuffer's unorm8 conversion in binary32:
    -> (rgb float32 [..., 3], rgba uint8 [..., 4]).  NaN and everything below or at zero go to 0, everything above 1 (+inf too) to 1, then
    x * 255 + 0.5 truncated, each operation rounded on its own; alpha 255."""
    planes = [np.asarray(p, np.float32) for p in (r, g, b)]
    with np.errstate(all="ignore"):
        rgb = (np.stack(planes, -1) / np.float32(iterations)).astype(np.float32)
        clamped = np.where(rgb > 0, np.minimum(rgb, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        scaled = (clamped * np.float32(255.0)).astype(np.float32)
        bytes3 = (scaled + np.float32(0.5)).astype(np.float32).astype(np.uint32).astype(np.uint8)
    rgba = np.concatenate([bytes3, np.full(bytes3.shape[:-1] + (1,), 255, np.uint8)], -1)
    return rgb, rgba


def rounding_boundaries(iterations):
    """for every k in 0..255 the binary32 nearest (k + 0.5) / 255 * iterations and its two binary32 neighbours on each side (k-major)"""
    mid = (((np.arange(256, dtype=np.float64) + 0.5) / 255.0) * float(iterations)).astype(np.float32)
    lo1, hi1 = np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf))
    lo2, hi2 = np.nextafter(lo1, np.float32(-np.inf)), np.nextafter(hi1, np.float32(np.inf))
    return np.stack([lo2, lo1, mid, hi1, hi2], 1).reshape(-1).astype(np.float32)


def special_values(iterations):
    """what present_inputs plants, but for the non-finite ones: the rounding boundaries, -0.0, a denormal, negatives, 1 and the value
    whose quotient is 1, each with its neighbours"""
    one = np.float32(1.0)
    full = np.float32(iterations)
    near = []
    for v in (one, full):
        near += [np.nextafter(np.nextafter(v, np.float32(0)), np.float32(0)), np.nextafter(v, np.float32(0)), v,
                 np.nextafter(v, np.float32(np.inf)), np.nextafter(np.nextafter(v, np.float32(np.inf)), np.float32(np.inf))]
    rest = np.array([-0.0, 0.0, 1e-40, -1e-40, 1.1754944e-38, -1.0, -1e-3, -1e30, 1e30, 0.5], np.float32)
    return np.concatenate([rounding_boundaries(iterations), np.array(near, np.float32), rest]).astype(np.float32)


def present_inputs(n, iterations, seed=11):
    """-> (r, g, b), float32 arrays of n: +inf, -inf and NaN once in every channel position (pixels 0..8, the other two channels finite),
    then special_values(iterations) -- in r as listed, in g and b rolled by a third and two thirds, so that every channel sees every value
    beside other neighbours --, seeded uniform values in [0, 1.25 * iterations) for the rest.  A short n holds what fits."""
    rng = np.random.default_rng(seed + 1000 * int(iterations))
    planes = [(rng.random(n, dtype=np.float32) * np.float32(1.25 * iterations)).astype(np.float32) for _ in range(3)]
    special = special_values(iterations)
    at = 0
    for value in (np.inf, -np.inf, np.nan):
        for channel in range(3):
            if at < n:
                planes[channel][at] = value
            at += 1
    room = max(0, min(n - at, special.size))
    for channel in range(3):
        planes[channel][at:at + room] = np.roll(special, channel * (special.size // 3))[:room]
    return tuple(planes)
