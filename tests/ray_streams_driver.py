"""Child program of tests/test_gpu_ray_streams.py (not a test module): `python tests/ray_streams_driver.py WORKDIR [case numbers]`.

ptmi_trace_streams_device and ptmi_trace_streams_indexed_device through Context.trace_streams, as a PyTorch caller uses them: device
tensors in, colour and seeds updated in place, on the context's stream, in a process where torch brings the HIP runtime up before the
library is loaded (bench.py's order).  The scenes, their rays and the reference -- the contract of include/ptmi.h in plain C over the
oracle's public functions (tests/cxx/ray_streams_reference.c) -- are tests/ray_streams_inputs.py's; a reference is computed once per
(scene, cap, spp, start, seed rule) and shared by the cases.  Every comparison is bit for bit, colours by words (a NaN for a NaN).  One
line per case, `ok <case>` or `FAILED <case>: <why>`; a failed comparison does not end the process, a runtime error does; the last line
is RAY_STREAMS_DONE."""
import ctypes as C
import os
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import ray_query_driver as Q  # noqa: E402
from ray_query_driver import SENTINEL, bits, dev, guarded, guards_intact, host, same_words  # noqa: E402

CASES = ["1 colour seed and lost against the reference", "2 sizes alignment guards", "3 a camera's rays equal a render", "4 sample split",
         "5 indexed", "6 the drop scene", "7 isolation", "8 refusals"]
CAPS, SPPS = (2, 3, 12, 1 << 16), (1, 3)
SIZES = (0, 1, 63, 64, 65, 257)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

torch = pkg = B = W = inputs = ref = None
KINDS, SEED0 = [], 0
SCENES = {}
_REFS = {}


def setup(workdir):
    global torch, pkg, B, W, inputs, ref, KINDS, SEED0
    import torch as _torch
    torch = Q.torch = _torch
    torch.zeros(1, device="cuda")                      # torch brings the runtime up first
    torch.cuda.synchronize()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg._build.build_lib()
    B, W = pkg.binding, pkg.world
    import ray_streams_inputs as _inputs
    inputs = _inputs
    KINDS, SEED0 = inputs.KINDS, inputs.SEED0
    ref = inputs.Reference(workdir)


def set_scene(c, kind, data):
    spheres, triangles, planes = data
    if kind.startswith("mesh"):
        c.set_scene_mesh(spheres, triangles, planes)
    elif kind.startswith("bvh"):
        c.set_scene_bvh(spheres, planes)
    else:
        c.set_scene(spheres, planes)


class Scene:
    def __init__(self, kind):
        self.kind = kind
        self.data = inputs.scene(kind)
        self.glass = inputs.has_glass(kind)
        self.rays = inputs.batch(kind, self.data, ref)
        self.n = len(self.rays)
        self.d_rays = dev(self.rays)
        torch.cuda.synchronize()
        self.ctx = pkg.Context(0)
        set_scene(self.ctx, kind, self.data)
        self.cap, self.rule = 1 << 16, B.SEED_AUTO

    def options(self, cap=1 << 16, rule=None):
        """the step cap and the seed rule of the scene's context (rule None = PTMI_SEED_AUTO)"""
        rule = B.SEED_AUTO if rule is None else rule
        if cap != self.cap:
            self.ctx.set_option(B.OPT_STREAM_STEP_CAP, cap)
        if rule != self.rule:
            self.ctx.set_option(B.OPT_STREAMS_SEED_RULE, rule)
        self.cap, self.rule = cap, rule


def start_colour(n, tag):
    """A start colour by name: zeros, or seeded values with -0.0, a NaN and an infinity among them"""
    if tag == "zero":
        return np.zeros((n, 3), np.float32)
    c = np.random.default_rng(17).normal(size=(n, 3)).astype(np.float32)
    if n > 7:
        c[5], c[6, 1], c[7, 2] = -0.0, np.nan, np.inf
    return c


def reference(kind, cap, spp, start="zero", rule=None):
    """(colour, seeds, lost) of the reference after spp samples from `start` and genSeeds(SEED0), computed once"""
    key = (kind, cap, spp, start, rule)
    if key not in _REFS:
        sc = SCENES[kind]
        from_result = None if rule is None else rule == B.SEED_FROM_RESULT
        _REFS[key] = ref.trace(sc.data, sc.rays, start_colour(sc.n, start), ref.seeds(sc.n), spp, cap=cap, from_result=from_result)[:3]
    return _REFS[key]


def d_seeds(n):
    return dev(ref.seeds(n).view(np.int32))


def run(c, rays, seeds, spp, color, index=None, lost=None, work=None):
    """Context.trace_streams on the context's OWN stream from torch's, with host waits on either side (the header's ordering rule)"""
    if color is None:
        color = torch.zeros((int(rays.shape[0]), 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    out = c.trace_streams(rays, seeds, spp=spp, color=color, index=index, lost=lost, work=work)
    c.synchronize()
    assert out is color
    return out


def compare(color, seeds, want, what, rows=None):
    w_color, w_seeds = want[0], want[1]
    g_color, g_seeds = host(color).reshape(-1, 3), host(seeds).view(np.uint32).reshape(-1, 4)
    if rows is not None:
        g_color, g_seeds, w_color, w_seeds = g_color[rows], g_seeds[rows], w_color[rows], w_seeds[rows]
    bad = np.flatnonzero((g_seeds != w_seeds).any(1))
    assert bad.size == 0, "%s: %d seeds differ, e.g. ray %d: %r, the reference has %r" % (what, bad.size, bad[0], g_seeds[bad[0]], w_seeds[bad[0]])
    bad = same_words(g_color, w_color)
    assert bad.size == 0, "%s: %d colours differ, e.g. ray %d: %r, the reference has %r" % (what, bad.size, bad[0], g_color[bad[0]], w_color[bad[0]])


def new_lost(values=(0, 0)):
    return dev(np.array(values, np.int64))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

def case_reference():
    """1: colour, seed and d_lost are the reference's, every scene, 1 and 3 spp, caps 2, 3, 12 and 65536, from a zero colour and from one
    with -0.0, a NaN and an infinity; an explicit PTMI_SEED_KEEP_ACCUMULATOR on the scenes without glass as well"""
    for kind in KINDS:
        sc = SCENES[kind]
        rules = (None,) if sc.glass else (None, B.SEED_KEEP_ACCUMULATOR)
        for rule in rules:
            for cap in CAPS:
                sc.options(cap, rule)
                for spp, start in ((1, "zero"), (3, "mixed"), (3, "zero"), (1, "mixed")) if rule is None and cap in (3, 1 << 16) else ((1, "zero"), (3, "mixed")):
                    what = "%s, rule %s, cap %d, %d spp from a %s colour" % (kind, rule, cap, spp, start)
                    seeds, color, lost = d_seeds(sc.n), dev(start_colour(sc.n, start)), new_lost((5, 7))
                    run(sc.ctx, sc.d_rays, seeds, spp, color, lost=lost)
                    want = reference(kind, cap, spp, start, rule)
                    compare(color, seeds, want, what)
                    got_lost = host(lost) - np.array([5, 7])
                    assert np.array_equal(got_lost, want[2]), "%s: lost %r, the reference has %r" % (what, got_lost, want[2])
        sc.options()
        if not sc.glass:                                # the two rules differ where a sample has a second hit
            a, b = reference(kind, 1 << 16, 1, "zero", None), reference(kind, 1 << 16, 1, "zero", B.SEED_KEEP_ACCUMULATOR)
            assert (a[1] != b[1]).any() and np.array_equal(bits(a[0]), bits(b[0])), kind


def case_sizes():
    """2: wave and block tails; rays, colour and seeds 16-byte aligned and 4 bytes off; guard words around colour, seeds, lost and the
    workspace, which is exactly trace_streams_bytes(n) long"""
    for kind in KINDS:
        sc = SCENES[kind]
        sc.options(12)
        want = reference(kind, 12, 2, "mixed")
        for n in SIZES:
            for misalign in (False, True):
                what = "%s, n = %d, %s" % (kind, n, "4 bytes off" if misalign else "aligned")
                rbuf, rays, _ = guarded(n, 6, torch.float32, misalign)
                cbuf, color, cstart = guarded(n, 3, torch.float32, misalign)
                sbuf, seeds, sstart = guarded(n, 4, torch.int32, misalign)
                need = sc.ctx.trace_streams_bytes(n)
                assert need == ((n + 63) // 64) * 4 * 64 * 64 and need % 16 == 0
                wbuf, work, wstart = guarded(need // 4, 1, torch.int32, False)
                work = work.view(torch.uint8)
                assert n == 0 or work.data_ptr() % 16 == 0
                lbuf, lost, lstart = guarded(2, 2, torch.int32, False)
                lost = lost.view(torch.int64).view(2)
                lost.zero_()
                if n:
                    rays.copy_(sc.d_rays[:n])
                    color.copy_(dev(start_colour(sc.n, "mixed")[:n]))
                    seeds.copy_(d_seeds(sc.n)[:n])
                run(sc.ctx, rays, seeds, 2, color, lost=lost, work=work)
                guards_intact(cbuf, cstart, 3 * n, what + ": colour")
                guards_intact(sbuf, sstart, 4 * n, what + ": seeds")
                guards_intact(wbuf, wstart, need // 4, what + ": the workspace")
                guards_intact(lbuf, lstart, 4, what + ": lost")
                if n:
                    compare(color, seeds, (want[0][:n], want[1][:n]), what)
        sc.options()


def case_camera():
    """3: a camera's primary rays at 64 x 32, path_seeds' seeds and a zero colour == init_output + render(STREAMS, PTMI_FORM_PIXEL) on all
    seven planes, bit for bit, on one scene per kind with and without GLASS and under both seed rules; d_lost == the stats' truncated and
    dropped deltas"""
    w, h, cam = 64, 32, W.initial_camera()
    n = w * h
    rays = dev(ref.primaries(cam, w, h))
    for kind in inputs.PLAIN + inputs.GLASS:
        glass = inputs.has_glass(kind)
        data = inputs.plain_glass_scene(kind) if glass else inputs.scene(kind)
        for rule, cap in ((None, 1 << 16), (B.SEED_KEEP_ACCUMULATOR, 3)) if not glass else ((None, 1 << 16), (None, 3)):
            what = "%s, rule %s, cap %d" % (kind, rule, cap)
            torch.cuda.synchronize()
            with pkg.Context(0) as c:
                set_scene(c, kind, data)
                c.set_option(B.OPT_STREAMS_FORM, B.FORM_PIXEL)
                c.set_option(B.OPT_STREAM_STEP_CAP, cap)
                if rule is not None:
                    c.set_option(B.OPT_STREAMS_SEED_RULE, rule)
                seeds = c.path_seeds(SEED0, n)
                lost = new_lost()
                color = run(c, rays, seeds, 3, None, lost=lost)
                c.resize(w, h)
                c.init_output(SEED0)
                before = c.stats()
                c.render(cam, 8, 3, pkg.STREAMS)
                planes = c.download_state()
                after = c.stats()
            g_color, g_seeds = host(color), host(seeds).view(np.uint32)
            for k, name in enumerate("rgb"):
                assert np.array_equal(bits(g_color[:, k]), bits(np.asarray(planes[k], np.float32).reshape(-1))), "%s: plane %s" % (what, name)
            for k, name in enumerate(("sa", "sb", "sc", "sctr")):
                assert np.array_equal(g_seeds[:, k], np.asarray(planes[3 + k]).view(np.uint32).reshape(-1)), "%s: plane %s" % (what, name)
            assert np.any(g_color != 0)
            deltas = [after[k] - before[k] for k in ("stream_rays_truncated", "stream_rays_dropped")]
            assert host(lost).tolist() == deltas, "%s: lost %r, the render's statistics moved by %r" % (what, host(lost).tolist(), deltas)
            if cap == 3:
                assert deltas[0] > 0, what


def case_split():
    """4: one call of 3 spp == three calls of 1 spp == the reference, colour, seeds and lost"""
    for kind in KINDS:
        sc = SCENES[kind]
        sc.options(12)
        want = reference(kind, 12, 3, "mixed")
        seeds, color, lost = d_seeds(sc.n), dev(start_colour(sc.n, "mixed")), new_lost()
        for _ in range(3):
            run(sc.ctx, sc.d_rays, seeds, 1, color, lost=lost)
        compare(color, seeds, want, "%s, three calls of 1 spp" % kind)
        assert np.array_equal(host(lost), want[2]), kind
        sc.options()


def case_indexed():
    """5: through ray_order's permutation the plain call's words; through a live-style list (-1 padding, entries outside [0, n)) the named
    rays alone are updated, the rest keeps every bit and the guards stand"""
    rng = np.random.default_rng(21)
    for kind in KINDS:
        sc = SCENES[kind]
        n = sc.n
        sc.options(12)
        want = reference(kind, 12, 2, "mixed")
        work = torch.empty(B.ray_order_bytes(n), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        order = sc.ctx.ray_order(sc.d_rays, work=work)
        sc.ctx.synchronize()
        assert np.array_equal(np.sort(host(order)), np.arange(n)), kind
        seeds, color, lost = d_seeds(n), dev(start_colour(n, "mixed")), new_lost()
        run(sc.ctx, sc.d_rays, seeds, 2, color, index=order, lost=lost)
        compare(color, seeds, want, "%s through the device order" % kind)
        assert np.array_equal(host(lost), want[2]), kind
        for m in (1, 65, 300):
            for misalign in (False, True):
                what = "%s, a list of %d, %s" % (kind, m, "4 bytes off" if misalign else "aligned")
                picks = rng.permutation(n)[:m].astype(np.int64)                 # every ray at most once
                if m >= 65:
                    picks[[1, 17, 40, 62]] = [-1, n, INT32_MIN, INT32_MAX]
                    picks[m - 20:] = -1                                           # the live list's padding
                named = picks[(picks >= 0) & (picks < n)]
                ibuf, d_index, istart = guarded(m, 1, torch.int32, misalign)
                d_index.copy_(dev(picks.astype(np.int32)))
                cbuf, color, cstart = guarded(n, 3, torch.float32, misalign)
                sbuf, seeds, sstart = guarded(n, 4, torch.int32, misalign)
                color.copy_(dev(start_colour(n, "mixed")))
                seeds.copy_(d_seeds(n))
                run(sc.ctx, sc.d_rays, seeds, 2, color, index=d_index)
                guards_intact(cbuf, cstart, 3 * n, what + ": colour")
                guards_intact(sbuf, sstart, 4 * n, what + ": seeds")
                guards_intact(ibuf, istart, m, what + ": the index")
                assert np.array_equal(host(d_index), picks.astype(np.int32)), what + ": the index was written"
                rest = np.setdiff1d(np.arange(n), named)
                compare(color, seeds, want, what + ", the named rays", rows=named)
                compare(color, seeds, (start_colour(n, "mixed"), ref.seeds(n)), what + ", the rays no entry names", rows=rest)
        seeds, color = d_seeds(n), dev(start_colour(n, "mixed"))                  # m == 0
        run(sc.ctx, sc.d_rays, seeds, 2, color, index=torch.zeros(0, dtype=torch.int32, device="cuda"))
        compare(color, seeds, (start_colour(n, "mixed"), ref.seeds(n)), "%s, an empty index" % kind)
        sc.options()


def case_drop():
    """6: on the drop scene children are dropped, as many as the reference drops; without d_lost the same colour and seeds"""
    sc = SCENES["drop"]
    want = reference("drop", 1 << 16, 2, "zero")
    assert want[2][1] > 0 and want[2][0] == 0
    seeds, lost = d_seeds(sc.n), new_lost()
    color = run(sc.ctx, sc.d_rays, seeds, 2, None, lost=lost)
    compare(color, seeds, want, "the drop scene")
    assert np.array_equal(host(lost), want[2]), (host(lost), want[2])
    seeds = d_seeds(sc.n)
    color = run(sc.ctx, sc.d_rays, seeds, 2, None)
    compare(color, seeds, want, "the drop scene without d_lost")


def case_isolation():
    """7: a render's planes, ptmi_get_stats and the dispatch order state -- the next render's planes and statistics -- are what they are
    without the calls; a set_scene enqueued right after a call does not disturb it"""
    from conftest import assert_planes_equal
    cam = W.initial_camera()
    for kind in ("glass", "main", "bvh_glass", "mesh_glass"):
        sc = SCENES[kind]
        want = reference(kind, 1 << 16, 2)
        seeds, color = d_seeds(sc.n), dev(start_colour(sc.n, "zero"))
        torch.cuda.synchronize()
        with pkg.Context(0) as c:
            set_scene(c, kind, sc.data)
            c.set_option(B.OPT_STREAMS_FORM, B.FORM_PIXEL)
            c.resize(64, 48)
            rounds = []
            for calls in (False, True):
                start = c.stats()
                c.init_output(SEED0)
                if calls:
                    c.trace_streams(sc.d_rays, seeds, spp=1, color=color)
                c.render(cam, 4, 2, pkg.STREAMS)
                mid = c.download_state()
                if calls:
                    before = c.stats()
                    c.trace_streams(sc.d_rays, seeds, spp=1, color=color)
                    c.synchronize()
                    after = c.stats()
                    moved = [k for k in after if k != "last_render_ms" and after[k] != before[k]]
                    assert not moved, "%s: a call moved the statistics %r" % (kind, moved)
                    assert_planes_equal(c.download_state(), mid, "%s: the planes behind a call" % kind)
                c.render(cam, 4, 1, pkg.STREAMS)             # in the dispatch order the render before it recorded
                end = c.stats()
                rounds.append((mid, c.download_state(), {k: end[k] - start[k] for k in end if k not in ("last_render_ms", "stream_iterations")},
                               end["stream_iterations"]))
            assert_planes_equal(rounds[1][0], rounds[0][0], "%s: the render behind a call" % kind)
            assert_planes_equal(rounds[1][1], rounds[0][1], "%s: the next render" % kind)
            assert rounds[1][2:] == rounds[0][2:], "%s: the statistics of renders around the calls %r, without them %r" % (kind, rounds[1][2:], rounds[0][2:])
            assert np.any(np.asarray(rounds[0][1][0]) != 0.0)
            c.synchronize()
            compare(color, seeds, want, "%s: calls around renders" % kind)
    # a scene call right behind: ordered behind the launch by the stream alone
    sc, other = SCENES["bvh_glass"], SCENES["main"]
    want = reference("bvh_glass", 1 << 16, 2)
    seeds, color = d_seeds(sc.n), dev(start_colour(sc.n, "zero"))
    torch.cuda.synchronize()
    with pkg.Context(0) as c:
        set_scene(c, "bvh_glass", sc.data)
        c.trace_streams(sc.d_rays, seeds, spp=2, color=color)
        set_scene(c, "main", other.data)
        c.synchronize()
    compare(color, seeds, want, "a set_scene right behind the call")


def case_refusals():
    """8: through the raw library handle, nothing written: PTMI_ESTATE before a scene; PTMI_EINVAL for a negative n or m, NULL required
    pointers with a positive count, a misaligned d_lost, a NULL, misaligned or short d_work on a GLASS scene, GLASS with an explicit
    PTMI_SEED_FROM_RESULT; d_work NULL accepted without GLASS; n == 0, m == 0 and n_spp <= 0 are PTMI_OK and touch nothing"""
    sc, plain = SCENES["bvh_glass"], SCENES["bvh"]
    n, m = 65, 40
    cbuf, color, _ = guarded(n, 3, torch.float32, False)
    sbuf, seeds, _ = guarded(n, 4, torch.int32, False)
    lbuf, lost, _ = guarded(2, 2, torch.int32, False)
    d_index = dev(np.arange(m, dtype=np.int32))
    need = B.load_library().ptmi_trace_streams_bytes(n)
    wbuf, work, _ = guarded(need // 4, 1, torch.int32, False)
    torch.cuda.synchronize()
    vp = lambda x, off=0: C.c_void_p(x.data_ptr() + off)  # noqa: E731
    rays, col, sd, index, lo, wk = vp(sc.d_rays), vp(color), vp(seeds), vp(d_index), vp(lost), vp(work)
    assert work.data_ptr() % 16 == 0 and lost.data_ptr() % 8 == 0

    def untouched(what):
        torch.cuda.synchronize()
        for buf in (cbuf, sbuf, lbuf, wbuf):
            assert (host(buf).view(np.uint32) == SENTINEL).all(), "%s wrote to an output" % what

    lib = B.load_library()
    assert lib.ptmi_trace_streams_bytes(0) == 0 and lib.ptmi_trace_streams_bytes(-5) == 0 and lib.ptmi_trace_streams_bytes(64) == 4 * 64 * 64
    assert lib.ptmi_trace_streams_bytes(65) == 2 * 4 * 64 * 64 and lib.ptmi_trace_streams_bytes(INT32_MAX) == (2 ** 31 // 64) * 4 * 64 * 64
    with pkg.Context(0) as c:
        h = c._h
        P, X = lib.ptmi_trace_streams_device, lib.ptmi_trace_streams_indexed_device
        assert P(h, rays, n, 1, col, sd, lo, wk, need) == B.PTMI_ESTATE and X(h, rays, n, index, m, 1, col, sd, lo, wk, need) == B.PTMI_ESTATE
        untouched("a call before any scene")
        set_scene(c, "bvh_glass", sc.data)
        for rc in (P(h, None, n, 1, col, sd, lo, wk, need), P(h, rays, n, 1, None, sd, lo, wk, need), P(h, rays, n, 1, col, None, lo, wk, need),
                   P(h, rays, -1, 1, col, sd, lo, wk, need), P(h, rays, n, 1, col, sd, vp(lost, 4), wk, need),
                   P(h, rays, n, 1, col, sd, lo, None, need), P(h, rays, n, 1, col, sd, lo, vp(work, 8), need), P(h, rays, n, 1, col, sd, lo, wk, need - 1),
                   P(h, rays, n, 1, col, sd, lo, wk, 0),
                   X(h, None, n, index, m, 1, col, sd, lo, wk, need), X(h, rays, n, index, m, 1, None, sd, lo, wk, need),
                   X(h, rays, n, index, m, 1, col, None, lo, wk, need), X(h, rays, -1, index, m, 1, col, sd, lo, wk, need),
                   X(h, rays, n, index, -1, 1, col, sd, lo, wk, need), X(h, rays, n, None, m, 1, col, sd, lo, wk, need),
                   X(h, rays, n, index, m, 1, col, sd, vp(lost, 4), wk, need), X(h, rays, n, index, m, 1, col, sd, lo, None, need),
                   X(h, rays, n, index, 65, 1, col, sd, lo, wk, lib.ptmi_trace_streams_bytes(64))):
            assert rc == B.PTMI_EINVAL, rc
        assert X(h, rays, n, index, m, 1, col, sd, lo, wk, lib.ptmi_trace_streams_bytes(m)) == B.PTMI_OK      # lanes is m with an index
        c.synchronize()
        seeds.copy_(dev(np.full((n, 4), SENTINEL, np.int32))); color.copy_(dev(np.full((n, 3), SENTINEL, np.int32)).view(torch.float32))
        lost.fill_(SENTINEL); work.fill_(SENTINEL)
        torch.cuda.synchronize()
        assert P(h, None, 0, 1, None, None, None, None, 0) == B.PTMI_OK and P(h, rays, n, 0, col, sd, lo, wk, need) == B.PTMI_OK
        assert P(h, rays, n, -1, col, sd, lo, wk, need) == B.PTMI_OK
        assert X(h, rays, n, None, 0, 1, col, sd, lo, wk, need) == B.PTMI_OK and X(h, None, 0, index, m, 1, None, None, None, None, 0) == B.PTMI_OK
        c.synchronize()
        untouched("a refused or empty call")
        c.set_option(B.OPT_STREAMS_SEED_RULE, B.SEED_FROM_RESULT)
        assert P(h, rays, n, 1, col, sd, lo, wk, need) == B.PTMI_EINVAL and b"PTMI_SEED_FROM_RESULT" in lib.ptmi_last_error(h)
        assert X(h, rays, n, index, m, 1, col, sd, lo, wk, need) == B.PTMI_EINVAL
        c.synchronize()
        untouched("GLASS under an explicit PTMI_SEED_FROM_RESULT")
        # without GLASS the workspace is ignored: NULL, misaligned and short are all accepted, and it is not written
        set_scene(c, "bvh", plain.data)
        want = reference("bvh", 1 << 16, 1, "zero", B.SEED_FROM_RESULT)
        for wk_arg, size in ((None, 0), (vp(work, 4), 3), (wk, need)):
            s2, c2 = d_seeds(plain.n)[:n].contiguous(), torch.zeros((n, 3), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            assert P(h, vp(plain.d_rays), n, 1, vp(c2), vp(s2), None, wk_arg, size) == B.PTMI_OK
            c.synchronize()
            compare(c2, s2, (want[0][:n], want[1][:n]), "without GLASS, a workspace of %d bytes" % size)
        assert (host(wbuf).view(np.uint32) == SENTINEL).all(), "a scene without GLASS wrote to the workspace"


RUN = dict(zip(CASES, (case_reference, case_sizes, case_camera, case_split, case_indexed, case_drop, case_isolation, case_refusals)))


def main():
    setup(sys.argv[1])
    only = sys.argv[2:]
    for kind in KINDS:
        SCENES[kind] = Scene(kind)
    for name in CASES:
        if only and name[0] not in only:
            continue
        try:
            RUN[name]()
            print("ok %s" % name, flush=True)
        except AssertionError as e:
            print("FAILED %s: %s" % (name, str(e).replace("\n", " ")[:1500] or traceback.format_exc()[-1500:].replace("\n", " | ")), flush=True)
        except B.PtmiError as e:                     # a runtime error: nothing more is started on the device
            print("FAILED %s: %s" % (name, e), flush=True)
            raise SystemExit(3)
    for sc in SCENES.values():
        sc.ctx.close()
    print("RAY_STREAMS_DONE", flush=True)


if __name__ == "__main__":
    main()
