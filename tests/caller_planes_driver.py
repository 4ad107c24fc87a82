"""Child program of tests/test_gpu_caller_planes.py (not a test module): `python tests/caller_planes_driver.py GROUP [tiny-rings library]`.

A PyTorch caller's path -- ptmi_bind_planes with seven tensor addresses, ptmi_set_stream with torch's stream, ptmi_get_planes,
ptmi_snapshot_color -- on a real device, in a process where torch brings the HIP runtime up first (bench.py's order).  Every case binds
a context to an ARENA (tests/caller_planes.py): seven planes inside a torch buffer, each at its own alignment, in shuffled order, a
guard band on both sides -- or seven allocations of their own.  After the calls all guards must be intact and the planes, read with
torch, equal the CPU oracle's bit for bit (a twin context with owned planes only where the table of the issue says so; the GLASS stream
form by its tolerance).  One line per case, the first failure ends the process, the last line is CALLER_PLANES_OK <count>; CASES lists
the names each group prints, and the parent compares."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import caller_planes as cp  # noqa: E402

SEED0 = 0x5EED1234
CAP = 1 << 16
SENTINEL = 0x7FC0DEAD                        # a NaN as a float, an unlikely seed word
KINDS3 = ("ODD", "ALIGNED", "SEPARATE")
KINDS2 = ("ODD", "ALIGNED")
PRESENT_SIZES = ((64, 48), (61, 7), (9, 2), (1, 1))          # n % 4 = 0, 3, 2, 1
PRESENT_ITERATIONS = (1, 7, 1000)
ROW_C = ((37, 13, 8, 2), (1, 64, 8, 2), (64, 1, 8, 2), (1, 1, 8, 2), (64, 16, 0, 2), (64, 16, 8, 0))

CASES = {
    "inline": ["a %s" % k for k in KINDS3]
              + ["b variant %d%s" % (v, ch) for v, ch in ((4, ""), (5, ""), (13, ""), (17, ""), (13, " chunks 4"), (17, " chunks 4"))]
              + ["c %dx%d limit %d spp %d" % c for c in ROW_C]
              + ["j %dx%d %s" % (w, h, alg) for (w, h) in ((64, 48), (61, 23)) for alg in ("inline", "stream form")],
    "streams": ["d %s" % k for k in KINDS3] + ["e ODD"]
               + ["f %s %s" % (t, k) for t in ("automatic tail", "tail 950") for k in KINDS3]
               + ["g stream form ODD", "g redone call ODD"],
    "scenes": ["h %s %s" % (alg, k) for k in KINDS3 for alg in ("inline", "streams", "tree walk")]
              + ["i %s %s" % (alg, when) for when in ("as set", "after update_mesh_vertices") for alg in ("inline", "streams")],
    "helpers": ["%s %s" % (what, k) for k in KINDS2 for what in ("init_output reseed create_with", "partition seeds", "upload download")]
               + ["present %dx%d %s" % (w, h, k) for k in KINDS2 for (w, h) in PRESENT_SIZES]
               + ["snapshot_color %s" % k for k in KINDS2] + ["device_planes %s" % k for k in KINDS2]
               + ["lifecycle unbind", "lifecycle rebind", "lifecycle partial bind", "lifecycle bind before resize", "lifecycle resize while bound"],
    "stream": ["caller stream %s %s" % (case, how) for case in ("inline 97x61", "streams 72x40", "stream form tail 128x64")
               for how in ("torch stream", "own stream", "second torch stream")] + ["bench configuration"],
}

torch = pkg = B = W = ora = cam = cam2 = None
assert_planes_equal = initial_planes = initial_rows = None
THREADS = max(1, min(16, os.cpu_count() or 1))
_group, _count = None, 0


def setup(group):
    """torch first (it brings the runtime up, as in bench.py), then the library"""
    global torch, pkg, B, W, ora, cam, cam2, assert_planes_equal, initial_planes, initial_rows, _group
    import torch as _torch
    torch = _torch
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    import __graft_entry__ as graft
    import conftest
    pkg = graft.load_package()
    pkg._build.build_lib()
    ora = graft.load_oracle()
    ora.build()
    B, W = pkg.binding, pkg.world
    cam = W.initial_camera()
    cam2 = cam.copy()
    cam2["position"][0] += 0.25
    assert_planes_equal, initial_planes, initial_rows = conftest.assert_planes_equal, conftest.initial_planes, conftest.initial_rows
    _group = group


def ok(name):
    global _count
    want = CASES[_group][_count] if _count < len(CASES[_group]) else None
    if name != want:
        raise SystemExit("case %r ran where %r was expected" % (name, want))
    _count += 1
    print("ok %s" % name, flush=True)


def fail(msg):
    raise SystemExit("FAILED: " + msg)


class Arena:
    """Seven planes of n elements in torch memory, laid out as `kind` says; guards filled, planes holding the sentinel."""

    def __init__(self, n, width, kind):
        self.n, self.kind, self.blocks, self.views = n, kind, [], [None] * 7
        if kind == "SEPARATE":
            for k in cp.SEPARATE_ORDER:
                lay = cp.arena_layout(n, width, (cp.SEPARATE_MISALIGN[k],))
                buf = torch.empty(lay.total, dtype=torch.int32, device="cuda")
                o = lay.offsets(buf.data_ptr())[0]
                self.blocks.append((buf, lay))
                self.views[k] = buf[o:o + n]
            want = cp.SEPARATE_MISALIGN
        else:
            want = cp.ALIGNED if kind == "ALIGNED" else cp.ODD
            lay = cp.arena_layout(n, width, want, cp.ORDER)
            buf = torch.empty(lay.total, dtype=torch.int32, device="cuda")
            self.blocks.append((buf, lay))
            for k, o in enumerate(lay.offsets(buf.data_ptr())):
                self.views[k] = buf[o:o + n]
        self.ptrs = [v.data_ptr() for v in self.views]
        assert [p % 16 for p in self.ptrs] == [4 * m for m in want], (kind, self.ptrs)
        for buf, lay in self.blocks:
            cp.fill_guards(buf, lay)
        self.fill(SENTINEL)
        torch.cuda.synchronize()

    def bind(self, ctx):
        ctx.bind_planes(self.ptrs, keep=self)
        if ctx.device_planes() != self.ptrs:
            fail("ptmi_get_planes does not return the bound addresses")

    def fill(self, word):
        for v in self.views:
            v.fill_(word)

    def write(self, planes):
        """seven host planes -> the arena (torch copies), complete on return"""
        for v, p in zip(self.views, planes):
            v.copy_(torch.from_numpy(np.ascontiguousarray(p).reshape(-1).view(np.int32).copy()))
        torch.cuda.synchronize()

    def read(self):
        out = [v.cpu().numpy() for v in self.views]
        return [a.view(np.float32) for a in out[:3]] + [a.view(np.uint32) for a in out[3:]]

    def check(self, what):
        for k, (buf, lay) in enumerate(self.blocks):
            bad = cp.guards_intact(buf, lay)
            if bad.size:
                off = lay.offsets(buf.data_ptr())
                fail("%s: %d guard elements of buffer %d (%s) were written, first at element %d (planes begin at %r, %d elements each)"
                     % (what, bad.size, k, self.kind, bad[0], off, lay.n))


def exact(got, want, what):
    try:
        assert_planes_equal(got, want, what)
    except AssertionError as e:
        fail(str(e))


def glass_rule(got, want, what):
    """the GLASS stream form: its additions have no defined order -- generator planes equal, colours to 1e-4 of max(|b|, 1e-3)"""
    for name, a, b in zip(cp.NAMES[3:], got[3:], want[3:]):
        if not np.array_equal(np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)):
            fail("%s: generator plane %s differs" % (what, name))
    for name, a, b in zip(cp.NAMES[:3], got[:3], want[:3]):
        a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
        err = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3)))
        print("   %s plane %s: largest |a - b| / max(|b|, 1e-3) = %.3g" % (what, name, err), flush=True)
        if not err <= 1e-4:
            fail("%s: colour plane %s is off by %.3g (> 1e-4)" % (what, name, err))


def bound(scene, w, h, kind, set_scene="set_scene", partition=None, library=None):
    """-> (context bound to a fresh arena, the arena)"""
    c = pkg.Context(0, library=library) if library is not None else pkg.Context(0)
    getattr(c, set_scene)(*scene)
    if partition:
        c.set_partition(*partition)
    c.resize(w, h)
    a = Arena(c.local_rows * w, w, kind)
    a.bind(c)
    return c, a


def render_and_compare(c, a, calls, wants, what, compare=exact):
    """every call, then ONE wait, the guards, the planes read with torch against wants[k]"""
    for k, (call, want) in enumerate(zip(calls, wants)):
        c.render(*call)
        c.synchronize()
        a.check("%s, launch %d" % (what, k))
        compare(a.read(), want, "%s, launch %d" % (what, k))


# ---- group inline: rows a, b, c, j ------------------------------------------------------------------------------------------------------
def group_inline():
    sp, pl = W.scene16()
    # a: the automatic choice; launches 1 to 4 with one camera record their cost, sort, dispatch in order; the fifth has another key
    w, h = 97, 61
    start = initial_planes(ora, w, h)
    steps = [(cam, 3), (cam, 1), (cam, 2), (cam, 1), (cam2, 2)]
    wants, cur = [], start
    for c_, spp in steps:
        cur, _ = ora.render_inline(sp, pl, c_, w, h, 15, spp, cur, n_threads=THREADS)
        wants.append(cur)
    for kind in KINDS3:
        c, a = bound((sp, pl), w, h, kind)
        with c:
            a.write(start)
            render_and_compare(c, a, [(c_, 15, spp, pkg.INLINE) for c_, spp in steps], wants, "a %s" % kind)
        ok("a %s" % kind)
    # b: the named variants of the product library, 13 and 17 also in four sample chunks
    w, h = 64, 48
    start = initial_planes(ora, w, h)
    want, _ = ora.render_inline(sp, pl, cam, w, h, 8, 4, start, n_threads=THREADS)
    for variant, chunks in ((4, 0), (5, 0), (13, 0), (17, 0), (13, 4), (17, 4)):
        c, a = bound((sp, pl), w, h, "ODD")
        with c:
            c.set_variant(variant)
            if chunks:
                c.set_option(B.OPT_SPP_CHUNKS, chunks)
            a.write(start)
            name = "b variant %d%s" % (variant, " chunks 4" if chunks else "")
            render_and_compare(c, a, [(cam, 8, 4, pkg.INLINE)], [want], name)
        ok(name)
    # c: the row mapping (below 64 x 16) and degenerate sizes; limit 0 and spp 0 on the smallest tiled size
    mp = W.main_scene()
    for (w, h, limit, spp) in ROW_C:
        start = initial_planes(ora, w, h)
        want, _ = ora.render_inline(mp[0], mp[1], cam, w, h, limit, spp, start)
        c, a = bound(mp, w, h, "ODD")
        with c:
            a.write(start)
            name = "c %dx%d limit %d spp %d" % (w, h, limit, spp)
            render_and_compare(c, a, [(cam, limit, spp, pkg.INLINE)], [want], name)
        ok(name)
    # j: three parts, each bound to an arena of its own rows, seeded by init_output from the global rows, stitched
    for (w, h) in ((64, 48), (61, 23)):
        start = initial_planes(ora, w, h)
        for alg in ("inline", "stream form"):
            if alg == "inline":
                want, _ = ora.render_inline(sp, pl, cam, w, h, 8, 2, start, n_threads=THREADS)
            else:
                want, _ = ora.render_streams(sp, pl, cam, w, h, CAP, 2, start, n_threads=THREADS)
            stitched = [np.zeros((h, w), np.float32) for _ in range(3)] + [np.zeros((h, w), np.uint32) for _ in range(4)]
            seen = 0
            for part in range(3):
                c, a = bound((sp, pl), w, h, "ODD", partition=(4, 3, part))
                with c:
                    if alg != "inline":
                        c.set_option(B.OPT_STREAMS_FORM, B.FORM_STREAM)
                    rows = c.global_rows()
                    c.init_output(SEED0)
                    c.render(cam, 8, 2, pkg.INLINE if alg == "inline" else pkg.STREAMS)
                    c.synchronize()
                    a.check("j %dx%d %s part %d" % (w, h, alg, part))
                    for s, g in zip(stitched, a.read()):
                        s[rows] = g.reshape(len(rows), w)
                    seen += len(rows)
            if seen != h:
                fail("j: the parts hold %d rows of %d" % (seen, h))
            exact(stitched, want, "j %dx%d %s, stitched" % (w, h, alg))
            ok("j %dx%d %s" % (w, h, alg))


# ---- group streams: rows d, e, f, g -----------------------------------------------------------------------------------------------------
def group_streams(tiny_rings):
    sp, pl = W.scene16()
    glass = W.glass_scene()
    w, h = 72, 40
    start = initial_planes(ora, w, h)
    want, _ = ora.render_streams(sp, pl, cam, w, h, CAP, 2, start, n_threads=THREADS)
    for kind in KINDS3:
        c, a = bound((sp, pl), w, h, kind)
        with c:
            a.write(start)
            render_and_compare(c, a, [(cam, 8, 2, pkg.STREAMS)], [want], "d %s" % kind)
        ok("d %s" % kind)
    want = ora.render_streams_tree(glass[0], glass[1], cam, w, h, CAP, 2, start, n_threads=THREADS)[0]
    c, a = bound(glass, w, h, "ODD")
    with c:
        a.write(start)
        render_and_compare(c, a, [(cam, 8, 2, pkg.STREAMS)], [want], "e ODD")
        if c.stats()["stream_rays_dropped"] != 0:
            fail("e: the tree walk dropped rays")
    ok("e ODD")
    # f: the stream form without GLASS: bit-identical to the chain.  The order and the tail's boundary are built before launches 2 and 3;
    # launches 3 and 4 run the tail on the context's side stream where the boundary leaves it positions
    w, h = 128, 64
    start = initial_planes(ora, w, h)
    wants, cur = [], start
    for _ in range(4):
        cur, _ = ora.render_streams(sp, pl, cam, w, h, CAP, 2, cur, n_threads=THREADS)
        wants.append(cur)
    for tail in (None, 950):
        for kind in KINDS3:
            c, a = bound((sp, pl), w, h, kind)
            with c:
                c.set_option(B.OPT_STREAMS_FORM, B.FORM_STREAM)
                if tail is not None:
                    c.set_option(B.OPT_STREAM_TAIL, tail)
                    if c.get_option(B.OPT_STREAM_TAIL) != tail:
                        fail("f: PTMI_OPT_STREAM_TAIL reads back %d" % c.get_option(B.OPT_STREAM_TAIL))
                if c.render_blocks(pkg.STREAMS):
                    fail("f: the stream form without GLASS says it blocks")
                a.write(start)
                name = "f %s %s" % ("automatic tail" if tail is None else "tail 950", kind)
                render_and_compare(c, a, [(cam, 8, 2, pkg.STREAMS)] * 4, wants, name)
            ok(name)
    # g: the stream form with GLASS: float atomics through plane_at's byte offsets
    w, h = 64, 48
    start = initial_planes(ora, w, h)
    want = ora.render_streams_tree(glass[0], glass[1], cam, w, h, CAP, 2, start, n_threads=THREADS)[0]
    c, a = bound(glass, w, h, "ODD")
    with c:
        c.set_option(B.OPT_STREAMS_FORM, B.FORM_STREAM)
        a.write(start)
        render_and_compare(c, a, [(cam, 15, 2, pkg.STREAMS)], [want], "g stream form ODD", compare=glass_rule)
        if c.stats()["stream_rays_dropped"] != 0:
            fail("g: rays were dropped")
    ok("g stream form ODD")
    # ... and a call that is REDONE: the colour planes copied aside and put back (StreamCall::copy_colour).  The overflow streams never hold
    # fewer slots than the waves' static blocks (393 472), so only an image of more pixels than that can drop children at one ray per
    # pixel: 800 x 600 at 4 spp, the size tests/test_gpu_wavefront.py forces the redo at -- 64 x 48 cannot take this route
    w, h, spp = 800, 600, 4
    start = initial_planes(ora, w, h)
    want = ora.render_streams_tree(glass[0], glass[1], cam, w, h, CAP, spp, start, n_threads=THREADS)[0]
    lib = B.open_library(tiny_rings)
    c, a = bound(glass, w, h, "ODD", library=lib)
    with c:
        c.set_option(B.OPT_STREAMS_FORM, B.FORM_STREAM)
        c.set_option(B.OPT_STREAM_CAPACITY, 1)
        a.write(start)
        render_and_compare(c, a, [(cam, 15, spp, pkg.STREAMS)], [want], "g redone call ODD", compare=glass_rule)
        grown, st = c.get_option(B.OPT_STREAM_CAPACITY), c.stats()
        print("   g redone call: capacity 1 -> %d rays per pixel, %d rays spilled, %d dropped" % (grown, st["stream_rays_spilled"], st["stream_rays_dropped"]), flush=True)
        if not grown > 1:
            fail("g: one ray per pixel held every child of a tiny-ring build: the call was not redone")
        if st["stream_rays_dropped"] != 0:
            fail("g: the redone call still dropped %d rays" % st["stream_rays_dropped"])
    ok("g redone call ODD")


# ---- group scenes: rows h, i ------------------------------------------------------------------------------------------------------------
def group_scenes():
    import mesh_rays
    w, h = 72, 40
    start = initial_planes(ora, w, h)
    field, glass_field = W.sphere_field(2000, seed=21), W.sphere_field(2000, seed=22, glass_fraction=0.1)
    wants = {"inline": ora.render_inline(field[0], field[1], cam, w, h, 8, 2, start, n_threads=THREADS)[0],
             "streams": ora.render_streams(field[0], field[1], cam, w, h, CAP, 2, start, n_threads=THREADS)[0],
             "tree walk": ora.render_streams_tree(glass_field[0], glass_field[1], cam, w, h, CAP, 2, start, n_threads=THREADS)[0]}
    for kind in KINDS3:
        for alg in ("inline", "streams", "tree walk"):
            c, a = bound(glass_field if alg == "tree walk" else field, w, h, kind, set_scene="set_scene_bvh")
            with c:
                a.write(start)
                name = "h %s %s" % (alg, kind)
                render_and_compare(c, a, [(cam, 8, 2, pkg.INLINE if alg == "inline" else pkg.STREAMS)], [wants[alg]], name)
            ok(name)
    # i: a mesh scene against a twin context with owned planes (the mesh oracle is a library of its own: not cheap to bring here)
    room = mesh_rays.closed_room(1)
    w, h = 67, 45
    start = initial_planes(ora, w, h)
    moved = W.triangle_vertices(room[1]) + np.array([0.2, 0.1, -0.3], np.float32)
    c, a = bound(room, w, h, "ODD", set_scene="set_scene_mesh")
    with c, pkg.Context(0) as twin:
        twin.set_scene_mesh(*room)
        twin.resize(w, h)
        images = []
        for when in ("as set", "after update_mesh_vertices"):
            if when != "as set":
                c.update_mesh_vertices(moved)
                twin.update_mesh_vertices(moved)
            for alg in ("inline", "streams"):
                algorithm = pkg.INLINE if alg == "inline" else pkg.STREAMS
                twin.upload_state(*start)
                twin.render(cam, 8, 2, algorithm)
                want = twin.download_state()
                a.write(start)
                name = "i %s %s" % (alg, when)
                render_and_compare(c, a, [(cam, 8, 2, algorithm)], [want], name)
                images.append(np.asarray(want[0]).copy())
                ok(name)
        if not np.any(images[0] != 0) or np.array_equal(images[0], images[2]):
            fail("i: the room is dark, or moving its vertices changed nothing: the twin comparison says little")


# ---- group helpers: the helper entries on bound planes, the lifecycle ------------------------------------------------------------------
def expect_error(code, call, what):
    try:
        call()
    except B.PtmiError as e:
        if e.code != code:
            fail("%s: error %d, expected %d (%s)" % (what, e.code, code, e))
        return
    fail("%s: accepted" % what)


def snapshot(c, dst_ptr, stream):
    c._check(c._lib.ptmi_snapshot_color(c._h, B._vp(dst_ptr), B._vp(stream) if stream else None))


def group_helpers():
    sp, pl = W.scene16()
    rng = np.random.default_rng(5)
    for kind in KINDS2:
        # init_output / reseed / create_with
        w, h = 70, 33
        n = w * h
        c, a = bound((sp, pl), w, h, kind)
        with c:
            c.init_output(0xABCDEF0123)
            c.synchronize()
            a.check("init_output")
            zero = [np.zeros(n, np.float32)] * 3
            exact(a.read(), zero + list(ora.gen_seeds(0xABCDEF0123, 0, n)), "init_output %s" % kind)
            colour = [rng.random(n, dtype=np.float32) for _ in range(3)]
            a.write(colour + [np.full(n, SENTINEL, np.uint32)] * 4)
            c.reseed(77)
            c.synchronize()
            a.check("reseed")
            exact(a.read(), colour + list(ora.gen_seeds(77, 0, n)), "reseed keeps the colours, %s" % kind)
            words = [rng.integers(0, 2 ** 32, n, dtype=np.uint32) for _ in range(3)]
            c.create_with(*words)
            a.check("create_with")
            got = a.read()
            exact(got[:3], colour, "create_with keeps the colours, %s" % kind)
            for i in (0, 1, 1234, n - 1):
                if tuple(int(p[i]) for p in got[3:]) != ora.sfc32_seed3(words[0][i], words[1][i], words[2][i]):
                    fail("create_with %s: element %d" % (kind, i))
        ok("init_output reseed create_with %s" % kind)
        # ... for a part of a partition: seeds from the GLOBAL rows
        w, h = 61, 23
        c, a = bound((sp, pl), w, h, kind, partition=(4, 3, 1))
        with c:
            rows = c.global_rows()
            c.init_output(SEED0)
            c.synchronize()
            a.check("init_output of a part")
            exact(a.read(), initial_rows(ora, w, rows), "init_output of part 1 of 3, %s" % kind)
            colour = [rng.random(len(rows) * w, dtype=np.float32) for _ in range(3)]
            a.write(colour + [np.zeros(len(rows) * w, np.uint32)] * 4)
            c.reseed(78)
            c.synchronize()
            a.check("reseed of a part")
            exact(a.read(), colour + initial_rows(ora, w, rows, 78)[3:], "reseed of part 1 of 3, %s" % kind)
        ok("partition seeds %s" % kind)
        # upload_state / download_state are exact copies, also with some planes left out
        w, h = 61, 7
        n = w * h
        c, a = bound((sp, pl), w, h, kind)
        with c:
            state = [rng.random(n, dtype=np.float32) for _ in range(3)] + [rng.integers(0, 2 ** 32, n, dtype=np.uint32) for _ in range(4)]
            c.upload_state(*state)
            a.check("upload_state")
            exact(a.read(), state, "upload_state then a torch read, %s" % kind)
            other = [rng.random(n, dtype=np.float32) for _ in range(3)] + [rng.integers(0, 2 ** 32, n, dtype=np.uint32) for _ in range(4)]
            c.upload_state(r=other[0], sb=other[4], sctr=other[6])
            a.check("upload_state of three planes")
            mixed = [other[0], state[1], state[2], state[3], other[4], state[5], other[6]]
            exact(a.read(), mixed, "upload_state of r, sb, sctr alone, %s" % kind)
            a.write(other)
            exact(c.download_state(), other, "a torch write then download_state, %s" % kind)
            exact(list(c.download_color()) + other[3:], other, "download_color, %s" % kind)
            a.check("download_state")
        ok("upload download %s" % kind)
    # present: ODD sends every lane through the scalar path, ALIGNED through the wide path with the scalar tail
    for kind in KINDS2:
        for (w, h) in PRESENT_SIZES:
            n = w * h
            c, a = bound((sp, pl), w, h, kind)
            with c:
                for iters in PRESENT_ITERATIONS:
                    r, g, b = cp.present_inputs(n, iters)
                    a.write([r, g, b] + [np.zeros(n, np.uint32)] * 4)
                    want_rgb, want_rgba = cp.present_reference(r, g, b, iters)
                    for rgb32f, rgba8 in ((True, True), (True, False), (False, True)):
                        what = "present %dx%d %s, %d iterations, outputs %s%s" % (w, h, kind, iters, "rgb " if rgb32f else "", "rgba" if rgba8 else "")
                        rgb, rgba = c.present(iters, rgb32f=rgb32f, rgba8=rgba8)
                        if (rgb is None) != (not rgb32f) or (rgba is None) != (not rgba8):
                            fail(what + ": wrong outputs returned")
                        if rgb is not None:
                            x, y = rgb.reshape(-1).view(np.uint32), want_rgb.reshape(-1).view(np.uint32)
                            if not np.array_equal(x, y):
                                bad = np.flatnonzero(x != y)
                                fail("%s: %d rgb words differ, first at pixel %d channel %d: %#x, expected %#x (input %r)"
                                     % (what, bad.size, bad[0] // 3, bad[0] % 3, x[bad[0]], y[bad[0]], (r, g, b)[bad[0] % 3][bad[0] // 3]))
                        if rgba is not None and not np.array_equal(rgba.reshape(-1, 4), want_rgba):
                            bad = np.flatnonzero(np.any(rgba.reshape(-1, 4) != want_rgba, axis=1))
                            fail("%s: %d rgba pixels differ, first at pixel %d: %r, expected %r (inputs %r %r %r)"
                                 % (what, bad.size, bad[0], rgba.reshape(-1, 4)[bad[0]].tolist(), want_rgba[bad[0]].tolist(), r[bad[0]], g[bad[0]], b[bad[0]]))
                        a.check(what)
            ok("present %dx%d %s" % (w, h, kind))
    # snapshot_color into a torch tensor with guards of its own
    w, h = 97, 61
    n = w * h
    start = initial_planes(ora, w, h)
    want, _ = ora.render_inline(sp, pl, cam, w, h, 8, 2, start, n_threads=THREADS)
    for kind in KINDS2:
        c, a = bound((sp, pl), w, h, kind)
        with c:
            lay = cp.arena_layout(3 * n, w, (1,) if kind == "ODD" else (0,))
            buf = torch.empty(lay.total, dtype=torch.int32, device="cuda")
            o = lay.offsets(buf.data_ptr())[0]
            dst = buf[o:o + 3 * n]
            side = torch.cuda.Stream()

            def taken(what, expected):
                got = dst.cpu().numpy().view(np.float32).reshape(3, n)
                exact(list(got) + list(expected[3:]), expected, "snapshot_color %s, %s" % (kind, what))
                bad = cp.guards_intact(buf, lay)
                if bad.size:
                    fail("snapshot_color %s, %s: %d guard elements of the destination were written, first %d" % (kind, what, bad.size, bad[0]))
                dst.fill_(SENTINEL)
                torch.cuda.synchronize()
            cp.fill_guards(buf, lay)
            dst.fill_(SENTINEL)
            a.write(start)
            colour = [rng.random(n, dtype=np.float32) for _ in range(3)]
            a.write(colour + list(start[3:]))
            snapshot(c, dst.data_ptr(), None)
            c.synchronize()
            taken("on the context's stream", colour + list(start[3:]))
            snapshot(c, dst.data_ptr(), side.cuda_stream)
            side.synchronize()
            taken("on a second torch stream", colour + list(start[3:]))
            a.write(start)
            c.render(cam, 8, 2, pkg.INLINE)                     # only enqueued ...
            snapshot(c, dst.data_ptr(), side.cuda_stream)       # ... the copy on the other stream is ordered behind it
            side.synchronize()
            taken("after a render that was only enqueued", want)
            c.synchronize()
            a.check("snapshot_color")
        ok("snapshot_color %s" % kind)
    for kind in KINDS2:
        c, a = bound((sp, pl), 9, 2, kind)
        with c:
            owned_before = None
            if c.device_planes() != a.ptrs:
                fail("device_planes while bound")
            c.unbind()
            owned = c.device_planes()
            if set(owned) & set(a.ptrs) or len(set(owned)) != 7 or any(p % 256 for p in owned):
                fail("device_planes after unbind: %r" % (owned,))
            a.bind(c)
            c.unbind()
            if c.device_planes() != owned:
                fail("the owned planes moved: %r then %r" % (owned, c.device_planes()))
            del owned_before
        ok("device_planes %s" % kind)
    lifecycle()


def lifecycle():
    sp, pl = W.scene16()
    w, h = 64, 48
    n = w * h
    start = initial_planes(ora, w, h)
    start_b = initial_planes(ora, w, h, 99)

    def inline(planes, spp, camera=None):
        return ora.render_inline(sp, pl, cam if camera is None else camera, w, h, 8, spp, planes, n_threads=THREADS)[0]
    with pkg.Context(0) as c:
        c.set_scene(sp, pl)
        c.resize(w, h)
        c.init_output(SEED0)
        c.render(cam, 8, 2, pkg.INLINE)
        owned = c.download_state()
        exact(owned, inline(start, 2), "owned planes before binding")
        a = Arena(n, w, "ODD")
        a.bind(c)
        c.init_output(99)
        c.render(cam, 8, 1, pkg.INLINE)
        c.synchronize()
        a.check("bind, init_output, render")
        in_a = a.read()
        exact(in_a, inline(start_b, 1), "bind, init_output, render")
        c.unbind()
        exact(c.download_state(), owned, "unbind: the owned planes are what was downloaded")
        c.render(cam, 8, 1, pkg.INLINE)
        exact(c.download_state(), inline(owned, 1), "after unbind the render continues from the owned planes")
        a.check("after unbind")
        exact(a.read(), in_a, "after unbind the arena no longer changes")
        ok("lifecycle unbind")
        # bind A, render; bind B, render: A is unchanged, B holds its own start state and the render
        a.bind(c)
        c.render(cam, 8, 1, pkg.INLINE)
        c.synchronize()
        in_a = a.read()
        exact(in_a, inline(start_b, 2), "arena A, second render")
        b = Arena(n, w, "ALIGNED")
        b.write(start)
        b.bind(c)
        c.render(cam2, 8, 2, pkg.INLINE)
        c.synchronize()
        a.check("arena A after binding B")
        b.check("arena B")
        exact(a.read(), in_a, "arena A after a render into arena B")
        in_b = inline(start, 2, cam2)
        exact(b.read(), in_b, "arena B: its own start state and the render")
        ok("lifecycle rebind")
        # one NULL among seven: PTMI_EINVAL, and the earlier binding still renders
        for k in (0, 3, 6):
            some = list(a.ptrs)
            some[k] = None
            expect_error(B.PTMI_EINVAL, lambda: c.bind_planes(some), "a bind with plane %d NULL" % k)
        if c.device_planes() != b.ptrs:
            fail("a refused bind changed the binding")
        c.render(cam2, 8, 1, pkg.INLINE)
        c.synchronize()
        in_b = inline(in_b, 1, cam2)
        exact(b.read(), in_b, "the earlier binding after a refused bind")
        exact(a.read(), in_a, "arena A after a refused bind of its planes")
        ok("lifecycle partial bind")
        with pkg.Context(0) as fresh:
            fresh.set_scene(sp, pl)
            expect_error(B.PTMI_ESTATE, lambda: fresh.bind_planes(a.ptrs), "a bind before resize")
            expect_error(B.PTMI_ESTATE, fresh.device_planes, "get_planes before resize")
        ok("lifecycle bind before resize")
        # resize while bound (to a SMALLER image: were the binding kept, its writes would still lie inside the arena and show)
        w2, h2 = 61, 23
        c.resize(w2, h2)
        now = c.device_planes()
        if set(now) & set(b.ptrs) or set(now) & set(a.ptrs):
            fail("resize kept a binding: %r" % (now,))
        z = c.download_state()
        if any(np.any(np.asarray(p).view(np.uint32) != 0) for p in z):
            fail("the owned planes after a resize are not zeroed")
        start2 = initial_planes(ora, w2, h2)
        c.init_output(SEED0)
        c.render(cam, 8, 2, pkg.INLINE)
        exact(c.download_state(), ora.render_inline(sp, pl, cam, w2, h2, 8, 2, start2)[0], "render after a resize while bound")
        a.check("arena A after resize")
        b.check("arena B after resize")
        exact(b.read(), in_b, "arena B after a resize")
        exact(a.read(), in_a, "arena A after a resize")
        ok("lifecycle resize while bound")


# ---- group stream: the caller's stream, bench.py's configuration -----------------------------------------------------------------------
def group_stream():
    """What this shows: work of ptmi_render launched on a WRONG stream (the context's own, the NULL stream) starts while the filler
    still runs on the caller's stream, reads the sentinel instead of the start planes that step 2 writes behind the filler, and fails
    reliably -- the filler lasts ten times the host time of steps 2 and 3.  A render that is not finished when step 4 clones, or a clone
    that is overtaken by step 5, fails the same way.  What it cannot show reliably: a MISSING JOIN of the tail's side stream -- the
    tail's pixels are then simply late, and whether the clone sees them depends on timing; such a defect may pass by luck."""
    sp, pl = W.scene16()
    cases = (("inline 97x61", 97, 61, pkg.INLINE, False), ("streams 72x40", 72, 40, pkg.STREAMS, False),
             ("stream form tail 128x64", 128, 64, pkg.STREAMS, True))
    big = torch.ones(1 << 24, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for name, w, h, algorithm, stream_form in cases:
        n = w * h
        start = initial_planes(ora, w, h)
        launches = 4 if stream_form else 1                   # (the tail runs from the third launch with one key on)
        wants, cur = [], start
        for _ in range(launches):
            if algorithm == pkg.INLINE:
                cur, _ = ora.render_inline(sp, pl, cam, w, h, 8, 2, cur, n_threads=THREADS)
            else:
                cur, _ = ora.render_streams(sp, pl, cam, w, h, CAP, 2, cur, n_threads=THREADS)
            wants.append(cur)
        start_dev = torch.from_numpy(np.stack([np.ascontiguousarray(p).reshape(-1).view(np.int32) for p in start])).to("cuda")
        main, second = torch.cuda.Stream(), torch.cuda.Stream()
        for how in ("torch stream", "own stream", "second torch stream"):
            c, a = bound((sp, pl), w, h, "ODD")
            with c:
                if stream_form:
                    c.set_option(B.OPT_STREAMS_FORM, B.FORM_STREAM)
                    c.set_option(B.OPT_STREAM_TAIL, 950)
                if c.render_blocks(algorithm):
                    fail("%s: render_blocks is 1" % name)
                if how == "own stream":
                    c.set_stream(main.cuda_stream)
                    c.set_stream(None)
                    a.write(start)
                    for k in range(launches):
                        c.render(cam, 8, 2, algorithm)
                        c.synchronize()
                        exact(a.read(), wants[k], "%s, the context's own stream, launch %d" % (name, k))
                    a.check(name)
                    ok("caller stream %s %s" % (name, how))
                    continue
                stream = main
                c.set_stream(main.cuda_stream)
                if how == "second torch stream":                # a switch: set_stream waits for the old stream
                    a.write(start)
                    c.render(cam, 8, 2, algorithm)
                    c.set_stream(second.cuda_stream)
                    exact(a.read(), wants[0], "%s: set_stream waited for the old stream" % name)
                    stream = second
                with torch.cuda.stream(stream):
                    def steps_2_and_3():
                        for v, s in zip(a.views, start_dev):
                            v.copy_(s, non_blocking=True)
                        c.render(cam, 8, 2, algorithm)
                    # the warm-up pass (allocations, code objects), timed on the host; the stream form's launches 2 to 4 behind it, so that
                    # the order and the tail's boundary stand and the launch under test -- the fifth with this key -- runs the tail
                    t0 = time.perf_counter()
                    steps_2_and_3()
                    host_s = time.perf_counter() - t0
                    for _ in range(launches - 1):
                        c.render(cam, 8, 2, algorithm)
                    stream.synchronize()
                    exact(a.read(), wants[-1], "%s, %s: the warm-up pass" % (name, how))
                    t0 = time.perf_counter()
                    steps_2_and_3()
                    host_s = max(host_s, time.perf_counter() - t0)
                    stream.synchronize()
                    big.mul_(1.0000001).add_(1e-9)                               # (the filler's kernels are loaded before they are timed)
                    stream.synchronize()
                    reps, filler_s = 4, 0.0
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    while True:
                        e0.record()
                        for _ in range(reps):
                            big.mul_(1.0000001).add_(1e-9)
                        e1.record()
                        stream.synchronize()
                        filler_s = e0.elapsed_time(e1) * 1e-3
                        if filler_s >= 10.0 * host_s or reps >= 1 << 12:
                            break
                        reps *= 2
                    print("   %s, %s: steps 2 and 3 take %.3f ms on the host, the filler (%d passes over 64 MB) %.3f ms on the device"
                          % (name, how, host_s * 1e3, reps, filler_s * 1e3), flush=True)
                    if filler_s < 10.0 * host_s:
                        fail("the filler cannot be made ten times as long as the host time of steps 2 and 3")
                    a.fill(SENTINEL)
                    stream.synchronize()
                    for _ in range(reps):                                        # 1 filler
                        big.mul_(1.0000001).add_(1e-9)
                    steps_2_and_3()                                              # 2 the start planes from a device tensor, 3 the render
                    clones = [v.clone() for v in a.views]                        # 4
                    a.fill(SENTINEL)                                             # 5
                    stream.synchronize()
                host = [t.cpu().numpy() for t in clones]
                got = [x.view(np.float32) for x in host[:3]] + [x.view(np.uint32) for x in host[3:]]
                exact(got, wants[0], "%s, %s: the clones taken behind the render" % (name, how))
                left = a.read()
                if any(np.any(p.view(np.uint32) != SENTINEL) for p in left):
                    fail("%s, %s: something wrote the arena after step 5" % (name, how))
                a.check("%s, %s" % (name, how))
                c.set_stream(None)
            ok("caller stream %s %s" % (name, how))
    bench_configuration()


def bench_configuration():
    """bench.py's order of calls at a reduced size: torch first (setup), Context, set_scene, set_partition, resize, bind_torch, a side
    stream, set_stream, init_output; three renders; the part's rows are the oracle's rows of the whole image"""
    sp, pl = W.scene16()
    w, h, spp, stripe = 160, 90, 4, 5
    c = pkg.Context(0)
    with c:
        c.set_scene(sp, pl)
        c.set_partition(stripe, 2, 0)
        c.resize(w, h)
        color = torch.zeros((3, c.local_rows, w), dtype=torch.float32, device="cuda")
        state = torch.zeros((4, c.local_rows, w), dtype=torch.int32, device="cuda")
        c.bind_torch(color, state)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        torch.cuda.set_stream(stream)
        c.set_stream(stream.cuda_stream)
        c.set_variant(0)
        c.init_output(SEED0)
        for _ in range(3):
            c.render(cam, 8, spp, pkg.INLINE)
        torch.cuda.synchronize()
        rows = c.global_rows()
        want = initial_planes(ora, w, h)
        for _ in range(3):
            want, _ = ora.render_inline(sp, pl, cam, w, h, 8, spp, want, n_threads=THREADS)
        got = list(color.cpu().numpy()) + list(state.cpu().numpy().view(np.uint32))
        exact(got, [np.asarray(p)[rows] for p in want], "bench.py's configuration, part 0 of 2")
        if len(rows) != 45:
            fail("part 0 of 2 holds %d rows" % len(rows))
        c.set_stream(None)
    ok("bench configuration")


GROUPS = {"inline": group_inline, "streams": group_streams, "scenes": group_scenes, "helpers": group_helpers, "stream": group_stream}


def main(argv):
    group = argv[1]
    setup(group)
    if group == "streams":
        group_streams(argv[2])
    else:
        GROUPS[group]()
    if _count != len(CASES[group]):
        raise SystemExit("%d cases ran, %d are listed" % (_count, len(CASES[group])))
    print("CALLER_PLANES_OK %d" % _count, flush=True)


if __name__ == "__main__":
    main(sys.argv)
