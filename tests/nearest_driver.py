"""Child program of tests/test_gpu_nearest.py (not a test module): `python tests/nearest_driver.py WORKDIR`.

The nearest-primitive query -- ptmi_nearest_device and its indexed form through Context.nearest -- as a PyTorch caller uses it: device
tensors in, device tensors out, on the context's stream, in a process where torch brings the HIP runtime up before the library is loaded.
The scenes are the five kinds of tests/ray_query_driver.py (its KINDS, imported; nearest_points.driver_scene makes them by its
constructors) with 4 096 points each (nearest_points.points: inside the box, on surfaces, at centres, on edges and vertices, far away,
beyond 2^40, non-finite); the reference is the host twin (binding.nearest -> ptmi_nearest), BIT FOR BIT in dist, idx and point.  Before any
device call the twin alone must show, per scene kind, that the comparison is not vacuous.  One line per case, `ok <case>` or
`FAILED <case>: <why>`; a failed comparison does not end the process, a runtime error does; the last line is NEAREST_DONE."""
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

CASES = ["1 the host twin", "2 sizes alignment guards", "3 indexed", "4 caller stream", "5 after device updates", "6 refusals", "7 render between queries",
         "8 non-finite scene data"]
SIZES = (0, 1, 63, 64, 65, 257, 4096)
GUARD = 64
SENTINEL = 0x7FC0DEAD

torch = pkg = B = W = N = mesh_rays = KINDS = None
SCENES = {}


def setup():
    global torch, pkg, B, W, N, mesh_rays, KINDS
    import torch as _torch
    torch = _torch
    torch.zeros(1, device="cuda")                      # torch brings the runtime up first
    torch.cuda.synchronize()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg._build.build_lib()
    B, W = pkg.binding, pkg.world
    import mesh_rays as _m
    import nearest_points as _N
    from ray_query_driver import KINDS as _kinds
    N, mesh_rays, KINDS = _N, _m, list(_kinds)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.cpu().numpy()


def nearest(c, points, **kw):
    """Context.nearest on the context's OWN stream from torch's, with host waits on either side"""
    torch.cuda.synchronize()
    out = c.nearest(points, point=True, **kw)
    c.synchronize()
    return tuple(host(x) for x in out)


def assert_same(got, want, what, rows=None):
    """dist, idx and point against the twin's, bit for bit; nothing reported is a NaN or an inf"""
    if rows is not None:
        want = tuple(w[rows] for w in want)
    bad = N.same_bits(got, want)
    assert bad.size == 0, "%s: %d points differ, e.g. point %d: device %r %r %r, twin %r %r %r" % (
        what, bad.size, bad[0], got[0][bad[0]], got[1][bad[0]], got[2][bad[0]], want[0][bad[0]], want[1][bad[0]], want[2][bad[0]])
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all(), what + ": a reported word is not finite"


class Scene:
    def __init__(self, kind):
        self.kind = kind
        self.spheres, self.triangles, self.planes, self.points = N.driver_scene(kind)
        self.n = len(self.points)
        self.want = self.twin(self.points, None)
        self.r_max = N.aimed_r_max(self.want[0], self.want[1])
        self.want_aimed = self.twin(self.points, self.r_max)
        # BEFORE any device call: answers of every primitive kind, negative distances, moved answers, points the walk does not serve
        idx, ns, npl = self.want[1], len(self.spheres), len(self.planes)
        served = N.served_by(kind, self.points)
        self.figures = (kind, int((idx >= 0).sum()), int(((idx >= 0) & (idx < ns)).sum()), int(((idx >= ns) & (idx < ns + npl)).sum()), int((idx >= ns + npl).sum()),
                        int((self.want[0] < 0).sum()), int((self.want_aimed[1] != idx).sum()), int((~served).sum()))
        assert self.figures[1] >= 3500 and self.figures[2] >= 200 and self.figures[5] >= 100 and self.figures[6] >= 400, self.figures
        if kind == "mesh":
            assert self.figures[4] >= 1000, self.figures
        if kind in ("bvh", "mesh"):
            assert self.figures[7] >= 8, self.figures
        self.d_points, self.d_r_max = dev(self.points), dev(self.r_max)
        torch.cuda.synchronize()
        self.ctx = pkg.Context(0)
        self.set(self.ctx)

    def twin(self, points, r_max, spheres=None, triangles=None):
        return B.nearest(self.spheres if spheres is None else spheres, self.planes, self.triangles if triangles is None else triangles, points, r_max, point=True)

    def set(self, c):
        if self.kind == "mesh":
            c.set_scene_mesh(self.spheres, self.triangles, self.planes)
        elif self.kind == "bvh":
            c.set_scene_bvh(self.spheres, self.planes)
        else:
            c.set_scene(self.spheres, self.planes)


def case_twin():
    """1: dist, idx and point are the host twin's, bit for bit, on every scene kind, without r_max and with r_max aimed at the winner's key;
    without the locations (point NULL) dist and idx are the same"""
    for kind in KINDS:
        sc = SCENES[kind]
        assert_same(nearest(sc.ctx, sc.d_points), sc.want, "%s, no r_max" % kind)
        assert_same(nearest(sc.ctx, sc.d_points, r_max=sc.d_r_max), sc.want_aimed, "%s, aimed r_max" % kind)
        torch.cuda.synchronize()
        d, i = sc.ctx.nearest(sc.d_points, r_max=sc.d_r_max)
        sc.ctx.synchronize()
        assert np.array_equal(host(d).view(np.uint32), sc.want_aimed[0].view(np.uint32)) and np.array_equal(host(i), sc.want_aimed[1]), "%s without locations" % kind


def guarded(n, words, dtype, off):
    """n x words elements between two guards -> (the whole buffer, the view, its first word); off: the view starts 4 bytes off a 16-byte boundary"""
    buf = torch.full((2 * GUARD + n * words + 4,), SENTINEL, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    start = GUARD + (1 if off else 0)
    view = buf[start:start + n * words].view(dtype)
    assert n == 0 or view.data_ptr() % 16 == (4 if off else 0)
    return buf, (view.view(n, words) if words > 1 else view), start


def guards_intact(buf, start, length, what):
    h = host(buf).view(np.uint32)
    assert (h[:start] == SENTINEL).all() and (h[start + length:] == SENTINEL).all(), "%s: a guard word was written" % what


def case_sizes():
    """2: wave and block tails; every array 16-byte aligned and 4 bytes off; 64 guard words on either side of every output"""
    for kind in KINDS:
        sc = SCENES[kind]
        for n in SIZES:
            for off in ((False, False, False), (True, True, True), (False, True, False), (True, False, True)):
                what = "%s, n = %d, arrays off by %r" % (kind, n, off)
                _, pts, _ = guarded(n, 3, torch.float32, off[0])
                pts.copy_(sc.d_points[:n])
                _, rm, _ = guarded(n, 1, torch.float32, off[2])
                rm.copy_(sc.d_r_max[:n])
                outs = [guarded(n, 1, torch.float32, off[1]), guarded(n, 1, torch.int32, off[2]), guarded(n, 3, torch.float32, off[0])]
                torch.cuda.synchronize()
                sc.ctx.nearest(pts, r_max=rm, out=tuple(o[1] for o in outs))
                sc.ctx.synchronize()
                for (buf, view, start), words in zip(outs, (1, 1, 3)):
                    guards_intact(buf, start, n * words, what)
                if n:
                    assert_same(tuple(host(o[1]) for o in outs), sc.want_aimed, what, rows=slice(0, n))


def case_indexed():
    """3: through ray_order's order over the rays [p, 0 0 1], through a list with m < n, and with entries outside [0, n): the words are the
    plain entry's, unnamed rows stay untouched"""
    for kind in KINDS:
        sc = SCENES[kind]
        rays = np.concatenate([sc.points, np.tile(np.array([0, 0, 1], np.float32), (sc.n, 1))], axis=1)
        torch.cuda.synchronize()
        order = sc.ctx.ray_order(dev(rays))
        sc.ctx.synchronize()
        assert np.array_equal(np.sort(host(order)), np.arange(sc.n))
        assert_same(nearest(sc.ctx, sc.d_points, index=order), sc.want, "%s, ray_order's order" % kind)
        rng = np.random.default_rng(9)
        live = np.sort(rng.choice(sc.n, sc.n // 3, replace=False)).astype(np.int32)
        index = np.concatenate([live[:500], [-1, sc.n, sc.n + 7, -2 ** 31, 2 ** 31 - 1], live[500:]]).astype(np.int32)
        rng.shuffle(index)
        outs = (torch.full((sc.n,), 7.5, dtype=torch.float32, device="cuda"), torch.full((sc.n,), 77, dtype=torch.int32, device="cuda"),
                torch.full((sc.n, 3), -7.5, dtype=torch.float32, device="cuda"))
        got = nearest(sc.ctx, sc.d_points, r_max=sc.d_r_max, index=dev(index), out=outs)
        named = np.zeros(sc.n, bool)
        named[live] = True
        assert_same(tuple(g[named] for g in got), sc.want_aimed, "%s, a list with m < n" % kind, rows=named)
        assert (got[0][~named] == 7.5).all() and (got[1][~named] == 77).all() and (got[2][~named] == -7.5).all(), "%s: an unnamed row was written" % kind
        fresh = nearest(sc.ctx, sc.d_points, index=dev(live))                          # allocated by the binding: the miss record first
        assert (fresh[0][~named].view(np.uint32) == 0).all() and (fresh[1][~named] == -1).all() and (fresh[2][~named].view(np.uint32) == 0).all(), kind


def case_caller_stream():
    """4: on torch's non-default stream through set_stream; the inputs are written on that stream behind a filler, the results are read
    after that stream alone is synchronised"""
    stream = torch.cuda.Stream()
    filler = torch.ones((2048, 2048), device="cuda")
    for kind in ("s16", "bvh", "mesh"):
        sc = SCENES[kind]
        pts, rm = torch.zeros_like(sc.d_points), torch.zeros_like(sc.d_r_max)
        torch.cuda.synchronize()
        sc.ctx.set_stream(stream.cuda_stream)
        try:
            with torch.cuda.stream(stream):
                x = filler
                for _ in range(20):
                    x = x @ filler * 1e-3
                pts.copy_(sc.d_points)
                rm.copy_(sc.d_r_max)
                a = sc.ctx.nearest(pts, r_max=rm, point=True)
                b = sc.ctx.nearest(pts, point=True)
            stream.synchronize()
            assert_same(tuple(host(v) for v in a), sc.want_aimed, "%s on the caller's stream, aimed r_max" % kind)
            assert_same(tuple(host(v) for v in b), sc.want, "%s on the caller's stream" % kind)
            assert float(x.sum()) == float(x.sum())
        finally:
            torch.cuda.synchronize()
            sc.ctx.set_stream(None)


def case_after_updates():
    """5: after update_spheres, set_bvh_spheres, update_mesh_vertices (a shift, then one that collapses kept triangles to zero area) and
    set_mesh_triangles from device tensors, a query enqueued at once answers for the new scene: it equals a context set afresh, and the
    twin of the new scene"""
    def held(what, c, fresh, sc, spheres=None, triangles=None):
        got = c.nearest(sc.d_points, point=True)         # at once: ordered behind the update by the stream alone
        c.synchronize()
        got = tuple(host(x) for x in got)
        assert_same(got, nearest(fresh, sc.d_points), what + ", against a context set afresh")
        assert_same(got, sc.twin(sc.points, None, spheres, triangles), what + ", against the twin")
        assert N.same_bits(got, sc.want).size > 100, what + ": the update changed nothing"

    sc = SCENES["bvh"]
    g = W.displaced_spheres(W.sphere_geometry(sc.spheres), 0.5, "wave", seed=2)
    moved = W.with_sphere_geometry(sc.spheres, g)
    other = np.ascontiguousarray(moved[::2].copy(), B.SPHERE_DTYPE)
    d_g, d_other = dev(np.ascontiguousarray(g, np.float32)), dev(other.view(np.float32).reshape(-1, 10).copy())
    torch.cuda.synchronize()
    with pkg.Context(0) as c, pkg.Context(0) as fresh:
        c.set_scene_bvh(sc.spheres, sc.planes)
        c.update_spheres(d_g)
        fresh.set_scene_bvh(moved, sc.planes)
        held("after update_spheres", c, fresh, sc, spheres=moved)
        c.set_bvh_spheres(d_other)
        fresh.set_scene_bvh(other, sc.planes)
        held("after set_bvh_spheres", c, fresh, sc, spheres=other)
    sc = SCENES["mesh"]
    shifted = sc.triangles.copy()
    for k in ("v0", "v1", "v2"):
        shifted[k] = shifted[k] + np.array([0.75, -0.5, 1.25], np.float32)
    d_v = dev(np.stack([shifted["v0"], shifted["v1"], shifted["v2"]], axis=1).astype(np.float32))
    t2 = np.ascontiguousarray(mesh_rays.adversarial_scene(1, seed=4)[1], B.TRIANGLE_DTYPE)
    d_t2 = dev(t2.view(np.float32).reshape(-1, 15).copy())
    torch.cuda.synchronize()
    with pkg.Context(0) as c, pkg.Context(0) as fresh:
        sc.set(c)
        c.update_mesh_vertices(d_v)
        fresh.set_scene_mesh(sc.spheres, shifted, sc.planes)
        held("after update_mesh_vertices", c, fresh, sc, triangles=shifted)
        # some kept triangles collapse to zero area: they stay in their leaves with a NaN normal and are no candidates any more, as in a
        # context set afresh, where they are in no leaf (the six most often the answer, so that the points at them see it)
        first = len(sc.spheres) + len(sc.planes)
        before = sc.twin(sc.points, None, triangles=shifted)[1] - first
        collapsed = np.argsort(-np.bincount(before[before >= 0], minlength=len(shifted)), kind="stable")[:6]
        assert np.isin(before, collapsed).sum() >= 200
        flat = shifted.copy()
        flat["v2"][collapsed] = flat["v1"][collapsed]
        c.update_mesh_vertices(dev(np.stack([flat["v0"], flat["v1"], flat["v2"]], axis=1).astype(np.float32)))
        fresh.set_scene_mesh(sc.spheres, flat, sc.planes)
        held("after update_mesh_vertices collapsing six triangles", c, fresh, sc, triangles=flat)
        got = c.nearest(sc.d_points)
        c.synchronize()
        assert not np.isin(host(got[1]) - first, collapsed).any(), "a triangle of zero area was reported"
        c.set_mesh_triangles(d_t2)
        fresh.set_scene_mesh(sc.spheres, t2, sc.planes)
        held("after set_mesh_triangles", c, fresh, sc, triangles=t2)


def case_refusals():
    """6: PTMI_ESTATE before a scene, PTMI_EINVAL for NULL with work to do and a negative n or m, through the raw library handle; nothing
    is written; r_max and point may be NULL"""
    sc = SCENES["bvh"]
    n = 65
    bufs = [guarded(n, 1, torch.float32, False), guarded(n, 1, torch.int32, False), guarded(n, 3, torch.float32, False)]
    d_r_max, d_index = dev(np.ones(n, np.float32)), dev(np.arange(n, dtype=np.int32))
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    pts, rm, ix, (dist, idx, at) = vp(sc.d_points), vp(d_r_max), vp(d_index), [vp(b[1]) for b in bufs]

    def untouched(what):
        torch.cuda.synchronize()
        for buf, _, _ in bufs:
            assert (host(buf).view(np.uint32) == SENTINEL).all(), "%s wrote to an output" % what

    with pkg.Context(0) as c:
        L, h = c._lib, c._h
        plain, indexed = L.ptmi_nearest_device, L.ptmi_nearest_indexed_device
        assert plain(h, pts, rm, n, dist, idx, at) == B.PTMI_ESTATE
        assert indexed(h, pts, rm, n, ix, n, dist, idx, at) == B.PTMI_ESTATE
        untouched("a query before any scene")
        sc.set(c)
        for rc in (plain(h, None, rm, n, dist, idx, at), plain(h, pts, rm, n, None, idx, at), plain(h, pts, rm, n, dist, None, at), plain(h, pts, rm, -1, dist, idx, at),
                   indexed(h, pts, rm, n, None, n, dist, idx, at), indexed(h, pts, rm, n, ix, -1, dist, idx, at), indexed(h, pts, rm, -1, ix, n, dist, idx, at),
                   indexed(h, None, rm, n, ix, n, dist, idx, at)):
            assert rc == B.PTMI_EINVAL, rc
        assert b"nearest" in L.ptmi_last_error(h)
        assert plain(h, None, None, 0, None, None, None) == B.PTMI_OK
        assert indexed(h, pts, rm, n, None, 0, dist, idx, at) == B.PTMI_OK and indexed(h, None, None, 0, ix, n, None, None, None) == B.PTMI_OK
        c.synchronize()
        untouched("a refused query")
        assert plain(h, pts, None, n, dist, idx, None) == B.PTMI_OK                     # r_max and point may be NULL
        c.synchronize()
        assert (host(bufs[2][0]).view(np.uint32) == SENTINEL).all(), "a NULL point array was written"
        assert plain(h, pts, None, n, dist, idx, at) == B.PTMI_OK
        c.synchronize()
        assert_same(tuple(host(b[1]) for b in bufs), sc.want, "r_max NULL through the raw handle", rows=slice(0, n))
        for (buf, _, start), words in zip(bufs, (1, 1, 3)):
            guards_intact(buf, start, n * words, "the raw handle")


def case_render_between_queries():
    """7: a render between two queries equals, on all seven planes, a render without them, and the statistics are the same"""
    from conftest import assert_planes_equal
    cam = W.initial_camera()
    for kind in ("bvh", "mesh"):
        sc = SCENES[kind]
        torch.cuda.synchronize()
        with pkg.Context(0) as c:
            sc.set(c)
            c.resize(64, 48)
            planes, stats, keep = [], [], []
            for queries in (False, True):
                c.init_output(0x5EED1234)
                for algorithm in (pkg.INLINE, pkg.STREAMS):
                    if queries:
                        keep.append(c.nearest(sc.d_points, point=True))         # (kept until the stream has passed the call)
                    c.render(cam, 4, 2, algorithm)
                    if queries:
                        keep.append(c.nearest(sc.d_points, r_max=sc.d_r_max))
                planes.append(c.download_state())
                s = c.stats()                             # (the counters run on over init_output: each pass adds the same to them)
                stats.append(tuple(s[f] for f in ("live_bounces", "nominal_bounces", "samples", "stream_iterations", "stream_rays_dropped", "stream_rays_truncated")))
            assert_planes_equal(planes[1], planes[0], "%s: a render between queries" % kind)
            first, both = stats
            assert both[3] == first[3] and tuple(b - a for a, b in zip(first, both))[:3] == first[:3] and both[4:] == first[4:] == (0, 0), (kind, stats)
            assert np.any(np.asarray(planes[0][0]) != 0.0)
            assert_same(tuple(host(x) for x in keep[0]), sc.want, "%s: the query before a render" % kind)


def case_nonfinite_scene_data():
    """8: scene data that is not finite, on a linear scene (ray_query_driver.py's): the twin's answers, and nothing reported is a NaN or an
    inf (assert_same); the bad primitives are never the answer"""
    sc = Scene("nonfinite linear")
    try:
        assert_same(nearest(sc.ctx, sc.d_points), sc.want, "nonfinite linear")
        assert_same(nearest(sc.ctx, sc.d_points, r_max=sc.d_r_max), sc.want_aimed, "nonfinite linear, aimed r_max")
        ns = len(sc.spheres)
        assert not np.isin(sc.want[1], [7, 11, 13, ns, ns + 1, ns + 2]).any()
    finally:
        sc.ctx.close()


RUN = dict(zip(CASES, (case_twin, case_sizes, case_indexed, case_caller_stream, case_after_updates, case_refusals, case_render_between_queries,
                       case_nonfinite_scene_data)))


def main():
    setup()
    for kind in KINDS:
        SCENES[kind] = Scene(kind)
        print("scene %s: answers %d (spheres %d, planes %d, triangles %d), negative distances %d; moved by the aimed r_max %d; not served %d" % SCENES[kind].figures,
              flush=True)
    for name in CASES:
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
    print("NEAREST_DONE", flush=True)


if __name__ == "__main__":
    main()
