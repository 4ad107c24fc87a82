"""Child program of tests/test_gpu_multi_hit.py (not a test module): `python tests/multi_hit_driver.py WORKDIR`.

ptmi_trace_rays_multi_device and its indexed form through Context.trace_rays_multi, as a PyTorch caller uses them: device tensors in,
device tensors out, on the context's stream, in a process where torch brings the HIP runtime up before the library is loaded.  The scenes
are tests/ray_query_driver.py's five kinds, each extended by the stack of tests/multi_hit_rays.py (driver_scene); the reference is the
specification by enumeration (tests/cxx/multi_hit_reference.c).  Before any device call the reference alone must show, per scene kind at
k = 4, that the comparison is not vacuous (multi_hit_rays.assert_not_vacuous).  One line per case, `ok <case>` or `FAILED <case>: <why>`;
a failed comparison does not end the process, a runtime error does; the last line is MULTI_HIT_DONE."""
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

CASES = ["1 the specification", "2 sizes alignment guards", "3 closest hit and occlusion", "4 listed distances", "5 indexed", "6 caller stream",
         "7 after device updates", "8 refusals", "9 render between queries", "10 non-finite scene data"]
KS = (1, 2, 3, 4, 5, 8, 15, 16)
SIZES = (0, 1, 63, 64, 65, 257, 4096)
GUARD = 64
SENTINEL = 0x7FC0DEAD

torch = pkg = B = W = M = mesh_rays = None
lib = mlib = None
SCENES = {}


def setup(workdir):
    global torch, pkg, B, W, M, mesh_rays, lib, mlib
    import torch as _torch
    torch = _torch
    torch.zeros(1, device="cuda")                      # torch brings the runtime up first
    torch.cuda.synchronize()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg._build.build_lib()
    graft.load_oracle().build()
    B, W = pkg.binding, pkg.world
    import mesh_rays as _m
    import multi_hit_rays as _M
    M, mesh_rays = _M, _m
    lib, mlib = M.multi_hit_lib(workdir), mesh_rays.traverse_lib(workdir)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def multi(c, rays, k, **kw):
    """Context.trace_rays_multi on the context's OWN stream from torch's, with host waits on either side"""
    torch.cuda.synchronize()
    out = c.trace_rays_multi(rays, k, **kw)
    c.synchronize()
    return tuple(host(x) for x in out)


class Scene:
    def __init__(self, kind):
        self.kind = kind
        self.spheres, self.triangles, self.planes, self.rays = M.driver_scene(kind)
        self.records = mesh_rays.records(mlib, self.triangles) if self.triangles is not None else None
        self.n = len(self.rays)
        self.served = M.served_by(kind, self.spheres, self.triangles, self.rays)
        self.refs = {}
        self.figures = M.assert_not_vacuous(kind, self.ref(4), self.served) if kind in M.KINDS else None      # BEFORE any device call
        self.d_rays = dev(self.rays)
        torch.cuda.synchronize()
        self.ctx = pkg.Context(0)
        self.set(self.ctx)

    def ref(self, k, t_max=None, key=None):
        """The specification at k, kept when t_max is None or named by `key`"""
        name = (k, key)
        if t_max is None or key is not None:
            if name not in self.refs:
                self.refs[name] = M.reference(lib, self.spheres, self.planes, self.records, self.rays, t_max, k)
            return self.refs[name]
        return M.reference(lib, self.spheres, self.planes, self.records, self.rays, t_max, k)

    def aimed(self, k):
        return M.aimed_t_max(self.ref(k + 1), k)

    def set(self, c):
        if self.kind == "mesh":
            c.set_scene_mesh(self.spheres, self.triangles, self.planes)
        elif self.kind in ("bvh", "nonfinite bvh"):
            c.set_scene_bvh(self.spheres, self.planes)
        else:
            c.set_scene(self.spheres, self.planes)


def assert_rows(got, want, what, rows=None):
    """The three outputs against the specification; unused slots are exactly (0, -1) (the reference writes them so, and t is compared as
    a number: multi_hit_rays.rows_differ); no listed t is a NaN or an inf"""
    if rows is not None:
        import types
        want = types.SimpleNamespace(t=want.t[rows], idx=want.idx[rows], count=want.count[rows])
    bad = M.rows_differ(got, want)
    assert bad.size == 0, "%s: %d rays differ, e.g. ray %d: device t %r idx %r count %d, expected t %r idx %r count %d" % (
        what, bad.size, bad[0], got[0][bad[0]], got[1][bad[0]], got[2][bad[0]], want.t[bad[0]], want.idx[bad[0]], want.count[bad[0]])
    assert np.isfinite(got[0]).all() and (got[0] >= 0).all(), what + ": a listed t is not finite or negative"
    unused = np.arange(got[0].shape[1])[None, :] >= got[2][:, None]
    assert (bits(got[0])[unused] == 0).all() and (got[1][unused] == -1).all(), what + ": an unused slot is not (0, -1)"


def case_specification():
    """1: t, idx and count are the specification's, for every scene kind and k, with t_max absent and from every family aimed at the 1st,
    the k-th and the (k+1)-th hit"""
    for kind in M.KINDS:
        sc = SCENES[kind]
        for k in KS:
            assert_rows(multi(sc.ctx, sc.d_rays, k), sc.ref(k), "%s, k = %d, no t_max" % (kind, k))
            t_max = sc.aimed(k)
            want = sc.ref(k, t_max, "aimed")
            assert (want.count < sc.ref(k).count).sum() >= 100 and (want.count == k).sum() >= (64 if k < 16 else 16), (kind, k)
            assert_rows(multi(sc.ctx, sc.d_rays, k, t_max=dev(t_max)), want, "%s, k = %d, aimed t_max" % (kind, k))


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
    """2: wave and block tails; every array 16-byte aligned and 4 bytes off (the rows' wide stores need k % 4 == 0 AND aligned arrays: k =
    4, 8 and 16 take them when aligned, 5 never does); 64 guard words on either side of every output"""
    for kind in M.KINDS:
        sc = SCENES[kind]
        for k in (4, 5, 8, 16):
            t_max = sc.aimed(k)
            want = sc.ref(k, t_max, "aimed")
            for n in SIZES:
                for off in ((False, False, False), (True, True, True), (False, True, False), (True, False, True)):
                    what = "%s, k = %d, n = %d, arrays off by %r" % (kind, k, n, off)
                    _, rays, _ = guarded(n, 6, torch.float32, off[0])
                    rays.copy_(sc.d_rays[:n])
                    _, tm, _ = guarded(n, 1, torch.float32, off[2])
                    tm.copy_(dev(t_max[:n]))
                    outs = [guarded(n, k, torch.float32, off[0]), guarded(n, k, torch.int32, off[1]), guarded(n, 1, torch.int32, off[2])]
                    torch.cuda.synchronize()
                    sc.ctx.trace_rays_multi(rays, k, t_max=tm, out=tuple(o[1] for o in outs))
                    sc.ctx.synchronize()
                    for (buf, view, start), words in zip(outs, (k, k, 1)):
                        guards_intact(buf, start, n * words, what)
                    if n:
                        assert_rows(tuple(host(o[1]) for o in outs), want, what, rows=slice(0, n))


def case_relations():
    """3: over the rays the reference marks free of NaN keys: column 0 at k = 1 without t_max is trace_rays' (t, idx) -- except that a closest
    hit at t = +inf, which the fold keeps when nothing nearer is hit, is no listed hit (every listed t is finite: the list is then empty);
    count > 0 at k = 1 is occluded under the same t_max -- on the device"""
    for kind in M.KINDS:
        sc = SCENES[kind]
        clean = (sc.ref(1).flags & 1) == 0
        assert clean.sum() >= 3000, (kind, int(clean.sum()))
        torch.cuda.synchronize()
        closest = sc.ctx.trace_rays(sc.d_rays)
        sc.ctx.synchronize()
        t, idx = (host(x) for x in closest)
        mt, mi, mc = multi(sc.ctx, sc.d_rays, 1)
        at_inf = np.isinf(t) & (idx >= 0)
        bad = np.flatnonzero(clean & np.where(at_inf, mc != 0, (bits(mt[:, 0]) != bits(t)) | (mi[:, 0] != idx)))
        assert bad.size == 0, "%s: %d rays differ from trace_rays, e.g. ray %d: (%r, %d) against (%r, %d)" % (
            kind, bad.size, bad[0], mt[bad[0], 0], mi[bad[0], 0], t[bad[0]], idx[bad[0]])
        assert (clean & ~at_inf & (idx >= 0)).sum() >= 2500, kind
        t_max = sc.aimed(1)
        d_t_max = dev(t_max)
        torch.cuda.synchronize()
        occ = sc.ctx.occluded(sc.d_rays, d_t_max)
        sc.ctx.synchronize()
        occ = host(occ)
        _, _, mc = multi(sc.ctx, sc.d_rays, 1, t_max=d_t_max)
        bad = np.flatnonzero(clean & ((mc > 0) != (occ != 0)))
        assert bad.size == 0, "%s: %d rays differ from occluded, e.g. ray %d (t_max %r): count %d, occluded %d" % (kind, bad.size, bad[0], t_max[bad[0]], mc[bad[0]], occ[bad[0]])
        assert (occ[clean] != 0).sum() >= 100 and (occ[clean] == 0).sum() >= 100, kind


def case_listed_distances():
    """4: on the linear scenes every listed t is ptmi_eval_distance_to_sphere's / ptmi_eval_distance_to_plane's for that primitive and ray,
    bit for bit"""
    for kind in ("plain", "s16", "runs"):
        sc = SCENES[kind]
        k = 16
        t, idx, count = multi(sc.ctx, sc.d_rays, k)
        ns = len(sc.spheres)
        for c in range(k):
            on = np.flatnonzero(c < count)
            if on.size == 0:
                continue
            j = idx[on, c]
            for rows, prims, fn in ((on[j < ns], sc.spheres[j[j < ns]], sc.ctx.eval_distance_to_sphere), (on[j >= ns], sc.planes[j[j >= ns] - ns], sc.ctx.eval_distance_to_plane)):
                if rows.size:
                    just, want = fn(prims, sc.rays[rows])[:2]
                    assert (np.asarray(just) != 0).all(), "%s: a listed primitive is no Just for its ray" % kind
                    assert np.array_equal(bits(t[rows, c]), bits(np.asarray(want, np.float32))), "%s, column %d: t differs from the point query" % (kind, c)
        assert (count == k).sum() >= 400, kind


def case_indexed():
    """5: through ray_order's order, through a list of live rays (m < n), and with entries outside [0, n): the words are the plain
    entry's, unnamed rows stay untouched"""
    for kind in M.KINDS:
        sc = SCENES[kind]
        for k in (3, 4, 16):
            want = sc.ref(k)
            torch.cuda.synchronize()
            order = sc.ctx.ray_order(sc.d_rays)
            sc.ctx.synchronize()
            assert_rows(multi(sc.ctx, sc.d_rays, k, index=order), want, "%s, k = %d, ray_order's order" % (kind, k))
            rng = np.random.default_rng(9)
            live = np.sort(rng.choice(sc.n, sc.n // 3, replace=False)).astype(np.int32)
            index = np.concatenate([live[:500], [-1, sc.n, sc.n + 7, -2 ** 31, 2 ** 31 - 1], live[500:]]).astype(np.int32)
            rng.shuffle(index)
            outs = (torch.full((sc.n, k), 7.5, dtype=torch.float32, device="cuda"), torch.full((sc.n, k), 77, dtype=torch.int32, device="cuda"),
                    torch.full((sc.n,), 777, dtype=torch.int32, device="cuda"))
            got = multi(sc.ctx, sc.d_rays, k, index=dev(index), out=outs)
            named = np.zeros(sc.n, bool)
            named[live] = True
            assert_rows(tuple(g[named] for g in got), want, "%s, k = %d, a live list" % (kind, k), rows=named)
            assert (got[0][~named] == 7.5).all() and (got[1][~named] == 77).all() and (got[2][~named] == 777).all(), "%s: an unnamed row was written" % kind
            fresh = multi(sc.ctx, sc.d_rays, k, index=dev(live))                      # allocated by the binding: the miss record and a count of 0 first
            assert (bits(fresh[0][~named]) == 0).all() and (fresh[1][~named] == -1).all() and (fresh[2][~named] == 0).all(), kind


def case_caller_stream():
    """6: on torch's non-default stream through set_stream; the inputs are written on that stream behind a filler, the results are read
    after that stream alone is synchronised"""
    stream = torch.cuda.Stream()
    filler = torch.ones((2048, 2048), device="cuda")
    for kind in ("s16", "bvh", "mesh"):
        sc = SCENES[kind]
        t_max = sc.aimed(4)
        d_t_max = dev(t_max)
        rays, tm = torch.zeros_like(sc.d_rays), torch.zeros_like(d_t_max)
        torch.cuda.synchronize()
        sc.ctx.set_stream(stream.cuda_stream)
        try:
            with torch.cuda.stream(stream):
                x = filler
                for _ in range(20):
                    x = x @ filler * 1e-3
                rays.copy_(sc.d_rays)
                tm.copy_(d_t_max)
                a = sc.ctx.trace_rays_multi(rays, 4, t_max=tm)
                b = sc.ctx.trace_rays_multi(rays, 16)
            stream.synchronize()
            assert_rows(tuple(host(v) for v in a), sc.ref(4, t_max, "aimed"), "%s on the caller's stream, k = 4" % kind)
            assert_rows(tuple(host(v) for v in b), sc.ref(16), "%s on the caller's stream, k = 16" % kind)
            assert float(x.sum()) == float(x.sum())
        finally:
            torch.cuda.synchronize()
            sc.ctx.set_stream(None)


def case_after_updates():
    """7: after update_spheres and after set_mesh_triangles from device tensors, a query enqueued at once answers for the new scene: it
    equals a context set afresh, and the specification of the new scene"""
    sc = SCENES["bvh"]
    g = W.displaced_spheres(W.sphere_geometry(sc.spheres), 0.5, "wave", seed=2)
    moved = W.with_sphere_geometry(sc.spheres, g)
    d_g = dev(np.ascontiguousarray(g, np.float32))
    torch.cuda.synchronize()
    with pkg.Context(0) as c, pkg.Context(0) as fresh:
        c.set_scene_bvh(sc.spheres, sc.planes)
        c.update_spheres(d_g)
        got = c.trace_rays_multi(sc.d_rays, 4)          # at once: ordered behind the update by the stream alone
        c.synchronize()
        got = tuple(host(x) for x in got)
        fresh.set_scene_bvh(moved, sc.planes)
        want = multi(fresh, sc.d_rays, 4)
        for a, b, name in zip(got, want, ("t", "idx", "count")):
            assert np.array_equal(bits(a), bits(b)), "after update_spheres: %s" % name
        assert_rows(got, M.reference(lib, moved, sc.planes, None, sc.rays, None, 4), "after update_spheres, against the specification")
        assert M.rows_differ(got, sc.ref(4)).size > 100, "the update moved nothing"
    sc = SCENES["mesh"]
    t2 = np.concatenate([mesh_rays.adversarial_scene(1, seed=4)[1], M.stack_quads(sc.triangles, M.STACK_BASE["mesh"])])
    d_t2 = dev(np.ascontiguousarray(t2).view(np.float32).reshape(-1, 15).copy())
    torch.cuda.synchronize()
    with pkg.Context(0) as c, pkg.Context(0) as fresh:
        sc.set(c)
        c.set_mesh_triangles(d_t2)
        got = c.trace_rays_multi(sc.d_rays, 4)
        c.synchronize()
        got = tuple(host(x) for x in got)
        fresh.set_scene_mesh(sc.spheres, t2, sc.planes)
        want = multi(fresh, sc.d_rays, 4)
        for a, b, name in zip(got, want, ("t", "idx", "count")):
            assert np.array_equal(bits(a), bits(b)), "after set_mesh_triangles: %s" % name
        assert_rows(got, M.reference(lib, sc.spheres, sc.planes, mesh_rays.records(mlib, t2), sc.rays, None, 4), "after set_mesh_triangles, against the specification")
        assert M.rows_differ(got, sc.ref(4)).size > 100, "the new triangles changed nothing"


def case_refusals():
    """8: PTMI_ESTATE before a scene, PTMI_EINVAL for NULL with work to do, a negative n or m and k < 1, PTMI_ELIMIT for k beyond
    PTMI_MULTI_HIT_MAX, through the raw library handle; nothing is written"""
    sc = SCENES["bvh"]
    n, k = 65, 4
    bufs = [guarded(n, k, torch.float32, False), guarded(n, k, torch.int32, False), guarded(n, 1, torch.int32, False)]
    d_t_max, d_index = dev(np.ones(n, np.float32)), dev(np.arange(n, dtype=np.int32))
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rays, tm, ix, (t, idx, cnt) = vp(sc.d_rays), vp(d_t_max), vp(d_index), [vp(b[1]) for b in bufs]

    def untouched(what):
        torch.cuda.synchronize()
        for buf, _, _ in bufs:
            assert (host(buf).view(np.uint32) == SENTINEL).all(), "%s wrote to an output" % what

    with pkg.Context(0) as c:
        L, h = c._lib, c._h
        plain, indexed = L.ptmi_trace_rays_multi_device, L.ptmi_trace_rays_multi_indexed_device
        assert plain(h, rays, tm, n, k, t, idx, cnt) == B.PTMI_ESTATE
        assert indexed(h, rays, tm, n, ix, n, k, t, idx, cnt) == B.PTMI_ESTATE
        untouched("a query before any scene")
        sc.set(c)
        for rc in (plain(h, None, tm, n, k, t, idx, cnt), plain(h, rays, tm, n, k, None, idx, cnt), plain(h, rays, tm, n, k, t, None, cnt),
                   plain(h, rays, tm, n, k, t, idx, None), plain(h, rays, tm, -1, k, t, idx, cnt), plain(h, rays, tm, n, 0, t, idx, cnt),
                   plain(h, rays, tm, n, -3, t, idx, cnt), indexed(h, rays, tm, n, None, n, k, t, idx, cnt), indexed(h, rays, tm, n, ix, -1, k, t, idx, cnt),
                   indexed(h, rays, tm, -1, ix, n, k, t, idx, cnt), indexed(h, rays, tm, n, ix, n, 0, t, idx, cnt), indexed(h, None, tm, n, ix, n, k, t, idx, cnt)):
            assert rc == B.PTMI_EINVAL, rc
        assert b"multi-hit" in L.ptmi_last_error(h)
        assert plain(h, rays, tm, n, 17, t, idx, cnt) == B.PTMI_ELIMIT and indexed(h, rays, tm, n, ix, n, 1 << 20, t, idx, cnt) == B.PTMI_ELIMIT
        assert plain(h, None, None, 0, k, None, None, None) == B.PTMI_OK
        assert indexed(h, rays, tm, n, None, 0, k, t, idx, cnt) == B.PTMI_OK and indexed(h, None, None, 0, ix, n, k, None, None, None) == B.PTMI_OK
        c.synchronize()
        untouched("a refused query")
        assert plain(h, rays, None, n, k, t, idx, cnt) == B.PTMI_OK                     # t_max may be NULL
        c.synchronize()
        assert_rows(tuple(host(b[1]) for b in bufs), sc.ref(k), "t_max NULL through the raw handle", rows=slice(0, n))
        for (buf, _, start), words in zip(bufs, (k, k, 1)):
            guards_intact(buf, start, n * words, "the raw handle")


def case_render_between_queries():
    """9: a render between two queries equals, on all seven planes, a render without them, and the statistics are the same"""
    from conftest import assert_planes_equal
    cam = W.initial_camera()
    for kind in ("bvh", "mesh"):
        sc = SCENES[kind]
        d_t_max = dev(sc.aimed(4))
        torch.cuda.synchronize()
        with pkg.Context(0) as c:
            sc.set(c)
            c.resize(64, 48)
            planes, stats, keep = [], [], []
            for queries in (False, True):
                c.init_output(0x5EED1234)
                for algorithm in (pkg.INLINE, pkg.STREAMS):
                    if queries:
                        keep.append(c.trace_rays_multi(sc.d_rays, 16))      # (kept until the stream has passed the call)
                    c.render(cam, 4, 2, algorithm)
                    if queries:
                        keep.append(c.trace_rays_multi(sc.d_rays, 4, t_max=d_t_max))
                planes.append(c.download_state())
                s = c.stats()                             # (the counters run on over init_output: each pass adds the same to them)
                stats.append(tuple(s[f] for f in ("live_bounces", "nominal_bounces", "samples", "stream_iterations", "stream_rays_dropped", "stream_rays_truncated")))
            assert_planes_equal(planes[1], planes[0], "%s: a render between queries" % kind)
            first, both = stats
            assert both[3] == first[3] and tuple(b - a for a, b in zip(first, both))[:3] == first[:3] and both[4:] == first[4:] == (0, 0), (kind, stats)
            assert np.any(np.asarray(planes[0][0]) != 0.0)


def case_nonfinite_scene_data():
    """10: scene data that is not finite (ray_query_driver.py's nonfinite scenes): the answers are the specification's, and no NaN or inf t
    is listed (assert_rows)"""
    for kind in ("nonfinite linear", "nonfinite bvh"):
        sc = Scene(kind)
        try:
            for k in (1, 4, 16):
                assert_rows(multi(sc.ctx, sc.d_rays, k), sc.ref(k), "%s, k = %d" % (kind, k))
                t_max = sc.aimed(k)
                assert_rows(multi(sc.ctx, sc.d_rays, k, t_max=dev(t_max)), sc.ref(k, t_max, "aimed"), "%s, k = %d, aimed t_max" % (kind, k))
            assert (sc.ref(4).flags & 1).sum() >= 1000 and (sc.ref(4).count > 0).sum() >= 1000, kind      # NaN keys everywhere, and hits listed beside them
        finally:
            sc.ctx.close()


RUN = dict(zip(CASES, (case_specification, case_sizes, case_relations, case_listed_distances, case_indexed, case_caller_stream, case_after_updates,
                       case_refusals, case_render_between_queries, case_nonfinite_scene_data)))


def main():
    setup(sys.argv[1])
    for kind in M.KINDS:
        SCENES[kind] = Scene(kind)
        print("scene %s: served rays with |H| > 4: %d, 0 < |H| < 4: %d, |H| = 0: %d, a tie listed: %d; not served: %d" % SCENES[kind].figures, flush=True)
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
    print("MULTI_HIT_DONE", flush=True)


if __name__ == "__main__":
    main()
