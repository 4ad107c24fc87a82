"""Child program of tests/test_gpu_ray_order.py (not a test module): `python tests/ray_order_driver.py WORKDIR`.

ptmi_ray_order_device and the indexed queries (ptmi_trace_rays_indexed_device, ptmi_occluded_indexed_device) through Context.ray_order and
the index= keyword of Context.trace_rays / Context.occluded, as a PyTorch caller uses them, in a process where torch brings the HIP runtime
up before the library is loaded.  The scenes, their 4 096 adversarial rays and the process set-up are tests/ray_query_driver.py's (setup,
Scene, guarded, same_words); the plain entries' answers, which the indexed ones must equal bit for bit, are taken once per scene and shared
by the cases.  One line per case, `ok <case>` or `FAILED <case>: <why>`; a failed comparison does not end the process, a runtime error does;
the last line is RAY_ORDER_DONE."""
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
import ray_order_inputs as inputs  # noqa: E402
import ray_query_driver as Q  # noqa: E402
from ray_query_driver import KINDS, N_RAYS, SENTINEL, Scene, bits, dev, guarded, guards_intact, host, same_words  # noqa: E402
from t_max_families import t_max_for  # noqa: E402

CASES = ["1 order against the host twin", "2 indexed against plain", "3 subsets and bad entries", "4 caller stream", "5 refusals", "6 render after queries"]
ORDER_SIZES = (0, 1, 63, 64, 65, 4095, 4096, 4097, 12293)       # 4 096: the sort's tile; 12 293: three tiles and five rays
SUBSET_SIZES = (0, 1, 63, 64, 65, 257)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
WORK_GUARD = 256                                                  # bytes behind the workspace
WORK_FILL = 0xA5

torch = B = pkg = None
SCENES = {}
PLAIN = {}                                                        # kind -> the plain entries' answers: t, idx, hit, t_max, occluded (host arrays)


def guarded_work(n):
    """ptmi_ray_order_bytes(n) bytes of workspace with guard bytes behind -> (the whole buffer, the workspace, its size)"""
    need = B.ray_order_bytes(n)
    buf = torch.full((need + WORK_GUARD,), WORK_FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 8 == 0
    return buf, buf[:need], need


def device_order(c, d_rays, n):
    """Context.ray_order into guarded memory on the context's own stream -> the order (host); asserts that no guard was written"""
    obuf, order, start = guarded(n, 1, torch.int32, False)
    wbuf, work, need = guarded_work(n)
    torch.cuda.synchronize()
    got = c.ray_order(d_rays, out=order, work=work)
    c.synchronize()
    assert got is order
    guards_intact(obuf, start, n, "order, n = %d" % n)
    assert (host(wbuf[need:]) == WORK_FILL).all(), "n = %d: a byte behind ptmi_ray_order_bytes(n) was written" % n
    return host(order)


def case_order():
    """1: the device order is ptmi_ray_order's, entry for entry"""
    sets = inputs.all_sets(pkg)
    for kind in KINDS:
        assert np.array_equal(bits(sets["adversarial " + kind]), bits(SCENES[kind].rays)), kind      # (the CPU tests' sets are the scenes' rays)
    sets["identical"] = inputs.identical_rays(4097)
    sets["none placed"] = inputs.unplaced_rays()
    c = SCENES["plain"].ctx
    for name, rays in sets.items():
        for n in ORDER_SIZES:
            tiled = inputs.tiled(rays, n)
            want = B.ray_order(tiled)
            got = device_order(c, dev(tiled) if n else torch.zeros((0, 6), dtype=torch.float32, device="cuda"), n)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "%s, n = %d: %d entries differ, e.g. position %d: ray %d, the host twin has ray %d" % (name, n, bad.size, bad[0], got[bad[0]], want[bad[0]])
            if name in ("identical", "none placed"):
                assert np.array_equal(got, np.arange(n)), (name, n)
    # rays 4 bytes off an 8-byte boundary take the dword loads
    rbuf, rays, _ = guarded(N_RAYS, 6, torch.float32, True)
    rays.copy_(SCENES["bvh"].d_rays)
    assert np.array_equal(device_order(c, rays, N_RAYS), B.ray_order(SCENES["bvh"].rays)), "rays 4 bytes off"


def indices_for(kind):
    """The device order, its reverse and a seeded random permutation, as device tensors"""
    sc = SCENES[kind]
    work = torch.empty(B.ray_order_bytes(N_RAYS), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    order = sc.ctx.ray_order(sc.d_rays, work=work)
    sc.ctx.synchronize()
    assert np.array_equal(host(order), B.ray_order(sc.rays)), kind
    perm = np.random.default_rng(7).permutation(N_RAYS).astype(np.int32)
    return {"the device order": order, "its reverse": torch.flip(order, (0,)).contiguous(), "a random permutation": dev(perm)}


def sentinel_outputs(n, misalign=False):
    """t, idx, hit, occluded between guards, every word the sentinel"""
    return [guarded(n, 1, torch.float32, misalign), guarded(n, 1, torch.int32, not misalign), guarded(n, 6, torch.float32, misalign),
            guarded(n, 1, torch.int32, misalign)]


def case_indexed():
    """2: whatever the index holds, the indexed entries' words are the plain entries'"""
    for kind in KINDS:
        sc, (t, idx, hit, t_max, occ) = SCENES[kind], PLAIN[kind]
        d_t_max = dev(t_max)
        for what, index in indices_for(kind).items():
            outs = sentinel_outputs(N_RAYS)
            torch.cuda.synchronize()
            sc.ctx.trace_rays(sc.d_rays, out=(outs[0][1], outs[1][1], outs[2][1]), index=index)
            sc.ctx.occluded(sc.d_rays, d_t_max, out=outs[3][1], index=index)
            sc.ctx.synchronize()
            for (buf, _, start), words in zip(outs, (1, 1, 6, 1)):
                guards_intact(buf, start, N_RAYS * words, "%s through %s" % (kind, what))
            assert same_words(host(outs[0][1]), t).size == 0, "%s through %s: t" % (kind, what)
            assert np.array_equal(host(outs[1][1]), idx), "%s through %s: idx" % (kind, what)
            bad = same_words(host(outs[2][1]), hit)
            assert bad.size == 0, "%s through %s: %d hit records differ, e.g. ray %d" % (kind, what, bad.size, bad[0])
            assert np.array_equal(host(outs[3][1]), occ), "%s through %s: occluded" % (kind, what)
        # outputs allocated by the binding -- on torch's stream, which the context then launches on: the miss record (t 0, idx -1, zeros)
        # and 0 where no entry names a ray
        some = dev(np.arange(0, N_RAYS, 3, dtype=np.int32))
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        sc.ctx.set_stream(stream.cuda_stream)
        try:
            with torch.cuda.stream(stream):
                got = list(sc.ctx.trace_rays(sc.d_rays, hit=True, index=some)) + [sc.ctx.occluded(sc.d_rays, d_t_max, index=some)]
            stream.synchronize()
        finally:
            torch.cuda.synchronize()
            sc.ctx.set_stream(None)
        named = np.zeros(N_RAYS, bool)
        named[::3] = True
        for g, plain, fill, name in zip((host(x) for x in got), (t, idx, hit, occ), (0.0, -1, 0.0, 0), ("t", "idx", "hit", "occluded")):
            want = plain.copy()
            want[~named] = fill
            same = same_words(g, want).size == 0 if plain.dtype == np.float32 else np.array_equal(g, want)
            assert same and g.dtype == plain.dtype, "%s: %s into outputs the binding allocates" % (kind, name)


def subset_index(m, rng):
    """m entries: rays with duplicates, and -1, n, INT32_MIN, INT32_MAX among them once there is room -> (the index, the rays it names)"""
    picks = rng.integers(0, N_RAYS, size=m).astype(np.int64)
    if m >= 2:
        picks[m // 2] = picks[0]                                  # a duplicate
    if m >= 63:
        picks[3::7] = picks[2::7][:len(picks[3::7])]              # many duplicates
        picks[[1, 17, 40, 62]] = [-1, N_RAYS, INT32_MIN, INT32_MAX]
    named = np.unique(picks[(picks >= 0) & (picks < N_RAYS)])
    return picks.astype(np.int32), named


def expect(plain, named, words):
    """The sentinel everywhere, the plain entries' words at the named positions (as uint32) and which of those are NaN"""
    want = np.full((N_RAYS, words), SENTINEL, np.uint32)
    p = np.ascontiguousarray(plain).view(np.uint32).reshape(N_RAYS, words)
    want[named] = p[named]
    nan = np.zeros((N_RAYS, words), bool)
    if plain.dtype == np.float32:
        nan[named] = np.isnan(plain.reshape(N_RAYS, words)[named])
    return want, nan


def check_words(view, plain, named, words, what):
    got = host(view).view(np.uint32).reshape(N_RAYS, words)
    want, nan = expect(plain, named, words)
    bad = (got != want) & ~(nan & np.isnan(got.view(np.float32)))
    rows = np.flatnonzero(bad.any(1))
    assert rows.size == 0, "%s: %d positions differ, e.g. %d (%s): %r, expected %r" % (
        what, rows.size, rows[0], "named" if rows[0] in named else "not named", got[rows[0]], want[rows[0]])


def case_subsets():
    """3: m of n = 4 096 rays, with duplicates and entries outside [0, n): exactly the named positions hold the plain entries' words"""
    rng = np.random.default_rng(21)
    for kind in KINDS:
        sc, (t, idx, hit, t_max, occ) = SCENES[kind], PLAIN[kind]
        trials = [(m, misalign) + subset_index(m, rng) for m in SUBSET_SIZES for misalign in (False, True)]
        trials += [(1, False, np.array([bad], np.int32), np.zeros(0, np.int64)) for bad in (-1, N_RAYS, INT32_MIN, INT32_MAX)]
        for m, misalign, index, named in trials:
            what = "%s, m = %d, %s" % (kind, m, "4 bytes off" if misalign else "8-byte aligned")
            rbuf, rays, _ = guarded(N_RAYS, 6, torch.float32, misalign)
            rays.copy_(sc.d_rays)
            mbuf, tm, _ = guarded(N_RAYS, 1, torch.float32, misalign)
            tm.copy_(dev(t_max))
            ibuf, d_index, istart = guarded(m, 1, torch.int32, misalign)
            if m:
                d_index.copy_(dev(index))
            outs = sentinel_outputs(N_RAYS, misalign)
            torch.cuda.synchronize()
            sc.ctx.trace_rays(rays, out=(outs[0][1], outs[1][1], outs[2][1]), index=d_index)
            sc.ctx.occluded(rays, tm, out=outs[3][1], index=d_index)
            sc.ctx.synchronize()
            for (buf, _, start), words in zip(outs, (1, 1, 6, 1)):
                guards_intact(buf, start, N_RAYS * words, what)
            guards_intact(ibuf, istart, m, what + ": the index")
            assert m == 0 or np.array_equal(host(d_index), index), what + ": the index was written"
            for (_, view, _), plain, words, name in zip(outs, (t, idx, hit, occ), (1, 1, 6, 1), ("t", "idx", "hit", "occluded")):
                check_words(view, plain, named, words, "%s: %s" % (what, name))


def case_caller_stream():
    """4: order, indexed trace and indexed occlusion back to back on torch's non-default stream behind a filler; no host wait in between;
    read after that stream alone is synchronised"""
    stream = torch.cuda.Stream()
    filler = torch.ones((2048, 2048), device="cuda")
    for kind in ("s16", "bvh", "mesh"):
        sc, (t, idx, hit, t_max, occ) = SCENES[kind], PLAIN[kind]
        d_t_max = dev(t_max)
        rays = torch.zeros_like(sc.d_rays)
        tm = torch.zeros_like(d_t_max)
        torch.cuda.synchronize()
        sc.ctx.set_stream(stream.cuda_stream)
        try:
            with torch.cuda.stream(stream):
                x = filler
                for _ in range(20):
                    x = x @ filler * 1e-3
                rays.copy_(sc.d_rays)
                tm.copy_(d_t_max)
                order = sc.ctx.ray_order(rays)
                g_t, g_idx, g_hit = sc.ctx.trace_rays(rays, hit=True, index=order)
                g_occ = sc.ctx.occluded(rays, tm, index=order)
            stream.synchronize()
            assert np.array_equal(host(order), B.ray_order(sc.rays)), "%s: the order on the caller's stream" % kind
            assert same_words(host(g_t), t).size == 0 and np.array_equal(host(g_idx), idx), "%s: closest hit on the caller's stream" % kind
            assert same_words(host(g_hit), hit).size == 0, "%s: hit records on the caller's stream" % kind
            assert np.array_equal(host(g_occ), occ), "%s: occluded on the caller's stream" % kind
            assert float(x.sum()) == float(x.sum())
        finally:
            torch.cuda.synchronize()
            sc.ctx.set_stream(None)


def case_refusals():
    """5: every row of the header's refusal lists through the raw library handle; outputs and workspace untouched"""
    sc = SCENES["bvh"]
    n, m = 65, 40
    outs = sentinel_outputs(n)
    obuf, order, _ = guarded(n, 1, torch.int32, False)
    wbuf, work, need = guarded_work(n)
    d_t_max = dev(np.ones(n, np.float32))
    d_index = dev(np.arange(m, dtype=np.int32))
    torch.cuda.synchronize()
    vp = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    rays, (t, idx, hit, occ), tmx, index = vp(sc.d_rays), [vp(o[1]) for o in outs], vp(d_t_max), vp(d_index)

    def untouched(what):
        torch.cuda.synchronize()
        for buf, _, _ in outs + [(obuf, None, None)]:
            assert (host(buf).view(np.uint32) == SENTINEL).all(), "%s wrote to an output" % what
        assert (host(wbuf) == WORK_FILL).all(), "%s wrote to the workspace" % what

    with pkg.Context(0) as c:
        lib, h = c._lib, c._h
        assert lib.ptmi_trace_rays_indexed_device(h, rays, n, index, m, t, idx, hit) == B.PTMI_ESTATE
        assert lib.ptmi_occluded_indexed_device(h, rays, tmx, n, index, m, occ) == B.PTMI_ESTATE
        untouched("an indexed query before any scene")
        assert need == lib.ptmi_ray_order_bytes(n) and lib.ptmi_ray_order_bytes(0) == 0 and lib.ptmi_ray_order_bytes(-3) == 0
        refused = [(lib.ptmi_ray_order_device(h, rays, -1, vp(order), vp(work), need), B.PTMI_EINVAL, "n < 0"),
                   (lib.ptmi_ray_order_device(h, None, n, vp(order), vp(work), need), B.PTMI_EINVAL, "no rays"),
                   (lib.ptmi_ray_order_device(h, rays, n, None, vp(work), need), B.PTMI_EINVAL, "no order"),
                   (lib.ptmi_ray_order_device(h, rays, n, vp(order), None, need), B.PTMI_EINVAL, "no workspace"),
                   (lib.ptmi_ray_order_device(h, rays, n, vp(order), C.c_void_p(work.data_ptr() + 4), need), B.PTMI_EINVAL, "workspace 4 bytes off"),
                   (lib.ptmi_ray_order_device(h, rays, n, vp(order), vp(work), need - 1), B.PTMI_EINVAL, "workspace one byte short"),
                   (lib.ptmi_ray_order_device(h, rays, n, vp(order), vp(work), 0), B.PTMI_EINVAL, "workspace of no bytes"),
                   (lib.ptmi_ray_order_device(h, rays, B.RAY_ORDER_MAX + 1, vp(order), vp(work), 1 << 40), B.PTMI_ELIMIT, "n > PTMI_RAY_ORDER_MAX")]
        for rc, want, what in refused:
            assert rc == want, (what, rc)
        assert lib.ptmi_ray_order_device(h, None, 0, None, None, 0) == B.PTMI_OK
        c.synchronize()
        untouched("a refused ray order")
        # no scene is needed for the order
        assert lib.ptmi_ray_order_device(h, rays, n, vp(order), vp(work), need) == B.PTMI_OK
        c.synchronize()
        assert np.array_equal(host(order), B.ray_order(sc.rays[:n])), "the order before any scene"
        assert (host(wbuf[need:]) == WORK_FILL).all()
        order.fill_(SENTINEL)
        wbuf.fill_(WORK_FILL)
        sc.set(c)
        T, O = lib.ptmi_trace_rays_indexed_device, lib.ptmi_occluded_indexed_device
        for rc in (T(h, None, n, index, m, t, idx, hit), T(h, rays, n, index, m, None, idx, hit), T(h, rays, n, index, m, t, None, hit),
                   T(h, rays, -1, index, m, t, idx, hit), T(h, rays, n, index, -1, t, idx, hit), T(h, rays, n, None, m, t, idx, hit),
                   O(h, None, tmx, n, index, m, occ), O(h, rays, None, n, index, m, occ), O(h, rays, tmx, n, index, m, None),
                   O(h, rays, tmx, -5, index, m, occ), O(h, rays, tmx, n, index, -2, occ), O(h, rays, tmx, n, None, m, occ)):
            assert rc == B.PTMI_EINVAL, rc
        assert b"ray-query" in lib.ptmi_last_error(h)
        assert T(h, rays, n, None, 0, t, idx, hit) == B.PTMI_OK and O(h, rays, tmx, n, None, 0, occ) == B.PTMI_OK            # m == 0
        assert T(h, None, 0, index, m, None, None, None) == B.PTMI_OK and O(h, None, None, 0, index, m, None) == B.PTMI_OK  # n == 0: every entry is outside
        c.synchronize()
        untouched("a refused indexed query")
        assert T(h, rays, n, index, m, t, idx, None) == B.PTMI_OK                                  # hit may be NULL: t and idx alone are written
        c.synchronize()
        p_t, p_idx = PLAIN["bvh"][0], PLAIN["bvh"][1]
        assert same_words(host(outs[0][1])[:m], p_t[:m]).size == 0 and np.array_equal(host(outs[1][1])[:m], p_idx[:m])
        assert (host(outs[0][1]).view(np.uint32)[m:] == SENTINEL).all() and (host(outs[2][0]).view(np.uint32) == SENTINEL).all()


def case_render_after_queries():
    """6: a render with order and indexed queries in between equals, on all seven planes, one without them (64 x 48, one BVH and one mesh scene)"""
    from conftest import assert_planes_equal
    cam = Q.W.initial_camera()
    for kind in ("bvh", "mesh"):
        sc = SCENES[kind]
        d_t_max = dev(PLAIN[kind][3])
        work = torch.empty(B.ray_order_bytes(N_RAYS), dtype=torch.uint8, device="cuda")
        order = torch.empty(N_RAYS, dtype=torch.int32, device="cuda")
        outs = (torch.empty(N_RAYS, dtype=torch.float32, device="cuda"), torch.empty(N_RAYS, dtype=torch.int32, device="cuda"),
                torch.empty((N_RAYS, 6), dtype=torch.float32, device="cuda"))
        occ = torch.empty(N_RAYS, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pkg.Context(0) as c:
            sc.set(c)
            c.resize(64, 48)
            planes = []
            for queries in (False, True):
                c.init_output(0x5EED1234)
                for algorithm in (pkg.INLINE, pkg.STREAMS):
                    if queries:
                        c.ray_order(sc.d_rays, out=order, work=work)
                        c.trace_rays(sc.d_rays, out=outs, index=order)
                    c.render(cam, 4, 2, algorithm)
                    if queries:
                        c.occluded(sc.d_rays, d_t_max, out=occ, index=order)
                planes.append(c.download_state())
            assert_planes_equal(planes[1], planes[0], "%s: a render between order and indexed queries" % kind)
            assert np.any(np.asarray(planes[0][0]) != 0.0)
            c.synchronize()
            assert np.array_equal(host(occ), PLAIN[kind][4]) and np.array_equal(host(outs[1]), PLAIN[kind][1]), kind


RUN = dict(zip(CASES, (case_order, case_indexed, case_subsets, case_caller_stream, case_refusals, case_render_after_queries)))


def main():
    global torch, B, pkg
    Q.setup(sys.argv[1])
    torch, B, pkg = Q.torch, Q.B, Q.pkg
    for kind in KINDS:
        sc = SCENES[kind] = Scene(kind)
        t_max, _, _ = t_max_for(sc)
        t, idx, hit = (host(x) for x in Q.trace(sc.ctx, sc.d_rays, hit=True))
        occ = host(Q.occluded(sc.ctx, sc.d_rays, dev(t_max)))
        assert np.array_equal(bits(t), bits(sc.t)) and np.array_equal(idx, sc.idx), kind
        PLAIN[kind] = (t, idx, hit, t_max, occ)
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
    print("RAY_ORDER_DONE", flush=True)


if __name__ == "__main__":
    main()
