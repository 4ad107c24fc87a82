"""Every kernel launch and memset one render call enqueues, pinned for a fixed matrix of calls (tests/golden/launch_table.json).

A CHILD process runs libptmi and libptmi_ablations on the HIP stand-in of tests/cxx/hip_stub.cpp (preloaded, without a sanitizer: kernels
do not run, launches and memsets are logged in order) and records, for every case, the log of one render call: kernel, grid, block and
dynamic LDS bytes of each launch, value and size of each memset.  The matrix crosses scenes (small linear = staged in LDS, big linear =
scalar loads, GLASS, BVH, BVH with GLASS), Inline and Streams, the kernel variants, a row-mapped and a tiled image, sample counts that
choose sample chunks automatically or have them forced, the degenerate limit 0 and spp 0, render1 with explicit screen coordinates, a
partitioned context, both forms of Streams and contracted arithmetic.  A refused call is recorded with its error code.

The golden file is what the launchers did when it was made; a change that moves a launch on purpose regenerates it
(python tests/test_launch_table.py --regenerate) and says why.  What this does NOT test: any kernel, any rendered value."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_table.json")
STUB = os.path.join(ROOT, "build", "hip_stub", "libhipstub_plain.so")

SHAPES = ((40, 10), (160, 96))                       # rows of 64 / 8x8 tiles
COUNTS = (("spp1", 8, 1, 0), ("spp256", 8, 256, 0), ("chunks1", 8, 256, 1), ("chunks4", 8, 256, 4), ("limit0", 0, 4, 0), ("spp0", 8, 0, 0))
ABLATION_COUNTS = COUNTS[:2] + COUNTS[4:]


def record(pkg, stub):
    """{case: [log lines]} for the whole matrix (in the child)."""
    import ctypes
    B, world = pkg.binding, pkg.world
    stub.hipstub_log.restype = ctypes.c_char_p
    cam = world.initial_camera()
    names = {}

    def short(line):                                  # the demangled kernel name without namespaces and parameters
        if not line.startswith("launch "):
            return line
        mangled, rest = line[7:].split(" ", 1)
        if mangled not in names:
            dem = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
            names[mangled] = dem.replace("void ", "", 1).replace("(anonymous namespace)::", "").split("(")[0]
        return "launch %s %s" % (names[mangled], rest)

    out = {}

    def case(key, call):
        stub.hipstub_clear_log()
        try:
            call()
            res = []
        except B.PtmiError as e:
            res = ["error %d" % e.code]
        log = stub.hipstub_log().decode()
        assert "truncated" not in log, key
        out[key] = [short(x) for x in log.splitlines()] + res

    scenes = {"small": lambda c: c.set_scene(*world.scene16()),
              "big": lambda c: c.set_scene(*world.sphere_field(120, seed=1)),
              "glass": lambda c: c.set_scene(*world.glass_scene()),
              "bvh": lambda c: c.set_scene_bvh(*world.sphere_field(3000, seed=2)),
              "bvhglass": lambda c: c.set_scene_bvh(*world.sphere_field(3000, seed=3, glass_fraction=0.2))}
    algs = (("inline", pkg.INLINE), ("streams", pkg.STREAMS))

    def sweep(lib, tag, scene_names, variants, counts):
        for sname in scene_names:
            with pkg.Context(0, library=lib) as c:
                scenes[sname](c)
                for (w, h) in SHAPES:
                    c.resize(w, h)
                    c.init_output(7)
                    for v in variants:
                        for aname, alg in algs:
                            for cname, limit, spp, chunks in counts:
                                def call():
                                    c.set_variant(v)
                                    c.set_option(B.OPT_SPP_CHUNKS, chunks)
                                    c.render(cam, limit, spp, alg)
                                case("%s/%s/%dx%d/v%d/%s/%s" % (tag, sname, w, h, v, aname, cname), call)
                    quiet(lambda: c.set_variant(0))

    def quiet(call):
        try:
            call()
        except B.PtmiError:
            pass

    default = B.load_library()
    ablations = B.open_library(pkg._build.ABLATIONS_LIB)
    sweep(default, "lib", list(scenes), (0, 4, 5, 9, 13, 17), COUNTS)
    sweep(ablations, "abl", ["small", "big"], range(1, 19), ABLATION_COUNTS)

    for lib, tag, variants in ((default, "lib", (0, 4, 5, 9, 13, 17)), (ablations, "abl", range(1, 19))):     # a part with no rows
        with pkg.Context(0, library=lib) as c:
            c.set_scene(*world.scene16())
            c.set_partition(8, 8, 7)
            c.resize(160, 16)
            c.init_output(3)
            for v in variants:
                for aname, alg in algs:
                    def call():
                        c.set_variant(v)
                        c.render(cam, 8, 4, alg)
                    case("empty/%s/v%d/%s" % (tag, v, aname), call)

    # the other entry points and options, on the scenes they apply to
    for sname in scenes:
        with pkg.Context(0) as c:
            scenes[sname](c)
            for (w, h) in SHAPES:
                xs, ys = world.screen_pixels(w, h)
                p = [np.zeros((h, w), np.float32) for _ in range(3)] + [np.arange(w * h, dtype=np.uint32).reshape(h, w) + k for k in range(4)]
                for aname, alg in algs:
                    case("render1/%s/%dx%d/%s" % (sname, w, h, aname), lambda: c.render1(cam, 8, w, h, p, alg))
                    case("render1-screen/%s/%dx%d/%s" % (sname, w, h, aname), lambda: c.render1(cam, 8, w, h, p, alg, screen=(xs, ys)))
            c.resize(160, 96)
            c.init_output(7)
            for form, fname in ((B.FORM_PIXEL, "pixel"), (B.FORM_STREAM, "stream")):
                quiet(lambda: c.set_option(B.OPT_STREAMS_FORM, form))
                for cname, limit, spp, _ in COUNTS[:2] + (("spp4", 8, 4, 0),):      # (spp4: one pass with a cost order -- the stream form's tail)
                    case("form-%s/%s/%s" % (fname, sname, cname), lambda: c.render(cam, limit, spp, pkg.STREAMS))
            quiet(lambda: c.set_option(B.OPT_STREAMS_FORM, B.FORM_AUTO))
            quiet(lambda: c.set_option(B.OPT_ARITHMETIC, B.ARITH_CONTRACTED))
            for v in (0, 9, 13, 17):
                for cname, limit, spp, _ in COUNTS:
                    def call():
                        c.set_variant(v)
                        c.render(cam, limit, spp, pkg.INLINE)
                    case("contracted/%s/v%d/%s" % (sname, v, cname), call)
            quiet(lambda: c.set_variant(0))
        for n_parts, part, stripe in ((2, 1, 16), (8, 7, 8)):
            with pkg.Context(0) as c:
                scenes[sname](c)
                c.set_partition(stripe, n_parts, part)
                c.resize(160, 192)
                c.init_output(5)
                for aname, alg in algs:
                    for cname, limit, spp, _ in COUNTS[:2]:
                        case("part%d.%d.%d/%s/%s/%s" % (n_parts, part, stripe, sname, aname, cname), lambda: c.render(cam, limit, spp, alg))
    return out


def child(out_path):
    import ctypes
    import __graft_entry__ as graft
    pkg = graft.load_package()
    stub = ctypes.CDLL(os.environ["PTMI_HIPSTUB"])
    assert stub.hipstub_is_the_stub() == 1
    stub.hipstub_set_device_size.argtypes = [ctypes.c_int, ctypes.c_ulonglong]
    stub.hipstub_set_device_size(8, 4 << 30)
    with open(out_path, "w") as f:
        json.dump(record(pkg, stub), f)


def compact(table):
    """{case: log} -> {"logs": [distinct logs], "cases": {case: index}} (most cases share their log with others)."""
    logs, index, cases = [], {}, {}
    for key in sorted(table):
        text = "\n".join(table[key])
        if text not in index:
            index[text] = len(logs)
            logs.append(table[key])
        cases[key] = index[text]
    return {"logs": logs, "cases": cases}


def run_matrix(tmp_dir):
    from test_host_sanitized import build_stub
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg._build.build_lib()
    pkg._build.build_ablations_lib()
    stub = build_stub(STUB, sanitize=None)
    out = os.path.join(tmp_dir, "launch_table.json")
    env = dict(os.environ, PTMI_HIPSTUB=stub, LD_PRELOAD=stub)
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    with open(out) as f:
        return compact(json.load(f))


def test_every_render_call_enqueues_what_the_golden_table_says(tmp_path):
    got = run_matrix(str(tmp_path))
    with open(GOLDEN) as f:
        want = json.load(f)
    assert set(got["cases"]) == set(want["cases"]), sorted(set(got["cases"]) ^ set(want["cases"]))[:10]
    differ = [k for k in sorted(want["cases"]) if got["logs"][got["cases"][k]] != want["logs"][want["cases"][k]]]
    for k in differ[:3]:
        print(k, "\n  want:", "\n    ".join(want["logs"][want["cases"][k]]), "\n  got: ", "\n    ".join(got["logs"][got["cases"][k]]))
    assert not differ, "%d of %d cases enqueue something else, e.g. %s" % (len(differ), len(want["cases"]), differ[:10])


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
    elif sys.argv[1] == "--regenerate":
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            table = run_matrix(d)
        with open(GOLDEN, "w") as f:
            json.dump(table, f, indent=0)
            f.write("\n")
        print("%d cases, %d distinct logs -> %s" % (len(table["cases"]), len(table["logs"]), GOLDEN))
