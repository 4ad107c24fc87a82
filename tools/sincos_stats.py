#!/usr/bin/env python3
"""sincos_stats.py -- how many of C2's shade rounds leave the three-angle fast sin/cos?  Loads (building it first if it is missing or
stale: build it BEFORE going to the GPU box) a -DPTMI_SINCOS_STATS copy of libptmi -- diagnostic, never the measured library -- renders
C2 once with render_inline_kernel (1080p, 64 spp, limit 8, S16) and prints the wave-level counts of sincos3_probe (csrc/ptmi_device.h):
shade rounds, and those in which a lane held an angle the quadrant form does not cover.  On S16 that can only be |y| < 2^-12: the half
angles are hk * rv with hk <= pi/2, |rv| < 1.  For a Matte hit that is one angle in ~6 000; but hk = (1 - p) / 2 of a Glossy surface is small
(0.05 and 0.1 on S16) and 0 for the Glossy sphere with p = 1, every hit of which draws three zero angles: 27 % of C2's rounds hold such a lane.
Those rounds now stay in the fast form and run its fix-up (counter [29]); only an angle beyond +-T2, inf or NaN leaves it ([31])."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

FLAGS = ["-DPTMI_SINCOS_STATS"]


def library(pkg):
    out = os.path.join(ROOT, "build", "diag", "libptmi_sincos_stats.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if pkg._build.is_stale(out, FLAGS):
        pkg._build.build_lib(out=out, extra_flags=FLAGS)
    return out


def main():
    pkg = graft.load_package()
    out = library(pkg)
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        print(out)
        return
    pkg.binding._lib = None
    pkg.binding.load_library(out)
    sp, pl = pkg.world.scene16()
    w, h, spp = 1920, 1080, 64
    with pkg.Context(0) as ctx:
        ctx.set_scene(sp, pl)
        ctx.resize(w, h)
        ctx.init_output(0x5EED1234)
        ctx.reset_stats()
        ctx.render(pkg.world.initial_camera(), 8, spp)
        raw = ctx.debug_counters().astype("uint32")
    rounds, slow, fixed = int(raw[30]), int(raw[31]), int(raw[29])
    # the three outcomes of the vote: three sincos() (an angle beyond +-T2, inf or NaN), the quadrant form with the fix-up for angles below
    # 2^-12, the quadrant form alone
    print(json.dumps({"build_id": pkg.load_library().build_id, "workload": "C2: 1920x1080, 64 spp, limit 8, S16, render Inline",
                      "wave_shade_rounds": rounds, "rounds_leaving_the_fast_form": slow, "fraction": slow / max(rounds, 1),
                      "rounds_in_the_fast_form_with_the_tiny_fixup": fixed, "fixup_fraction": fixed / max(rounds, 1),
                      "rounds_in_the_fast_form_alone": rounds - slow - fixed}))


if __name__ == "__main__":
    main()
