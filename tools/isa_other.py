#!/usr/bin/env python3
"""isa_other.py [--json] [PHASE_STATS.json] -- where the non-arithmetic quarter of render_inline_kernel's VALU instructions sits.

rocprofv3 counts a launch's VALU wave-instructions by class (SQ_INSTS_VALU_ADD_F32, ..._MUL_F32, ...); what is in none of them -- moves,
compares, selects, lane reads, the division helpers -- is the class OTHER (profiles/rNN_valu_roofline.json: mix_wave_instr_per_launch),
24.5 % of the kernel's instructions on C2 in round 5.  This tool
  1. cuts the kernel's assembly (build/isa/ptmi_inline.s, written by tools/kernel_resources.py) into basic blocks, keeps the blocks of the
     main loop (the compiler's own loop comments), and counts every block's VALU instructions by the counters' classes, OTHER by opcode;
  2. gives every block a ROLE by its signature (the sphere test holds v_min_f32 and a ds_read_b128, its candidate path the v_sqrt_f32, the
     plane test the division, the sin/cos blocks the f64 arithmetic ...) and every role its executions per launch from the WAVE-level
     counters of a -DPTMI_PHASE_STATS / -DPTMI_SPHERE_STATS build (tools/phase_stats.py: `wave_block_executions` -- exact counts of how often
     a wave runs the block on C2, 64 spp);
  3. prints OTHER per role: static opcodes, executions, wave-instructions per launch, share -- and how the sum compares with the measured
     OTHER total of the committed PMC profile.
Blocks without a signature of their own are booked under the loop's control flow at one execution per trip: an estimate, labelled so.

    isa_other.py --cycles [--isa-dir=DIR] [--json]
prices EVERY VALU opcode of the main loop with the 8-waves-per-SIMD figures of the newest profiles/rNN_valu_rates.json (2.2 cycles for
f32 add / sub / mul, moves, shifts and two-operand logic, 4.1 for compares, selects, min / max, three-operand integer ops, f64 and
conversions, 8.1 for sqrt / rcp; a v_cndmask_b32_e32 directly behind another at what tools/cndmask_probe.hip measured for the second
of such a pair), multiplies by the same executions and prints SIMD cycles per trip by role.  --isa-dir names another build/isa (a
parent's assembly) for the table before a change."""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CLASSES = ["ADD_F32", "MUL_F32", "FMA_F32", "TRANS_F32", "ADD_F64", "MUL_F64", "FMA_F64", "TRANS_F64", "CVT", "INT32", "INT64", "OTHER"]


def classify(op):
    """The counter class of one VALU opcode (gfx950 SQ_INSTS_VALU_* semantics as far as the guide states them; what matches none is OTHER)."""
    o = op
    for suffix in ("_e32", "_e64", "_dpp", "_sdwa"):
        if o.endswith(suffix):
            o = o[:-len(suffix)]
    if re.match(r"v_(pk_)?(fma|mad|mac|fmac|fmaak|fmamk|dot\d)_(f32|legacy_f32)", o) or o in ("v_fma_mix_f32",):
        return "FMA_F32"
    if re.match(r"v_(pk_)?(add|sub|subrev|min|max|min3|max3|med3)_f32", o):
        return "ADD_F32"
    if re.match(r"v_(pk_)?(mul|mul_legacy)_f32", o):
        return "MUL_F32"
    if re.match(r"v_(rcp|rsq|sqrt|sin|cos|exp|log|rcp_iflag)_(f32|legacy_f32)", o):
        return "TRANS_F32"
    if re.match(r"v_(fma|mad|fmac)_f64", o):
        return "FMA_F64"
    if re.match(r"v_(add|min|max)_f64", o):
        return "ADD_F64"
    if re.match(r"v_mul_f64", o):
        return "MUL_F64"
    if re.match(r"v_(rcp|rsq|sqrt)_f64", o):
        return "TRANS_F64"
    if re.match(r"v_cvt_", o):
        return "CVT"
    if re.match(r"v_(add|sub|subrev|mul|mad|lshl|lshr|ashr)\w*_(u64|i64|b64)", o) or o in ("v_lshlrev_b64", "v_lshrrev_b64", "v_ashrrev_i64", "v_mad_u64_u32", "v_mad_i64_i32"):
        return "INT64"
    if re.match(r"v_(add|sub|subrev|addc|subb|mul_lo|mul_hi|mul|mad|lshl|lshlrev|lshrrev|ashrrev|and|or|xor|xnor|not|bfe|bfi|alignbit|alignbyte|min|max|min3|max3|med3|"
                r"add3|lshl_add|add_lshl|lshl_or|and_or|or3|xad|perm|bcnt|ffbh|ffbl|sad)\w*_(u32|i32|b32|u16|i16|b16|u24|i24|co_u32|co_ci_u32)", o):
        return "INT32"
    return "OTHER"


def opcode_costs():
    """({exact opcode: cycles}, the class costs) from the 8-waves figures of the newest profiles/rNN_valu_rates.json"""
    import glob
    path = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_valu_rates.json")))[-1]
    ops = json.load(open(path))["results"]["waves_per_simd_8"]["ops"]
    c = {k: v["cycles"] for k, v in ops.items()}
    return path, {"two": c["v_add_f32"], "four": c["v_cndmask_b32_e64 (sgpr mask)"], "cmp": c["v_cmp_lt_f32_e64 (sgpr dst)"], "fma": c["v_fma_f32"], "fmac": c["v_fmac_f32"],
                  "cvt": c["v_cvt_f64_f32 / v_cvt_f32_f64"], "cvt_i": c["v_cvt_f32_i32"], "trans": c["v_sqrt_f32"], "max": c["v_max_f32"]}


# what a v_cndmask_b32_e32 directly behind another costs OVER the first (tools/cndmask_probe.hip: "cmp + 2 cndmask e32" 17.13 against "v_cmp vcc +
# cndmask vcc" 8.09 cycles, profiles/four_cycle_by_role.json); in real code, between other instructions' latencies, an upper bound
VCC_PAIR_SECOND = 17.13 - 8.09


def cycles_of(op, prev, k):
    """SIMD issue cycles of one VALU opcode at 8 waves per SIMD (k: opcode_costs' classes); prev: the instruction in front of it"""
    o = re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)
    if o == "v_cndmask_b32":
        return VCC_PAIR_SECOND if op.endswith("_e32") and prev.startswith("v_cndmask_b32_e32") else k["four"]
    if re.match(r"v_(sqrt|rcp|rsq|exp|log|sin|cos)_", o):
        return k["trans"]
    if o.endswith("_f64") or re.match(r"v_(cvt_f64|cvt_f32_f64|cvt_i32_f64)", o):
        return k["cvt"] if o.startswith("v_cvt") else k["four"]
    if o.startswith("v_cvt"):
        return k["cvt_i"]
    if o.startswith("v_cmp"):
        return k["cmp"]
    if re.match(r"v_(fma|mad)_f32", o):
        return k["fma"]
    if re.match(r"v_(fmac|mac)_f32", o):
        return k["fmac"]
    if re.match(r"v_(min|max|min3|max3|med3)_", o) or o.startswith("v_div_") or o.startswith("v_readlane") or o.startswith("v_readfirstlane") or o.startswith("v_writelane"):
        return k["max"]
    if re.match(r"v_(add|sub|subrev|mul)_f32$", o) or o in ("v_mov_b32", "v_add_u32", "v_sub_u32", "v_subrev_u32", "v_lshlrev_b32", "v_lshrrev_b32", "v_ashrrev_i32",
                                                          "v_xor_b32", "v_and_b32", "v_or_b32", "v_not_b32", "v_add_co_u32", "v_addc_co_u32"):
        return k["two"]
    return k["four"]                               # three-operand integer ops (add3, lshl_add, xad, alignbit, bitop3, bfe ...), mul_lo, everything unlisted


def kernel_body(sub, isa_dir=None):
    import glob
    for path in sorted(glob.glob(os.path.join(isa_dir or os.path.join(ROOT, "build", "isa"), "*.s"))):
        text = open(path).read()
        for m in re.finditer(r"^(_Z\S*):\s*;?.*?\n(.*?)\.Lfunc_end", text, re.S | re.M):
            name = m.group(1)
            if sub in name and "render" in name:
                return name, m.group(2)
    raise SystemExit("no kernel matching %r in build/isa/*.s (run tools/kernel_resources.py first)" % sub)


LOOPS = {}       # label -> the headers of the loops the block is in, outermost first (from the compiler's own comments)


def blocks_of(body):
    """[(label, [instruction lines])] in layout order; the entry block is labelled 'entry'."""
    out, label, cur = [], "entry", []
    lines = body.split("\n")
    for k, line in enumerate(lines):
        code = line.split(";")[0].rstrip()
        m = re.match(r"^(\.LBB\d+_\d+):", code)
        if m:
            out.append((label, cur))
            label, cur = m.group(1), []
            note = " ".join(l for l in lines[k:k + 4] if l.lstrip().startswith(";") or l is line)
            heads = re.findall(r"(?:Parent Loop|Header=|Loop Header:)\s*(BB\d+_\d+)?", note)
            own = ["BB" + label[4:]] if "Loop Header" in note else []
            LOOPS[label] = [h for h in re.findall(r"Parent Loop (BB\d+_\d+)", note)] + re.findall(r"Header=(BB\d+_\d+)", note) + own
            continue
        if not code.strip():
            continue
        if code.startswith("\t.") or code.startswith("."):
            continue
        cur.append(code.strip())
    out.append((label, cur))
    for lab, loops in LOOPS.items():                 # a block inside an inner loop names that loop's header only: the parents are the header's
        if loops:
            head = LOOPS.get(".L" + loops[0], [])
            if head and head[0] != loops[0]:
                LOOPS[lab] = head[:head.index(loops[0])] + loops if loops[0] in head else head + loops
    return out


def role_of(b, inner):
    ops = [i.split()[0] for i in b["code"]]
    has = lambda *names: any(any(o.startswith(n) for n in names) for o in ops)      # noqa: E731
    if has("v_cmp_class_f32") and has("v_sqrt_f32"):
        return "sqrt_slow"                         # the compiler's denormal-scaled square root: only when a lane holds 0 < x < 2^-96
    if has("v_min_f32") and has("v_cmp_ngt_f32") and has("v_cmp_gt_u32") and b["valu"] <= 26:
        return "sphere_test"                       # (until the candidates came from two compares: one compare of min(tca, x))
    if inner and ops.count("v_cmp_ngt_f32_e32") + ops.count("v_cmp_ngt_f32_e64") >= 2 and has("s_and_b64") and has("v_cmp_gt_u32") and b["valu"] <= 26 and not has("v_sqrt_f32"):
        return "sphere_test"                       # tca < 0 and d2 > r2 as two compares joined by s_and_b64; no v_min_f32, x is the stash's
    valu_ops = [o for o in ops if o.startswith("v_")]
    if inner and b["valu"] == 8 and sorted(o.rsplit("_", 1)[0] for o in valu_ops) == ["v_add_f32"] * 2 + ["v_mul_f32"] * 4 + ["v_sub_f32"] * 2:
        return "sphere_xy"                         # the x-y terms of the sphere test, skipped by a sphere that shares its predecessor's (SphereShare::kXY)
    if has("v_sqrt_f32"):
        return "sphere_candidate"                  # a dense pass of the sphere fold: every stashed lane's square root (one copy per sphere site, one behind the walk)
    if inner and b["valu"] == 3 and has("s_and_saveexec_b64") and all(o.startswith("v_mov_b32") for o in ops if o.startswith("v_")):
        return "sphere_stash"                      # a candidate lane keeps (tca, x, index): the masked block behind the sphere test
    if inner and b["valu"] in (4, 5) and sum(o.startswith("v_cndmask_b32") for o in ops) == 3 and sum(o.startswith("v_mov_b32") for o in ops) == 1 \
            and sum(o.startswith("v_sub_f32") for o in ops) == b["valu"] - 4:
        return "sphere_stash"                      # ... the same as three selects and the index's move (render Inline), with x = r2 - d2 in front of them
    if inner and has("v_cndmask_b32") and has("v_cmp_nle_f32") and b["valu"] <= 8 and not has("v_div_scale_f32"):
        return "sphere_candidate"                  # the fold update behind the square root
    if has("v_div_scale_f32") and (inner or has("v_cmp_nle_f32")):
        return "plane_test"                        # a dense pass of the plane fold: the division and the fold's compare (in the plane loop, and once behind it)
    if has("v_cvt_f64_f32") and has("v_fma_f64", "v_fmac_f64") and not has("v_cvt_i32_f64"):
        return "sincos3_fast"                      # the quadrant by comparison, all three evaluations of a shade in one block (no conversion to an integer)
    if has("v_cvt_f64_f32") or has("v_cvt_i32_f64"):
        return "sincos_reduce"
    if has("v_fma_f64", "v_fmac_f64", "v_mul_f64"):
        return "sincos_polynomial"
    if has("v_div_scale_f32"):
        return "division_fallback"                 # compiler divisions behind __all() range checks (normal of a hit, sincos of inf / NaN): rare
    if has("v_rcp_f32"):
        return "hit_normal"
    return None


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    stats_path = next((a for a in args if a.endswith(".json")), None)
    if stats_path is None:
        for tag in ("r06", "r05"):
            cand = os.path.join(ROOT, "profiles", "%s_phase_stats.json" % tag)
            if os.path.exists(cand) and "wave_block_executions" in open(cand).read():
                stats_path = cand
                break
    execs = None
    if stats_path:
        for line in open(stats_path):
            if "wave_block_executions" in line:
                execs = json.loads(line)["wave_block_executions"]
    measured = None
    for tag in ("r06", "r05"):
        cand = os.path.join(ROOT, "profiles", "%s_valu_roofline.json" % tag)
        if os.path.exists(cand):
            d = json.load(open(cand))
            measured = (tag, d["mix_wave_instr_per_launch"], d.get("build_id", d.get("source_hash")))
            break
    isa_arg = next((a for a in sys.argv[1:] if a.startswith("--isa-dir=")), None)
    name, body = kernel_body("render_inline_kernelILb1ELi8EE", isa_arg.split("=", 1)[1] if isa_arg else None)
    rates_path, klass = opcode_costs()
    blocks = blocks_of(body)
    main_header = max(set(h[0] for h in LOOPS.values() if h), key=lambda hd: sum(1 for h in LOOPS.values() if h and h[0] == hd))
    table = []
    for label, code in blocks:
        loops = LOOPS.get(label, [])
        if not loops or loops[0] != main_header:
            continue
        counts = dict.fromkeys(CLASSES, 0)
        other_ops = {}
        cycles, four, prev = 0.0, 0, ""
        for ins in code:
            op = ins.split()[0]
            if op.startswith("v_"):
                cost = cycles_of(op, prev, klass)
                cycles += cost
                four += cost > 3.0 and not op.startswith(("v_sqrt", "v_rcp"))
                cls = classify(op)
                counts[cls] += 1
                if cls == "OTHER":
                    key = re.sub(r"_(e32|e64)$", "", op)
                    other_ops[key] = other_ops.get(key, 0) + 1
            if not op.startswith("s_nop") and not op.startswith(";"):
                prev = op
        table.append({"label": label, "code": code, "valu": sum(counts.values()), "counts": counts, "other_ops": other_ops, "inner": len(loops) > 1,
                      "cycles": cycles, "four_cycle": four})
    roles = {}
    order = ["sphere_test", "sphere_xy", "sphere_stash", "sphere_candidate", "plane_test", "sincos3_fast", "sincos_reduce", "sincos_polynomial", "hit_normal", "rest_of_loop", "sqrt_slow", "division_fallback"]
    for b in table:
        r = role_of(b, b["inner"]) or "rest_of_loop"
        roles.setdefault(r, []).append(b)
    # executions of ONE copy of a role's code per launch.  A role with k copies in the kernel (unrolled sites, the three sin/cos evaluations) runs
    # each copy (role executions / k) times; all copies hold the same instructions, so instructions per launch = mean static count x role executions
    e = execs or {}
    # a kernel with the three-angle fast form runs sincos()'s blocks only in the shade rounds whose vote leaves it (tools/sincos_stats.py
    # counts them; a --slow-rounds=N argument, else the share it measured on C2, 0.27: S16 holds a Glossy sphere with p = 1, whose half angles are all 0)
    fast_form = any(role_of(b, b["inner"]) == "sincos3_fast" for b in table)
    slow_arg = next((a for a in sys.argv[1:] if a.startswith("--slow-rounds=")), None)
    slow_rounds = (float(slow_arg.split("=")[1]) if slow_arg else 0.27 * e.get("shade", 0.0)) if fast_form else e.get("shade", 0.0)
    role_execs = {"sphere_test": e.get("sphere_tests"), "sphere_xy": e["sphere_tests"] - e["sphere_shared"] if "sphere_tests" in e and "sphere_shared" in e else None,   # (unknown without the shared-test counter)
                  "sphere_stash": e.get("sphere_sqrt_path"),
                  "sphere_candidate": e.get("sphere_passes", e.get("sphere_sqrt_path")), "plane_test": e.get("plane_passes", e.get("plane_division_path")),
                  "sincos3_fast": e["shade"] - slow_rounds if e else None, "sincos_reduce": 3 * slow_rounds if e else None,
                  "sincos_polynomial": 3 * slow_rounds if e else None, "hit_normal": None,
                  "rest_of_loop": e.get("trips"), "sqrt_slow": 0, "division_fallback": 0}
    what = {"sphere_test": "distanceTo @Sphere, the part every lane runs at every sphere (lz, tca, d2, x, the candidate test)",
            "sphere_xy": "... its x-y terms (lx, ly, lx dx + ly dy, lx lx + ly ly): every sphere but those that share their predecessor's cx and cy", "sphere_stash": "... a test with a candidate lane: the lane keeps (tca, x, index), three moves under the candidates' mask, or three selects and a move",
            "sphere_candidate": "... a dense pass: square root, t and the fold update of every lane that holds a stash (before the plane fold: once per test with a candidate)",
            "plane_test": "distanceTo @Plane: a dense pass of the plane fold (each lane on its own stashed plane), IEEE division and fold update", "sincos_reduce": "sin/cos: argument reduction (f64), three per shade (with the fast form: per shade round that leaves it)",
            "sincos3_fast": "sin/cos of a shade's three half angles, quadrant by comparison: cvt, hpi - |x|, selects, the two f64 polynomials (the vote's 6 instructions sit with the draws, in rest_of_loop)",
            "sincos_polynomial": "sin/cos: the two f64 polynomials, sign and swap by bit operations", "hit_normal": "hit: the sphere normal's three divisions by one length",
            "rest_of_loop": "everything else in the loop, booked at ONE execution per trip: flags and masks, frozen check and finish, restart, draws, rotation, apply_bounce",
            "sqrt_slow": "compiler's scaled square root (a lane with 0 < x < 2^-96): practically never", "division_fallback": "compiler divisions behind range checks (huge or zero operands, inf / NaN): practically never"}
    # copies per role: sphere and plane tests are counted per TEST, a test runs one copy; sin/cos roles per evaluation
    out_rows, total = [], 0.0
    for r in order:
        bs = roles.get(r, [])
        if not bs:
            continue
        valu = sum(b["valu"] for b in bs)
        other = sum(b["counts"]["OTHER"] for b in bs)
        ops = {}
        for b in bs:
            for k, v in b["other_ops"].items():
                ops[k] = ops.get(k, 0) + v
        if r in ("sphere_test", "sphere_xy"):
            copies = len(bs)
        elif r == "sphere_stash":
            copies = len(bs)
        elif r == "sphere_candidate":                            # (with dense passes: one more copy behind the walk)
            copies = max(1, len(roles.get("sphere_test", [])) + (1 if roles.get("sphere_stash") else 0))
        elif r == "plane_test":
            copies = max(1, sum(1 for b in bs if any(i.startswith("v_div_fixup") for i in b["code"])))
        elif r in ("sincos_reduce", "sincos_polynomial"):
            copies = 3
        elif r == "sincos3_fast":
            copies = len(bs)
        else:
            copies = 1
        if r == "hit_normal":
            n_exec = e.get("trace") if e else None               # at most once per trace (a sphere hit with a normal to normalise)
        else:
            n_exec = role_execs.get(r)
        dyn = None if n_exec is None else other / copies * n_exec
        dyn_valu = None if n_exec is None else valu / copies * n_exec
        cyc = sum(b["cycles"] for b in bs)
        trips = e.get("trips")
        if dyn:
            total += dyn
        out_rows.append({"role": r, "what": what[r], "blocks": len(bs), "copies": copies, "static_valu": valu, "static_other": other, "other_opcodes": ops,
                         "executions_per_launch": n_exec, "other_wave_instr_per_launch": dyn, "valu_wave_instr_per_launch": dyn_valu,
                         "static_cycles": round(cyc, 1), "static_four_cycle_instr": sum(b["four_cycle"] for b in bs),
                         "cycles_per_execution": round(cyc / copies, 1),
                         "cycles_per_trip": None if n_exec is None or not trips else round(cyc / copies * n_exec / trips, 1),
                         "valu_per_trip": None if n_exec is None or not trips else round(valu / copies * n_exec / trips, 1)})
    if "--cycles" in sys.argv:
        print("kernel ...%s: main loop %s; opcode costs from %s (8 waves per SIMD); wave-level executions from %s" % (name[-48:], main_header, os.path.relpath(rates_path, ROOT), stats_path))
        print("%-18s %6s %7s %14s %10s %12s %12s" % ("role", "VALU", "4-cycle", "executions", "cyc / exec", "VALU / trip", "cycles / trip"))
        for row in out_rows:
            print("%-18s %6d %7d %14s %10.1f %12s %12s" % (row["role"], row["static_valu"], row["static_four_cycle_instr"],
                  "%.0f" % row["executions_per_launch"] if row["executions_per_launch"] is not None else "-", row["cycles_per_execution"],
                  row["valu_per_trip"] if row["valu_per_trip"] is not None else "-", row["cycles_per_trip"] if row["cycles_per_trip"] is not None else "-"))
        print("sum %.0f VALU instructions and %.0f SIMD cycles per trip (roles with known executions)" % (
              sum(r["valu_per_trip"] or 0 for r in out_rows), sum(r["cycles_per_trip"] or 0 for r in out_rows)))
        if "--json" in sys.argv:
            print(json.dumps({"kernel": name, "main_loop": main_header, "opcode_costs": os.path.relpath(rates_path, ROOT), "wave_block_executions": execs,
                              "roles": [{k: r[k] for k in ("role", "blocks", "copies", "static_valu", "static_four_cycle_instr", "executions_per_launch", "cycles_per_execution", "valu_per_trip", "cycles_per_trip")} for r in out_rows],
                              "valu_per_trip": sum(r["valu_per_trip"] or 0 for r in out_rows), "cycles_per_trip": sum(r["cycles_per_trip"] or 0 for r in out_rows)}))
        return
    print("kernel ...%s: main loop %s, %d blocks; wave-level executions from %s" % (name[-48:], main_header, len(table), stats_path))
    print("%-18s %4s %6s %6s %14s %14s %7s  %s" % ("role", "blk", "VALU", "OTHER", "executions", "OTHER / launch", "share", "OTHER opcodes (static, all copies)"))
    for row in out_rows:
        dyn = row["other_wave_instr_per_launch"]
        print("%-18s %4d %6d %6d %14s %14s %6s  %s" % (row["role"], row["blocks"], row["static_valu"], row["static_other"],
              "%.0f" % row["executions_per_launch"] if row["executions_per_launch"] is not None else "-", "%.0f" % dyn if dyn is not None else "-",
              "%.1f%%" % (100.0 * dyn / total) if dyn else "-", " ".join("%s:%d" % kv for kv in sorted(row["other_opcodes"].items(), key=lambda kv: -kv[1]))))
    if measured:
        print("sum %.0f M OTHER wave-instructions per launch; the PMC profile profiles/%s_valu_roofline.json (binary %s) measured %.0f M" % (total / 1e6, measured[0], measured[2], measured[1]["OTHER"] / 1e6))
    if "--json" in sys.argv:
        print(json.dumps({"kernel": name, "main_loop": main_header, "wave_block_executions": execs, "roles": out_rows, "sum_other": total,
                          "measured_other": measured[1]["OTHER"] if measured else None, "measured_in": measured[0] if measured else None}))


if __name__ == "__main__":
    main()
