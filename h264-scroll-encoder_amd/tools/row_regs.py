#!/usr/bin/env python3
"""row_regs.py -- register budget and spill traffic of k_dyn_row, without a GPU.

    python h264-scroll-encoder_amd/tools/row_regs.py [-D...] [--src FILE] [--keep OUT.s | --listing IN.s]
                                                     [--inst TEXT] [--phase N]

Compiles csrc/dyn_kernels.hip device-only to gfx950 assembly with the
Makefile's flags (plus any -D given) and prints, for every k_dyn_row
instantiation:
  * the code object's metadata (SGPRs, VGPRs, spills, private segment, LDS);
  * per barrier-delimited phase (phase n = the code between the n-th and the
    n+1-th s_barrier in program order) the number of VALU and SALU
    instructions, of the lane operations (v_readlane_b32 / v_writelane_b32)
    an SGPR spilled to a VGPR lane turns into, of the branch / wait / control
    instructions (ctl) and of the memory instructions (mem: LDS, buffer,
    global, scalar loads);
  * per loop (a backward branch to a label) the same counts with the source
    lines of dyn_kernels.hip the loop's instructions come from, so a loop
    that reloads or saves a spilled value is named.
The counts are static: one per instruction in the listing, whatever its trip
count.  --inst keeps the instantiations whose name holds TEXT (e.g. "<false,
false>"); --phase N lists only the loops inside phase N (3 is the CAVLC
stretch of the normal path: sort scatter's barrier to the records' one), so
two revisions' level loops can be set side by side.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
LANE = ("v_readlane_b32", "v_writelane_b32")
SMEM = ("s_load_", "s_buffer_load_", "s_memrealtime", "s_memtime")
# scalar instructions that are neither ALU nor memory: waits, control, messages
SCTL = ("s_waitcnt", "s_barrier", "s_nop", "s_endpgm", "s_sleep", "s_branch", "s_cbranch", "s_swappc",
        "s_setpc", "s_getpc", "s_sendmsg", "s_setprio", "s_code_end", "s_inst_prefetch", "s_trap", "s_sethalt")
META = (".sgpr_count", ".sgpr_spill_count", ".vgpr_count", ".vgpr_spill_count", ".agpr_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size", ".wavefront_size")


def compile_asm(src, defs, out):
    rocm = os.environ.get("ROCM", "/opt/rocm")
    cmd = [os.path.join(rocm, "bin", "hipcc"), "-O3", "-g", "-fPIC", "--offload-arch=gfx950", "-Wall", "-std=c++17",
           "-munsafe-fp-atomics", *defs, "-I" + os.path.join(PKG, "..", "include"), "-I" + os.path.join(PKG, "csrc"),
           "--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True)


def demangle(names):
    try:
        p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, p.stdout.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kind(m):
    if m in LANE:
        return "lane"
    if m.startswith("v_"):
        return "valu"
    if m.startswith("s_"):
        if m.startswith(SMEM):
            return "smem"
        if m.startswith(SCTL):
            return "sctl"
        return "salu"
    return "mem"                                    # ds_, buffer_, global_, flat_, scratch_


def parse_body(lines, files):
    """[(mnemonic, operands, line of the source file or 0)], {label: index}; files: its .file numbers"""
    ins, labels, line = [], {}, 0
    for ln in lines:
        s = ln.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            line = int(m.group(2)) if m.group(1) in files else 0
            continue
        m = re.match(r"(\.LBB\d+_\d+):", s)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        if not s or s[0] in ".;/" or s.endswith(":"):
            continue
        s = s.split(";")[0].strip()
        p = s.split(None, 1)
        ins.append((p[0], p[1] if len(p) > 1 else "", line))
    return ins, labels


def count(ins):
    c = collections.Counter(kind(m) for m, _, _ in ins)
    c["valu"] += c["lane"]                            # lane operations issue as VALU
    return c


def fmt(c):
    return "VALU %5d  SALU %5d  lane ops %4d  ctl %4d  mem %4d" % (c["valu"], c["salu"], c["lane"], c["sctl"],
                                                                   c["mem"] + c["smem"])


def report(name, lines, meta, files, only_phase=None):
    ins, labels = parse_body(lines, files)
    print("== " + name)
    for k in META:
        if k in meta:
            print("   %-30s %s" % (k, meta[k]))
    print("   body: %d instructions, %s" % (len(ins), fmt(count(ins))))
    ph, cur, bounds, start = [], [], [], 0
    for n, i in enumerate(ins):
        if i[0] == "s_barrier":
            ph.append(cur)
            bounds.append((start, n))
            cur, start = [], n + 1
        else:
            cur.append(i)
    ph.append(cur)
    bounds.append((start, len(ins)))
    print("   phases (between s_barrier instructions, program order):")
    for n, p in enumerate(ph):
        src = sorted({l for _, _, l in p if l})
        span = "lines %d-%d" % (src[0], src[-1]) if src else ""
        print("     %2d: %5d instr  %s  %s" % (n, len(p), fmt(count(p)), span))
    loops = {}                                      # header -> its last backward branch
    for i, (m, ops, _) in enumerate(ins):
        if m.startswith(("s_cbranch", "s_branch")) and ops.strip() in labels and labels[ops.strip()] <= i:
            loops[labels[ops.strip()]] = i
    print("   loops (a label with backward branches to it; nested loops count in their parents too):")
    for a, b in sorted(loops.items()):
        if only_phase is not None and not (only_phase < len(bounds) and bounds[only_phase][0] <= a and
                                           b < bounds[only_phase][1]):
            continue
        body = ins[a:b + 1]
        src = collections.Counter(l for _, _, l in body if l)
        top = sorted(l for l, _ in src.most_common(3))
        lo, hi = (min(src), max(src)) if src else (0, 0)
        print("     instr %5d-%5d: %5d instr  %s  lines %d-%d (mostly %s)" %
              (a, b, len(body), fmt(count(body)), lo, hi, ", ".join(map(str, top))))
    print()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--src", default=os.path.join(PKG, "csrc", "dyn_kernels.hip"))
    ap.add_argument("--keep", help="keep the assembly listing here")
    ap.add_argument("--listing", help="read this listing instead of compiling")
    ap.add_argument("--kernel", default="k_dyn_row", help="kernels whose name holds this (default k_dyn_row)")
    ap.add_argument("--inst", help="only the instantiations whose demangled name holds this")
    ap.add_argument("--phase", type=int, help="list only the loops inside this phase")
    args, defs = ap.parse_known_args()
    with tempfile.TemporaryDirectory() as td:
        out = args.listing or args.keep or os.path.join(td, "dyn_kernels.s")
        if not args.listing:
            compile_asm(args.src, defs, out)
        text = open(out).read().split("\n")
    # metadata: the amdhsa.kernels YAML at the end of the listing
    # (one list entry per kernel; its own keys are indented by four columns)
    metas, cur = {}, {}
    for ln in text:
        m = re.match(r"  (?:- |  )(\.[a-z_]+):\s*(\S*)", ln)
        if not m:
            continue
        if ln.startswith("  - "):
            cur = {}
        cur[m.group(1)] = m.group(2)
        if m.group(1) == ".symbol":
            metas[m.group(2).strip("'\"")[:-len(".kd")]] = cur
    base = os.path.basename(args.src)
    files = {m.group(1) for m in (re.match(r'\s*\.file\s+(\d+)\s.*"([^"]*)"(?:\s+md5.*)?$', ln) for ln in text)
             if m and os.path.basename(m.group(2)) == base}
    names = demangle([k for k in metas if args.kernel in k])
    syms = [k for k in names if re.search(r"\b" + re.escape(args.kernel) + r"\b", names[k])
            and (not args.inst or args.inst in names[k])]
    for sym in sorted(syms, key=lambda k: names[k]):
        a = next(i for i, ln in enumerate(text) if ln.startswith(sym + ":"))
        b = next(i for i in range(a, len(text)) if text[i].strip().startswith(".Lfunc_end"))
        report(re.sub(r"^void |\(anonymous namespace\)::|\(.*$", "", names[sym]), text[a + 1:b], metas[sym], files, args.phase)
    if not syms:
        sys.exit("no kernel named *%s* in the listing" % args.kernel)


if __name__ == "__main__":
    main()
