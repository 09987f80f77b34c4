"""Static check of k_physics<512>'s gfx950 code: registers, scratch bytes per lane, and the scratch / LDS / VALU instruction counts of the
solver's iteration loop (the ISA between the source lines of the loop head and of its closing stamp, via -gline-tables-only) and of the
per-pass stage functions the loop calls: the lines of the same file between the comments `// isa_check: loop stage begin` and
`// isa_check: loop stage end` (any number of such ranges).  The loop is looked for in sdx_physics.hip and the sdx_phys_*.h it includes;
code inlined from any other line of those files is not part of the loop.
usage: python tools/isa_check.py [--randomize] [--force] [--report] [extra hipcc flags...]      (cross-compiles; no GPU needed)
--report: ... for the contact-report variant k_physics<512 | SDX_PHYS_REPORT> (516; with --randomize / --force 517 .. 519)
--randomize: the same report for the domain-randomization variant k_physics<512 | SDX_PHYS_DR> (= k_physics<513>)
--force: ... for the external-wrench variant k_physics<512 | SDX_PHYS_FORCE> (514; with --randomize 515)
--osc: registers, scratch and occupancy of k_osc_torques<false> and k_osc_torques<true> (sdx_phys_osc.h) instead, nothing about the loop
--ik: the same for k_solve_ik (sdx_phys_ik.h)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "seqdex_amd", "csrc")
SRC = os.path.join(CSRC, "sdx_physics.hip")
RANDOMIZE = "--randomize" in sys.argv
if RANDOMIZE:
    sys.argv.remove("--randomize")
FORCE = "--force" in sys.argv
if FORCE:
    sys.argv.remove("--force")
REPORT = "--report" in sys.argv
if REPORT:
    sys.argv.remove("--report")
OSC = "--osc" in sys.argv
if OSC:
    sys.argv.remove("--osc")
IK = "--ik" in sys.argv
if IK:
    sys.argv.remove("--ik")
OSC_TAGS = [("k_osc_torques<false>", "k_osc_torquesILb0E"), ("k_osc_torques<true>", "k_osc_torquesILb1E")]
KEYS = ("VGPRs:", "AGPRs:", "ScratchSize [bytes/lane]:", "SGPRs Spill:", "VGPRs Spill:", "Occupancy [waves/SIMD]:", "LDS Size [bytes/block]:")
TAG = "k_physicsILi%dE" % (512 + (1 if RANDOMIZE else 0) + (2 if FORCE else 0) + (4 if REPORT else 0))
KERN = "_Z9%sEvPK8SdxConst6SdxBuf" % TAG

# the unit's files: the .hip and the private headers it includes; the one with the loop markers is where the loop's lines are counted
UNIT = ["sdx_physics.hip"] + re.findall(r'^#include "(sdx_phys_\w+\.h)"', open(SRC).read(), flags=re.M)
LOOPFILE = next(f for f in UNIT if "for (int it = it0;" in open(os.path.join(CSRC, f)).read())
src = open(os.path.join(CSRC, LOOPFILE)).read().split("\n")
lo = next(i for i, l in enumerate(src) if "for (int it = it0;" in l) + 1
hi = next(i for i, l in enumerate(src) if "SSTAMP(22);" in l and i > lo) + 1
# the loop itself, then the marked ranges of the stage functions it calls (1-based, inclusive)
begins = [i + 1 for i, l in enumerate(src) if "// isa_check: loop stage begin" in l]
ends = [i + 1 for i, l in enumerate(src) if "// isa_check: loop stage end" in l]
assert len(begins) == len(ends) and all(b < e for b, e in zip(begins, ends)), "unpaired loop stage markers in " + LOOPFILE
RANGES = [(lo, hi)] + list(zip(begins, ends))
with tempfile.TemporaryDirectory() as td:
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-gline-tables-only",
           "-Rpass-analysis=kernel-resource-usage", "-save-temps=obj", "-c", SRC, "-o", os.path.join(td, "p.o")] + sys.argv[1:]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=td)
    rem = r.stderr
    if OSC or IK:
        for name, tag in (OSC_TAGS if OSC else []) + ([("k_solve_ik", "k_solve_ikPK8SdxConst")] if IK else []):
            blk = rem[rem.index(tag):]
            print(name + ":", ", ".join("%s %s" % (key, (re.search(re.escape(key) + r"\s*(\d+)", blk) or [None, "?"])[1]) for key in KEYS))
        sys.exit(0)
    blk = rem[rem.index(TAG):]
    for key in ("VGPRs:", "ScratchSize [bytes/lane]:", "SGPRs Spill:", "VGPRs Spill:", "Occupancy [waves/SIMD]:"):
        m = re.search(re.escape(key) + r"\s*(\d+)", blk)
        print(key, m.group(1) if m else "?")
    asm = [f for f in os.listdir(td) if f.endswith("gfx950.s")][0]
    inside, cur = False, None
    loop = {"scratch": 0, "ds": 0, "valu": 0, "salu": 0, "barrier": 0, "total": 0}
    tot_scratch = 0
    seen_lo = False
    fileno, unit_nos = None, set()
    for line in open(os.path.join(td, asm)):
        if line.startswith(KERN + ":"):
            inside = True
            continue
        m = re.match(r'\s*\.file\s+(\d+)\s+"[^"]*"\s+"(?:[^"]*/)?(sdx_phys\w+\.h(?:ip)?)"', line)   # (a header's comes where its first line is used)
        if m and m.group(2) in UNIT:
            unit_nos.add(int(m.group(1)))
            if m.group(2) == LOOPFILE:
                fileno = int(m.group(1))
        if not inside:
            continue
        if ".end_amdhsa_kernel" in line or line.startswith("\t.section"):
            break
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", line)
        if m:
            if int(m.group(1)) == fileno:
                cur = int(m.group(2))
            elif int(m.group(1)) in unit_nos:   # another file of the unit: as far from the loop as another line of the loop's file
                cur = None
            continue
        t = line.strip()
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        op = t.split()[0]
        if op.startswith("scratch_"):
            tot_scratch += 1
        if cur is not None and any(a <= cur <= b for a, b in RANGES):
            loop["total"] += 1
            if op.startswith("scratch_"):
                loop["scratch"] += 1
            elif op.startswith("ds_"):
                loop["ds"] += 1
            elif op.startswith("v_"):
                loop["valu"] += 1
            elif op == "s_barrier":
                loop["barrier"] += 1
            elif op.startswith("s_"):
                loop["salu"] += 1
    print("scratch instructions in the kernel:", tot_scratch)
    print("iteration loop (%ssource lines %s):" % ("" if LOOPFILE == "sdx_physics.hip" else LOOPFILE + ", ", ", ".join("%d-%d" % r for r in RANGES)), loop)
