"""Is the device code of two trees the same?  Every .hip of seqdex_amd/csrc of this tree and of another checkout (the parent commit, say)
is compiled for gfx950 with the Makefile's flags plus -save-temps=obj; for every kernel (.amdhsa_kernel) the instruction text from its
label to .end_amdhsa_kernel, the .amdhsa_* resource lines included, must be the same on both sides, and neither side may have a kernel
the other lacks.  Kernels are matched by symbol across all files of a side: one that changed files is reported as `moved a.hip -> b.hip`
next to its verdict, not as dropped and added.  Comments, debug / .loc / .file lines, the function numbers inside local labels and the order of the symbols are ignored.

    git worktree add /tmp/parent HEAD~1      (a whole checkout: the sources include ../../include/seqdex.h)
    python tools/kernel_identity.py /tmp/parent/seqdex_amd/csrc [--out profiles/kernel_identity.txt] [--work DIR] [--jobs 8] [--flags "-DSDX_PHASE_CLOCK"]

--flags: extra hipcc flags appended on both sides (the profiling builds: "-DSDX_PHASE_CLOCK", "-DSDX_PHASE_CLOCK -DSDX_LANE_CLOCK"); give
each set of flags a --work of its own.  --ignore-kernarg-size: the .amdhsa_kernarg_size line is left out of the comparison and a kernel whose
size changed says so next to its verdict (a struct passed by value - SdxBuf - grew at its end: the offsets of everything in front of the
new fields, and so every instruction, stay what they were).  Cross-compiles; no GPU needed.  --work keeps the assembly between runs (a side is recompiled when one of its sources is newer).  Exit 1 on a difference."""
import argparse
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def makefile_flags(csrc):
    """(CXXFLAGS, {file: FLAGS_<file>}) of csrc/Makefile, $(ARCH) resolved: both sides are compiled the way THIS tree's library is built"""
    txt = open(os.path.join(csrc, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", txt, flags=re.M))
    return var["CXXFLAGS"].replace("$(ARCH)", var["ARCH"]).split(), {k[6:]: v.split() for k, v in var.items() if k.startswith("FLAGS_")}


FLAGS, EXTRA = makefile_flags(os.path.join(ROOT, "seqdex_amd", "csrc"))


def compile_one(csrc, name, out, extra=()):
    os.makedirs(out, exist_ok=True)
    asm = glob.glob(os.path.join(out, name + "-hip-amdgcn-*gfx950*.s"))
    newest = max(os.path.getmtime(f) for f in glob.glob(os.path.join(csrc, "*.h*")))
    if not asm or os.path.getmtime(asm[0]) < newest:
        cmd = ["/opt/rocm/bin/hipcc"] + FLAGS + EXTRA.get(name, []) + list(extra) + ["-save-temps=obj", "-c", os.path.join(csrc, name + ".hip"), "-o", os.path.join(out, name + ".o")]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=out)
        if r.returncode != 0:
            raise RuntimeError("%s: %s" % (name, r.stderr[-2000:]))
        asm = glob.glob(os.path.join(out, name + "-hip-amdgcn-*gfx950*.s"))
    return asm[0]


KERNARG = re.compile(r"^\.amdhsa_kernarg_size (\d+)$", flags=re.M)


def kernels(asm):
    """{kernel symbol: normalised text from its label to .end_amdhsa_kernel}"""
    lines = open(asm).read().split("\n")
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    label = [l.split(";")[0].strip() for l in lines]
    start = {l[:-1]: i for i, l in enumerate(label) if l.endswith(":") and l[:-1] in names}
    out = {}
    for k in names:
        body = []
        for l in lines[start[k] + 1:]:
            t = l.split(";")[0].strip()
            if t and not re.match(r"\.(loc|file|cfi_\w+|Ltmp\d+:|Lfunc_(begin|end)\d+:)", t):
                body.append(re.sub(r"\.L(BB|JTI)\d+_", r".L\1_", re.sub(r"\s+", " ", t)))
            if t == ".end_amdhsa_kernel":
                break
        out[k] = "\n".join(body)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other", help="seqdex_amd/csrc of the tree to compare against")
    ap.add_argument("--out", default="")
    ap.add_argument("--work", default="")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--flags", default="", help="extra hipcc flags for every file of both sides")
    ap.add_argument("--ignore-kernarg-size", action="store_true", help="compare everything but .amdhsa_kernarg_size; report the sizes that changed")
    argv = sys.argv[1:]
    if "--flags" in argv[:-1]:   # (argparse takes a lone value that begins with "-" for an option: hand it over as --flags=VALUE)
        i = argv.index("--flags")
        argv[i:i + 2] = ["--flags=" + argv[i + 1]]
    a = ap.parse_args(argv)
    mine = os.path.join(ROOT, "seqdex_amd", "csrc")
    work = a.work or tempfile.mkdtemp(prefix="kernel_identity_")
    sides = (("other", a.other), ("this", mine))
    files = {side: sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(d, "*.hip"))) for side, d in sides}
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        fut = {(side, n): ex.submit(compile_one, d, n, os.path.join(work, side, n), a.flags.split()) for side, d in sides for n in files[side]}
        asm = {k: f.result() for k, f in fut.items()}
    # {(file, symbol): text} per side; a kernel is matched in its own file first (two files may each have a static kernel of one name),
    # then by symbol across all files of a side when exactly one of that name is left over on either side: it moved
    found = {side: {(n, k): text for (s, n), path in asm.items() if s == side for k, text in kernels(path).items()} for side, _ in sides}
    ko, kt = found["other"], found["this"]
    pairs = [(fk, fk) for fk in sorted(set(ko) & set(kt))]
    left_o, left_t = sorted(set(ko) - set(kt)), sorted(set(kt) - set(ko))
    for sym in sorted(set(k for _, k in left_o + left_t)):
        o, t = [fk for fk in left_o if fk[1] == sym], [fk for fk in left_t if fk[1] == sym]
        pairs += [(o[0], t[0])] if len(o) == 1 and len(t) == 1 else [(fk, None) for fk in o] + [(None, fk) for fk in t]
    report, bad, nmoved = [], 0, 0
    strip = (lambda text: KERNARG.sub(".amdhsa_kernarg_size -", text)) if a.ignore_kernarg_size else (lambda text: text)
    for o, t in sorted(pairs, key=lambda p: p[1] or p[0]):
        verdict = "identical" if o and t and strip(ko[o]) == strip(kt[t]) else ("DIFFERS" if o and t else ("ADDED" if t else "DROPPED"))
        bad += verdict != "identical"
        moved = "   moved %s.hip -> %s.hip" % (o[0], t[0]) if o and t and o[0] != t[0] else ""
        nmoved += bool(moved)
        if verdict == "identical" and ko[o] != kt[t]:
            moved += "   kernarg size %s -> %s" % (KERNARG.search(ko[o]).group(1), KERNARG.search(kt[t]).group(1))
        report.append("%-18s %-10s %s%s" % ((t or o)[0] + ".hip", verdict, (t or o)[1], moved))
    report.append("%d kernels, %d not identical, %d moved" % (len(report), bad, nmoved))
    text = "\n".join(report) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/kernel_identity.py <csrc of the parent commit>: gfx950 instruction text + .amdhsa_* resources per kernel, parent vs this tree%s%s\n" % (a.flags and "; extra flags on both sides: " + a.flags, "; .amdhsa_kernarg_size not compared (--ignore-kernarg-size)" if a.ignore_kernarg_size else "") + text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
