"""Is the device code of two trees the same?  Every .hip of seqdex_amd/csrc of this tree and of another checkout (the parent commit, say)
is compiled for gfx950 with the Makefile's flags plus -save-temps=obj; for every kernel (.amdhsa_kernel) the instruction text from its
label to .end_amdhsa_kernel, the .amdhsa_* resource lines included, must be the same on both sides, and neither side may have a kernel
the other lacks.  Comments, debug / .loc / .file lines, the function numbers inside local labels and the order of the symbols are ignored.

    git worktree add /tmp/parent HEAD~1      (a whole checkout: the sources include ../../include/seqdex.h)
    python tools/kernel_identity.py /tmp/parent/seqdex_amd/csrc [--out profiles/kernel_identity.txt] [--work DIR] [--jobs 8]

Cross-compiles; no GPU needed.  --work keeps the assembly between runs (a side is recompiled when one of its sources is newer).  Exit 1 on a difference."""
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


def compile_one(csrc, name, out):
    os.makedirs(out, exist_ok=True)
    asm = glob.glob(os.path.join(out, name + "-hip-amdgcn-*gfx950*.s"))
    newest = max(os.path.getmtime(f) for f in glob.glob(os.path.join(csrc, "*.h*")))
    if not asm or os.path.getmtime(asm[0]) < newest:
        cmd = ["/opt/rocm/bin/hipcc"] + FLAGS + EXTRA.get(name, []) + ["-save-temps=obj", "-c", os.path.join(csrc, name + ".hip"), "-o", os.path.join(out, name + ".o")]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=out)
        if r.returncode != 0:
            raise RuntimeError("%s: %s" % (name, r.stderr[-2000:]))
        asm = glob.glob(os.path.join(out, name + "-hip-amdgcn-*gfx950*.s"))
    return asm[0]


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
    a = ap.parse_args()
    mine = os.path.join(ROOT, "seqdex_amd", "csrc")
    work = a.work or tempfile.mkdtemp(prefix="kernel_identity_")
    files = sorted(set(os.path.basename(f)[:-4] for d in (mine, a.other) for f in glob.glob(os.path.join(d, "*.hip"))))
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        fut = {(side, n): ex.submit(compile_one, d, n, os.path.join(work, side, n)) for side, d in (("other", a.other), ("this", mine)) for n in files}
        asm = {k: f.result() for k, f in fut.items()}
    report, bad = [], 0
    for n in files:
        ko, kt = kernels(asm[("other", n)]), kernels(asm[("this", n)])
        for k in sorted(set(ko) | set(kt)):
            verdict = "identical" if ko.get(k) == kt.get(k) else ("DIFFERS" if k in ko and k in kt else ("ADDED" if k in kt else "DROPPED"))
            bad += verdict != "identical"
            report.append("%-18s %-10s %s" % (n + ".hip", verdict, k))
    report.append("%d kernels, %d not identical" % (len(report), bad))
    text = "\n".join(report) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# python tools/kernel_identity.py <csrc of the parent commit>: gfx950 instruction text + .amdhsa_* resources per kernel, parent vs this tree\n" + text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
