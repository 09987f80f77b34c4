"""Static instruction counts of k_update_persistent<false> per interval of its phase clock, for one or two builds.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -S --cuda-device-only seqdex_amd/csrc/sdxp_persist.hip -o result.s
    python tools/isa_intervals.py parent.s result.s

The kernel's text is cut at the s_memtime of every TS(i) (in text order: a block the compiler moved behind the loop is counted where it stands).
Per interval: VALU instructions, ds_read*, s_waitcnt with lgkmcnt(0), and v_mul_f32 / v_fma_f32 / v_fmac_f32 (a change that must keep every
rounding keeps these three).  Counts, not timings."""
import re
import sys

NAMES = ["prologue", "A:dY0 gather+gram+ctl", "A:adam L0", "A:stage+fwd0", "sh1:adam L1", "wait x1", "B:fwd1", "sh2:adam L2/heads", "wait x2", "C:fwd2",
         "sh3:gram x2, x1", "wait hw+x3", "D:head fwd", "D:losses,dmu", "D:bwd heads", "D:B1", "sh4:stats,grams,hterm", "wait dY1", "E:B0", "sh5:gram dY1",
         "epilogue"]
COLS = ["VALU", "ds_read*", "lgkmcnt(0)", "v_mul_f32", "v_fma_f32", "v_fmac_f32"]


def intervals(path, kernel="_Z19k_update_persistentILb0EE"):
    out, cur, inside = [], None, False
    for line in open(path):
        t = line.strip()
        if not inside:
            if re.match(re.escape(kernel) + r"\w*:", t):
                inside, cur = True, dict.fromkeys(COLS, 0)
            continue
        if t.startswith(".Lfunc_end"):
            break
        op = t.split()[0] if t else ""
        if op == "s_memtime":
            out.append(cur)
            cur = dict.fromkeys(COLS, 0)
        elif op.startswith("v_"):
            cur["VALU"] += 1
            base = re.sub(r"_(e32|e64|dpp|sdwa|e64_dpp)$", "", op)
            if base in cur:
                cur[base] += 1
        elif op.startswith("ds_read"):
            cur["ds_read*"] += 1
        elif op == "s_waitcnt" and "lgkmcnt(0)" in t:
            cur["lgkmcnt(0)"] += 1
    out.append(cur)
    return out


def main():
    builds = [intervals(p) for p in sys.argv[1:3]]
    n = len(builds[0])
    assert all(len(b) == n for b in builds), [len(b) for b in builds]
    names = NAMES if n == len(NAMES) else ["interval %d" % i for i in range(n)]
    print("%-24s" % "interval" + "".join("%16s" % c for c in COLS))
    tot = [dict.fromkeys(COLS, 0) for _ in builds]
    for i in range(n):
        print("%-24s" % names[i] + "".join("%16s" % " -> ".join("%d" % b[i][c] for b in builds) for c in COLS))
        for t, b in zip(tot, builds):
            for c in COLS:
                t[c] += b[i][c]
    print("%-24s" % "total" + "".join("%16s" % " -> ".join("%d" % t[c] for t in tot) for c in COLS))


if __name__ == "__main__":
    main()
