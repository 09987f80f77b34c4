"""Times the sim snapshot calls (include/seqdex.h sdx_state_*) against the only route a tree without them has: one
torch copy per tensor view.  save_all, restore_all and a clone of env 0 into every other env of its class, at N = 1 024 and N = 4 096,
with HIP events: warm-up, then `--repeats` timed windows of `--batch` back-to-back calls each; median and [min, max] of the per-call time.
On a tree whose library has no sdx_state_* the tool times the baseline alone.  Bytes = what the copy has to read plus write (the state
tensors with the warm-start rows up to their counts), reported over the time as a share of the 8 TB/s HBM peak.

    python tools/bench_state.py [--sizes 1024 4096] [--repeats 30] [--batch 10] [--out profiles/state_snapshot_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seqdex_amd.sim import SdxSim  # noqa: E402

# the tensor views that are state (the per-tensor route copies each of them): per-env rows, then the global ones
ENV = ["ROOT", "DOF", "RB", "CONTACT", "JAC_EEF", "TARGETS", "PREV_TARGETS", "OBS", "STATES", "OBS_CLAMPED", "STATES_CLAMPED", "REW", "RESET",
       "PROGRESS", "RANDOMIZE", "ACTIONS", "INIT_POS", "INIT_ROT", "SUCCESSES", "META_REW", "FINGER_DIST", "TVALUE", "ARM_CONTACTS",
       "STUDENT_OBS", "SUCCESS_BUF", "PILE_CHOICE", "NCONTACTS", "INSERT_AUX", "SEG_PIXELS", "EMERGENCE", "JACOBIAN", "WARM_COUNT", "CAM_ROT",
       "DR_DOF", "DR_LINK", "DR_BRICK", "WARM_KEYS", "WARM_LAMBDA"]
GLOBAL = ["CONS_SUCCESSES", "DR_GRAVITY", "DR_FRAME"]
PEAK = 8.0e12


def timed(fn, repeats, batch, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / batch)      # microseconds per call
    return out


def summary(us):
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "n": len(us)}


def bench(n, repeats, batch):
    s = SdxSim(n, device="cuda:0", seed=22)
    g = torch.Generator().manual_seed(0)
    for _ in range(4):                                           # a contact-rich state with filled warm-start caches
        s.step((torch.rand(n, 23, generator=g) * 2 - 1).cuda())
    torch.cuda.synchronize()
    views = {k: s.tensor(k) for k in ENV + GLOBAL}
    rows = {k: views[k].view(n, -1) for k in ENV}
    count = s.WARM_COUNT.cpu().long()
    fixed = sum(rows[k].shape[1] * rows[k].element_size() for k in ENV if not k.startswith("WARM_K") and k != "WARM_LAMBDA")
    env_bytes = fixed + 16 * count                               # per env: everything but the cache, plus 4 x 4 bytes per cached contact
    cls = [e for e in range(n) if e % 8 == 0 and e != 0]
    src_rep = torch.zeros(len(cls), dtype=torch.int64, device="cuda")
    dst = torch.tensor(cls, dtype=torch.int64, device="cuda")
    res = {"n": n, "mean_warm_count": float(count.float().mean()), "tensors": len(views), "ops": {}}
    bytes_of = {"save_all": 2 * int(env_bytes.sum()), "restore_all": 2 * int(env_bytes.sum()), "clone_class": 2 * int(env_bytes[0]) * len(cls)}

    # ---- baseline: one copy per tensor view (whole warm-start rows: a per-tensor copy cannot stop at the counts without a host round trip)
    keep = {k: torch.empty_like(v) for k, v in views.items()}

    def base_save():
        for k, v in views.items():
            keep[k].copy_(v)

    def base_restore():
        for k, v in views.items():
            v.copy_(keep[k])

    def base_clone():
        for k in ENV:
            rows[k].index_copy_(0, dst, rows[k].index_select(0, src_rep))

    for name, fn in (("save_all", base_save), ("restore_all", base_restore), ("clone_class", base_clone)):
        res["ops"][name] = {"bytes": bytes_of[name], "baseline": summary(timed(fn, repeats, batch))}

    # ---- the snapshot calls (one launch each)
    if hasattr(s, "snapshot"):
        st = s.snapshot()
        src32 = torch.zeros(len(cls), dtype=torch.int32, device="cuda")
        dst32 = dst.to(torch.int32)
        for name, fn in (("save_all", st.save), ("restore_all", st.restore), ("clone_class", lambda: s.clone_envs(src32, dst32))):
            if name == "restore_all":
                st.save()
            r = summary(timed(fn, repeats, batch))
            r["share_of_peak"] = bytes_of[name] / (r["median_us"] * 1e-6) / PEAK
            b = res["ops"][name]["baseline"]
            r["faster_than_baseline"] = r["median_us"] < b["median_us"] and r["max_us"] < b["min_us"]
            res["ops"][name]["snapshot"] = r
        assert s.state_stats() == [0, 0, 0], s.state_stats()
        st.close()
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_state.py needs a GPU"
    lines = []
    for n in a.sizes:
        r = bench(n, a.repeats, a.batch)
        lines.append("N = %d: %d tensor views, mean warm count %.0f" % (n, r["tensors"], r["mean_warm_count"]))
        for name, o in r["ops"].items():
            b = o["baseline"]
            t = "  %-12s %8.1f MB  per-tensor torch: median %8.1f us [%8.1f, %8.1f]" % (name, o["bytes"] / 1e6, b["median_us"], b["min_us"], b["max_us"])
            if "snapshot" in o:
                x = o["snapshot"]
                t += "   snapshot: median %7.1f us [%7.1f, %7.1f] = %.2f TB/s, %.0f %% of the 8 TB/s peak, x%.1f%s" % (
                    x["median_us"], x["min_us"], x["max_us"], o["bytes"] / (x["median_us"] * 1e-6) / 1e12, 100 * x["share_of_peak"],
                    b["median_us"] / x["median_us"], "" if x["faster_than_baseline"] else "   NOT FASTER (spreads overlap)")
            lines.append(t)
        lines.append(json.dumps(r))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
