"""Cost of the contact report, HIP events:

- simulate() with the report off (k_physics<512>) against simulate() with it armed (k_report_table + k_physics<516>), on the same simulator
  and state: arming changes no result, so the two variants alternate window by window over one trajectory;
- the reducer k_contact_wrenches: net wrenches of all bodies, the 5 x 3 sensor / filter matrix, and both;
- beside them the bytes an armed step writes: sum over the envs of count x 44 B (two body rows, key, point, normal, force, separation).

The protocol of tools/time_osc.py: a window is `reps` calls between two device events.  The state is the one bench.py times: the default
scene after `steps0` steps of random actions.  Prints one JSON line per N.

    python tools/time_contact_report.py [N=1024] [windows=20] [reps=10] [steps0=10]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seqdex_amd import _abi                                    # noqa: E402
from seqdex_amd.contact_report import fingertip_bodies          # noqa: E402
from seqdex_amd.sim import SdxSim                              # noqa: E402


def measure(n, windows, reps, steps0):
    s = SdxSim(n, seed=22)
    g = torch.Generator().manual_seed(0)
    for _ in range(steps0):
        s.step((torch.rand(n, 23, generator=g) * 2 - 1).cuda())
    rep = s.contact_report()
    s.simulate()
    torch.cuda.synchronize()
    count = rep.count.cpu().numpy().astype(np.int64)
    sensors = fingertip_bodies(s.scene) + [int(s.scene.hand_base_body)]
    filters = [_abi.BODY_BRICK0, _abi.BODY_BRICK0 + 5, -1]
    net = torch.empty(n, _abi.BODIES, 6, device="cuda:0")
    pf = torch.empty(n, len(sensors), len(filters), 3, device="cuda:0")

    def arm(on):
        s._check(s.lib.sdx_set_contact_report(s.h, rep.struct if on else None, None))     # (host state only: nothing is enqueued)

    def physics(on):
        arm(on)
        s.simulate()

    def both():
        rep.net_wrenches(out=net)
        rep.pair_forces(sensors, filters, out=pf)

    variants = {"simulate_report_off": lambda: physics(False), "simulate_report_armed": lambda: physics(True),
                "k_contact_wrenches_net": lambda: rep.net_wrenches(out=net),
                "k_contact_wrenches_pairs": lambda: rep.pair_forces(sensors, filters, out=pf), "k_contact_wrenches_net_then_pairs": both}
    for fn in variants.values():                               # warm-up: code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    for _ in range(windows):
        for name, fn in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn()
            t1.record()
            t1.synchronize()
            us[name].append(t0.elapsed_time(t1) * 1e3 / reps)
    arm(True)
    out = {"what": "per call, HIP events, windows of %d calls alternating between the variants; simulate() = k_physics + k_order (+ k_report_table when armed)" % reps,
           "num_envs": n, "windows": windows, "contacts_per_env": {"mean": round(float(count.mean()), 1), "max": int(count.max())},
           "report_bytes_per_step": int(count.sum() * 44 + 4 * n)}
    for name, v in us.items():
        out[name + "_us"] = {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2), "max": round(float(np.max(v)), 2)}
    med = {k: float(np.median(v)) for k, v in us.items()}
    out["armed_over_off"] = round(med["simulate_report_armed"] / med["simulate_report_off"], 4)
    out["armed_minus_off_us"] = round(med["simulate_report_armed"] - med["simulate_report_off"], 2)
    s.close()
    return out


def main():
    ns = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [1024]
    windows = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    steps0 = int(sys.argv[4]) if len(sys.argv) > 4 else 10
    for n in ns:
        print(json.dumps(measure(n, windows, reps, steps0)))


if __name__ == "__main__":
    main()
