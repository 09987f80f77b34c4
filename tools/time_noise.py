"""Cost of the observation / action noise: sdx_step of BlockAssemblyGraspSim with randomization on (identity rows)
and the shipped `observations` / `actions` blocks past their schedules, against the same library with noise off.  The two simulators
alternate window by window in one process; a window is `steps` env steps between two device events.  Prints one JSON line.

    python tools/time_noise.py [N=1024] [windows=30] [steps=10]"""
import json
import os
import sys

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seqdex_amd import domain_randomization as dr      # noqa: E402
from seqdex_amd.sim import SdxSim                      # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    windows = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    with open(os.path.join(ROOT, "seqdex_amd", "cfg", "allegro_hand_block_assembly_grasp_sim.yaml")) as f:
        params = yaml.safe_load(f)["task"]["randomization_params"]
    sims = {}
    for name in ("noise_off", "noise_on"):
        s = SdxSim(n, seed=22)
        s.DR_FRAME[0] = 50000                                  # past schedule_steps: full-strength noise
        s.set_randomization(dr.identity_desc(10 ** 9))         # the same physics on both sides
        if name == "noise_on":
            s.set_noise(params)
        sims[name] = s
    g = torch.Generator().manual_seed(0)
    acts = [(torch.rand(n, 23, generator=g) * 2 - 1).cuda() for _ in range(steps)]
    for s in sims.values():                                    # warm-up: code objects, the first reset of every env
        for _ in range(3):
            for a in acts:
                s.step(a)
    torch.cuda.synchronize()
    us = {k: [] for k in sims}
    for _ in range(windows):
        for name, s in sims.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for a in acts:
                s.step(a)
            t1.record()
            t1.synchronize()
            us[name].append(t0.elapsed_time(t1) * 1e3 / steps)
    out = {"what": "sdx_step per env step, HIP events, windows of %d steps alternating between the two simulators" % steps,
           "num_envs": n, "windows": windows}
    for name, v in us.items():
        out[name + "_us"] = {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2), "max": round(float(np.max(v)), 2)}
    out["noise_cost_us"] = round(out["noise_on_us"]["median"] - out["noise_off_us"]["median"], 2)
    out["noise_cost_pct"] = round(100.0 * out["noise_cost_us"] / out["noise_off_us"]["median"], 2)
    out["contacts_mean"] = {k: round(float(s.NCONTACTS.float().mean()), 1) for k, s in sims.items()}
    print(json.dumps(out))
    for s in sims.values():
        s.close()


if __name__ == "__main__":
    main()
