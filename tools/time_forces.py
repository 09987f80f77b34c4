"""Cost of the random pushes: sdx_step of BlockAssemblyGraspSim with the sampler on (k_force_perturb and the
k_physics<512 | SDX_PHYS_FORCE> instantiation every step) against the same library with it off (k_physics<512>).  The protocol of
tools/time_noise.py: the two simulators alternate window by window in one process; a window is `steps` env steps between two device events.
Prints one JSON line.

    python tools/time_forces.py [N=1024] [windows=30] [steps=10] [force_scale=2.0]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seqdex_amd import _abi                            # noqa: E402
from seqdex_amd.sim import SdxSim                      # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    windows = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    scale = float(sys.argv[4]) if len(sys.argv) > 4 else 2.0
    sims, keep = {}, []
    for name in ("pushes_off", "pushes_on"):
        s = SdxSim(n, seed=22)
        if name == "pushes_on":                                # the defaults of the task classes: forceProbRange, forceDecay, forceDecayInterval
            keep += [torch.zeros(n, _abi.BODIES, 3, device="cuda:0"), torch.zeros(n, device="cuda:0")]
            s.set_force_perturbation(_abi.ForcePerturbAttr(scale, 0.001, 0.1, 0.99, 0.08), keep[0], keep[1])
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
           "num_envs": n, "windows": windows, "force_scale": scale}
    for name, v in us.items():
        out[name + "_us"] = {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2), "max": round(float(np.max(v)), 2)}
    out["push_cost_us"] = round(out["pushes_on_us"]["median"] - out["pushes_off_us"]["median"], 2)
    out["push_cost_pct"] = round(100.0 * out["push_cost_us"] / out["pushes_off_us"]["median"], 2)
    out["contacts_mean"] = {k: round(float(s.NCONTACTS.float().mean()), 1) for k, s in sims.items()}
    out["pushed_rows_now"] = int((keep[0] != 0).any(-1).sum())
    print(json.dumps(out))
    for s in sims.values():
        s.close()


if __name__ == "__main__":
    main()
