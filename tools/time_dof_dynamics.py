"""Cost of the joint-space dynamics kernel and of joint torques in the step, per launch, HIP events:

- k_dof_dynamics (SdxSim.dof_dynamics): all outputs, mass only, bias and drive only;
- beside it in the same run: k_kinematics (refresh_kinematics) and one k_physics launch (simulate);
- simulate() with the k_physics<512 | SDX_PHYS_FORCE> instantiation carrying only DOF forces, and carrying only a wrench (what the
  instantiation did before it read DOF forces; a library without sdx_apply_dof_forces reports that one alone).

The protocol of tools/time_forces.py: the variants alternate window by window in one process; a window is `reps` launches between two
device events.  Every simulate() window starts from the same saved state (a snapshot restored outside the timed span).  Prints one JSON
line per N.

    python tools/time_dof_dynamics.py [N=1024,4096] [windows=20] [reps=10]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seqdex_amd import _abi                            # noqa: E402
from seqdex_amd.sim import SdxSim                      # noqa: E402


def measure(n, windows, reps):
    s = SdxSim(n, seed=22)
    g = torch.Generator().manual_seed(0)
    for _ in range(10):                                        # a contact-rich state: resets, then a few steps of random actions
        s.step((torch.rand(n, 23, generator=g) * 2 - 1).cuda())
    snap = s.snapshot()
    snap.save()
    has_dof = hasattr(s, "apply_dof_forces")
    zero_u = torch.zeros(n, _abi.NDOF, device="cuda:0")
    zero_w = torch.zeros(n, _abi.BODIES, 3, device="cuda:0")

    def sim_plain():
        s.simulate()

    def sim_wrench():
        s.apply_rigid_body_forces(zero_w, None, "env")
        s.simulate()

    def sim_dof():
        s.apply_dof_forces(zero_u, 0)
        s.simulate()

    variants = {"k_kinematics": (s.refresh_kinematics, False), "k_physics": (sim_plain, True), "k_physics_force_wrench_only": (sim_wrench, True)}
    if has_dof:
        variants.update({"k_dof_dynamics_all": (lambda: s.dof_dynamics(), False),
                         "k_dof_dynamics_mass_only": (lambda: s.dof_dynamics(bias=False, drive=False), False),
                         "k_dof_dynamics_bias_and_drive": (lambda: s.dof_dynamics(mass=False), False),
                         "k_physics_force_dof_forces_only": (sim_dof, True)})
    for fn, _ in variants.values():                            # warm-up: code objects, allocations
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    for _ in range(windows):
        for name, (fn, steps_state) in variants.items():
            if steps_state:
                snap.restore()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn()
            t1.record()
            t1.synchronize()
            us[name].append(t0.elapsed_time(t1) * 1e3 / reps)
    out = {"what": "per launch, HIP events, windows of %d launches alternating between the variants; simulate() includes k_order" % reps,
           "num_envs": n, "windows": windows}
    for name, v in us.items():
        out[name + "_us"] = {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2), "max": round(float(np.max(v)), 2)}
    snap.close()
    s.close()
    return out


def main():
    ns = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [1024, 4096]
    windows = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    for n in ns:
        print(json.dumps(measure(n, windows, reps)))


if __name__ == "__main__":
    main()
