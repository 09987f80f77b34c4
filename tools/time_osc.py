"""Cost of the operational-space torque kernel, per control step, HIP events:

- k_osc_torques (SdxSim.osc_torques), torques only and with the wrench;
- beside it in the same run: k_dof_dynamics with mass and bias (SdxSim.dof_dynamics(drive=False)), which the kernel shares its forward
  kinematics with;
- the formulation it replaces: dof_dynamics(drive=False), then the same law in batched torch ops on the [N, 7, 7] block and SDX_T_JAC_EEF
  (Cholesky factorisations and solves, matrix products, the clamp), float32 on the device.

The protocol of tools/time_dof_dynamics.py: the variants alternate window by window in one process; a window is `reps` control steps between
two device events.  Prints one JSON line per N, with the ratios of the medians.

    python tools/time_osc.py [N=1024,4096] [windows=20] [reps=10]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seqdex_amd import _abi                            # noqa: E402
from seqdex_amd import torque_control as tc            # noqa: E402
from seqdex_amd.sim import SdxSim                      # noqa: E402


def torch_law(s, dpose, gains, effort):
    """dof_dynamics() followed by the law of DESIGN.md section 23 in batched torch ops; returns the [N, NDOF] row"""
    n = s.num_envs
    dyn = s.dof_dynamics(drive=False)
    M = dyn.mass[:, :7, :7]
    b = dyn.bias[:, :7]
    J = s.JAC_EEF.view(n, 6, 7)
    dof = s.DOF.view(n, _abi.NDOF, 2)
    q, qd = dof[:, :7, 0], dof[:, :7, 1]
    Jt = J.transpose(1, 2)
    LM = torch.linalg.cholesky(M)
    A = J @ torch.cholesky_solve(Jt, LM) + gains["damping"] ** 2 * torch.eye(6, device=M.device)
    LA = torch.linalg.cholesky(A)
    F = gains["kp"] * dpose - gains["kd"] * (J @ qd.unsqueeze(-1)).squeeze(-1)
    w = torch.cholesky_solve(F.unsqueeze(-1), LA)
    u_null = M @ (gains["kp_null"] * (gains["q_null"] - q) - gains["kd_null"] * qd).unsqueeze(-1)
    u = Jt @ w + u_null - Jt @ torch.cholesky_solve(J @ torch.cholesky_solve(u_null, LM), LA) + b.unsqueeze(-1)
    out = torch.zeros(n, _abi.NDOF, device=M.device)
    out[:, :7] = torch.minimum(torch.maximum(u.squeeze(-1), -effort), effort)
    return out


def measure(n, windows, reps):
    s = SdxSim(n, seed=22)
    g = torch.Generator().manual_seed(0)
    for _ in range(10):                                        # a state off the start pose: resets, then a few steps of random actions
        s.step((torch.rand(n, 23, generator=g) * 2 - 1).cuda())
    s.refresh_kinematics()
    gains = tc.OscGains(q_null=[0.5 * (lo + up) for lo, up in zip(s.scene.lower[:7], s.scene.upper[:7])])
    tg = {k: torch.tensor(getattr(gains, k), device="cuda:0") for k in ("kp", "kd", "kp_null", "kd_null", "q_null")}
    tg["damping"] = gains.damping
    effort = torch.tensor([float(v) for v in s._desc.effort][:7], device="cuda:0")
    dpose = ((torch.rand(n, 6, generator=g) * 2 - 1) * torch.tensor([0.03] * 3 + [0.1] * 3)).cuda().contiguous()
    attr = gains.to_attr()
    a = s.osc_torques(dpose, attr).clone()
    b = torch_law(s, dpose, tg, effort)
    torch.cuda.synchronize()
    agree = float((a - b).abs().max() / a.abs().max())
    assert agree < 1e-3, agree                                 # the two formulations compute the same row
    variants = {"k_osc_torques": lambda: s.osc_torques(dpose, attr),
                "k_osc_torques_with_wrench": lambda: s.osc_torques(dpose, attr, wrench=True),
                "k_dof_dynamics_mass_and_bias": lambda: s.dof_dynamics(drive=False),
                "torch_formulation": lambda: torch_law(s, dpose, tg, effort)}
    for fn in variants.values():                               # warm-up: code objects, allocations
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
    out = {"what": "per control step, HIP events, windows of %d steps alternating between the variants" % reps, "num_envs": n, "windows": windows,
           "kernel_vs_torch_max_rel_difference": agree}
    for name, v in us.items():
        out[name + "_us"] = {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2), "max": round(float(np.max(v)), 2)}
    med = {k: float(np.median(v)) for k, v in us.items()}
    out["k_osc_torques_over_k_dof_dynamics"] = round(med["k_osc_torques"] / med["k_dof_dynamics_mass_and_bias"], 3)
    out["torch_formulation_over_k_osc_torques"] = round(med["torch_formulation"] / med["k_osc_torques"], 2)
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
