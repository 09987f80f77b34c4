"""Cost of the pose solver, per solve, HIP events:

- k_solve_ik (SdxSim.solve_ik) with tolerances 0 and max_iters = 16: the work is fixed, 16 arm steps and 16 steps of every finger;
- what a user does without it, 16 times: write SDX_T_DOF, refresh_kinematics(), one damped-least-squares step of the arm and of the four
  fingers in batched float32 torch ops from SDX_T_RB and SDX_T_JACOBIAN (Cholesky factorisations and solves, the step limit, the clamp).
  Arm and fingers step together there, one refresh per iteration; the kernel's law finishes the arm first.  The arm's angles must agree;
  a finger has 4 DOFs for a point, so the two orders end at different angles with the same tip point: the tip errors of both are reported.

The protocol of tools/time_osc.py: the variants alternate window by window in one process; a window is `reps` solves between two device
events.  Prints one JSON line per N, with the ratio of the medians.

    python tools/time_ik.py [N=1024,4096] [windows=20] [reps=5]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seqdex_amd import _abi                            # noqa: E402
from seqdex_amd import ik                              # noqa: E402
from seqdex_amd import torque_control as tc            # noqa: E402
from seqdex_amd.sim import SdxSim                      # noqa: E402

ITERS = 16
OFFSET = (0.0, 0.0, 0.02)


def qrot(q, v):
    """quat_apply, xyzw"""
    u = q[..., :3]
    t = 2.0 * torch.cross(u, v, dim=-1)
    return v + q[..., 3:4] * t + torch.cross(u, t, dim=-1)


def dls(J, e, damping, max_step):
    """J^T (J J^T + damping^2 I)^-1 e, then the step limit; J [B, m, n], e [B, m]"""
    A = J @ J.transpose(1, 2) + damping * damping * torch.eye(J.shape[1], device=J.device)
    y = torch.cholesky_solve(e.unsqueeze(-1), torch.linalg.cholesky(A))
    dq = (J.transpose(1, 2) @ y).squeeze(-1)
    return dq / torch.clamp(dq.abs().amax(-1, keepdim=True) / max_step, min=1.0)


def tips_of(s, rb, off):
    k = torch.as_tensor(list(s.scene.fingertip_bodies), device=rb.device)
    p, r = rb[:, k, 0:3], rb[:, k, 3:7]
    return p, p + qrot(r, off.expand_as(p))


def torch_loop(s, q0, bp, bq, tp, par, lo, up, off):
    """ITERS x (write DOF, refresh, DLS of the arm and the four fingers, clamp); returns q [N, 23]"""
    n, ee = s.num_envs, int(s._desc.hand_base_body)
    dof = s.DOF.view(n, _abi.NDOF, 2)
    rb = s.RB.view(n, -1, 13)
    jac = s.JACOBIAN.view(n, _abi.NLINK - 1, 6, _abi.NDOF)
    q = q0.clone()
    fd = torch.arange(7, 23, device=q.device).view(4, 4)
    for _ in range(ITERS):
        dof[:, :, 0] = q
        s.refresh_kinematics()
        e = tc.pose_error(rb[:, ee, 0:3], rb[:, ee, 3:7], bp, bq)
        dq_arm = dls(jac[:, ee - 1, :, :7], e, par.damping_arm, par.max_step)
        p, c = tips_of(s, rb, off)
        tip_links = torch.as_tensor([k - 1 for k in s.scene.fingertip_bodies], device=q.device)
        Jt = jac[:, tip_links]                                                      # [N, 4, 6, 23]
        Jf = torch.stack([Jt[:, f][:, :, fd[f]] for f in range(4)], 1)              # [N, 4, 6, 4]: each finger's own columns
        arm_ = (c - p).unsqueeze(-1).expand(-1, -1, -1, 4)
        Jc = Jf[:, :, 0:3] + torch.cross(Jf[:, :, 3:6], arm_, dim=2)                # the point c: lin + ang x (c - p)
        dq_f = dls(Jc.reshape(n * 4, 3, 4), (tp - c).reshape(n * 4, 3), par.damping_finger, par.max_step).view(n, 16)
        q = torch.minimum(torch.maximum(q + torch.cat([dq_arm, dq_f], 1), lo), up)
    return q


def measure(n, windows, reps):
    s = SdxSim(n, seed=22)
    g = torch.Generator().manual_seed(0)
    lo = torch.tensor([float(v) for v in s.scene.lower], device="cuda:0")
    up = torch.tensor([float(v) for v in s.scene.upper], device="cuda:0")
    mid, half = 0.5 * (lo + up), 0.5 * (up - lo)
    qs = mid + 0.3 * half * (torch.rand(n, 23, generator=g) * 2 - 1).cuda()
    q0 = torch.minimum(torch.maximum(qs + 0.3 * (torch.rand(n, 23, generator=g) * 2 - 1).cuda(), lo), up).contiguous()
    off = torch.tensor(OFFSET, device="cuda:0")
    ee = int(s._desc.hand_base_body)
    s.DOF.view(n, 23, 2)[:, :, 0] = qs
    s.refresh_kinematics()
    rb = s.RB.view(n, -1, 13)
    bp, bq = rb[:, ee, 0:3].clone(), rb[:, ee, 3:7].clone()
    tp = tips_of(s, rb, off)[1].clone()
    par = ik.IkParams(max_iters=ITERS, pos_tol=0.0, rot_tol=0.0, tip_offset=OFFSET)
    attr = par.to_attr()
    saved = s.DOF.clone()

    def errors(q):
        s.DOF.view(n, 23, 2)[:, :, 0] = q
        s.refresh_kinematics()
        r = s.RB.view(n, -1, 13)
        e = tc.pose_error(r[:, ee, 0:3], r[:, ee, 3:7], bp, bq)
        return [float(e[:, :3].norm(dim=1).max()), float(e[:, 3:].norm(dim=1).max()), float((tp - tips_of(s, r, off)[1]).norm(dim=2).max())]

    a = s.solve_ik(bp, bq, tp, attr, q0=q0).q.clone()
    b = torch_loop(s, q0, bp, bq, tp, par, lo, up, off)
    torch.cuda.synchronize()
    arm_diff = float((a[:, :7] - b[:, :7]).abs().max())
    ea, eb = errors(a), errors(b)
    s.DOF.copy_(saved)
    s.refresh_kinematics()
    assert arm_diff < 1e-3, arm_diff                           # the two formulations take the arm to the same angles
    variants = {"k_solve_ik": lambda: s.solve_ik(bp, bq, tp, attr, q0=q0),
                "torch_formulation": lambda: torch_loop(s, q0, bp, bq, tp, par, lo, up, off)}
    for fn in variants.values():                               # warm-up: code objects, allocations
        for _ in range(2):
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
    out = {"what": "per solve of %d iterations, HIP events, windows of %d solves alternating between the variants" % (ITERS, reps), "num_envs": n,
           "windows": windows, "kernel_vs_torch_max_arm_angle_difference_rad": arm_diff,
           "k_solve_ik_errors_base_m_base_rot_tip_m": ea, "torch_formulation_errors_base_m_base_rot_tip_m": eb}
    for name, v in us.items():
        out[name + "_us"] = {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2), "max": round(float(np.max(v)), 2)}
    med = {k: float(np.median(v)) for k, v in us.items()}
    out["torch_formulation_over_k_solve_ik"] = round(med["torch_formulation"] / med["k_solve_ik"], 2)
    s.close()
    return out


def main():
    ns = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [1024, 4096]
    windows = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    for n in ns:
        print(json.dumps(measure(n, windows, reps)))


if __name__ == "__main__":
    main()
