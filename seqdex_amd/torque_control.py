"""Torque control on top of SdxSim.apply_dof_forces / SdxSim.dof_dynamics (include/seqdex.h sdx_apply_dof_forces, sdx_dof_dynamics;
DESIGN.md section 22): the reference's PD torque law of its torque_control mode (morb.py:1288-1297) and inverse dynamics from the mass
matrix and bias tensors.  Plain tensor expressions on whatever device the arguments live on; no kernel of its own."""
import collections

import torch

# what SdxSim.dof_dynamics returns: mass [N, 23, 23] = M(q) + armature, bias [N, 23] = C(q, qd) qd, drive [N, 23] = the clamped PD torque of
# the next launch's first substep; None for an output that was not asked for
DofDynamics = collections.namedtuple("DofDynamics", ["mass", "bias", "drive"])


def pd_torques(q, qd, targets, p_gain, d_gain, clip):
    """torques = clip(p_gain (targets - q) - d_gain qd, -clip, clip) (morb.py:1292, 1297; the reference passes the finite-difference joint
    velocity (q - q_prev) / dt as qd and clips to 20).  Gains and clip: numbers or tensors that broadcast against [N, NDOF]."""
    t = p_gain * (targets - q) - d_gain * qd
    if torch.is_tensor(clip):
        return torch.minimum(torch.maximum(t, -clip), clip)
    return torch.clamp(t, -clip, clip)


def inverse_dynamics(dyn, qdd):
    """the joint torques M qdd + bias that give the joint accelerations qdd [N, NDOF]; dyn: a DofDynamics with mass and bias"""
    if dyn.mass is None or dyn.bias is None:
        raise ValueError("inverse_dynamics: needs the mass and bias outputs of dof_dynamics()")
    return torch.bmm(dyn.mass, qdd.unsqueeze(-1)).squeeze(-1) + dyn.bias
