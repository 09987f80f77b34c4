"""Torque control on top of SdxSim.apply_dof_forces / SdxSim.dof_dynamics / SdxSim.osc_torques (include/seqdex.h sdx_apply_dof_forces,
sdx_dof_dynamics, sdx_osc_torques; DESIGN.md sections 22 and 23): the reference's PD torque law of its torque_control mode
(morb.py:1288-1297), inverse dynamics from the mass matrix and bias tensors, and the gains and the pose error of the operational-space
controller.  Plain tensor expressions on whatever device the arguments live on; no kernel of its own."""
import collections
import math

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


class OscGains(collections.namedtuple("OscGains", ["kp", "kd", "kp_null", "kd_null", "q_null", "damping", "compensate_bias"])):
    """the gains of SdxSim.osc_torques (sdx_osc_attr).  kp / kd: a number or 6 numbers (rows 0..2 linear, 3..5 angular); kp_null / kd_null: a
    number or 7; q_null: the 7 arm angles the posture spring pulls to (None: zeros).  A kd left None is critically damped: 2 sqrt(kp)."""
    __slots__ = ()

    def __new__(cls, kp=100.0, kd=None, kp_null=10.0, kd_null=None, q_null=None, damping=0.05, compensate_bias=True):
        def vec(v, n, what):
            out = [float(v)] * n if isinstance(v, (int, float)) else [float(x) for x in v]
            if len(out) != n:
                raise ValueError("OscGains: %s takes a number or %d of them, got %d" % (what, n, len(out)))
            return tuple(out)

        kp, kp_null = vec(kp, 6, "kp"), vec(kp_null, 7, "kp_null")
        kd = tuple(2.0 * math.sqrt(k) for k in kp) if kd is None else vec(kd, 6, "kd")
        kd_null = tuple(2.0 * math.sqrt(k) for k in kp_null) if kd_null is None else vec(kd_null, 7, "kd_null")
        q_null = (0.0,) * 7 if q_null is None else vec(q_null, 7, "q_null")
        return super().__new__(cls, kp, kd, kp_null, kd_null, q_null, float(damping), bool(compensate_bias))

    def to_attr(self):
        """the _abi.OscAttr of these gains"""
        from . import _abi
        a = _abi.OscAttr()
        for name in ("kp", "kd", "kp_null", "kd_null", "q_null"):
            getattr(a, name)[:] = getattr(self, name)
        a.damping, a.compensate_bias = self.damping, int(self.compensate_bias)
        return a


def pose_error(pos, quat, target_pos, target_quat):
    """dpose [N, 6] for SdxSim.osc_torques, the pose error control_ik takes: target_pos - pos, then sign(w) 2 xyz of target_quat (x)
    conj(quat), the rotation vector of the rotation from the current to the target orientation to first order (exact direction,
    2 sin(angle / 2) for its length).  Quaternions [N, 4] in xyzw order, as the rows of SDX_T_RB."""
    cx, cy, cz, cw = -quat[:, 0], -quat[:, 1], -quat[:, 2], quat[:, 3]
    tx, ty, tz, tw = target_quat[:, 0], target_quat[:, 1], target_quat[:, 2], target_quat[:, 3]
    x = tw * cx + tx * cw + ty * cz - tz * cy
    y = tw * cy - tx * cz + ty * cw + tz * cx
    z = tw * cz + tx * cy - ty * cx + tz * cw
    w = tw * cw - tx * cx - ty * cy - tz * cz
    rot = 2.0 * torch.sign(w).unsqueeze(-1) * torch.stack([x, y, z], -1)
    return torch.cat([target_pos - pos, rot], -1).contiguous()
