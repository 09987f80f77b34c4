"""TEST INFRASTRUCTURE ONLY: the robot's joint-space inertia in float64 numpy, straight from a scene descriptor (include/seqdex.h
sdx_scene_desc): M(q) = sum over the links k of m_k Jv_k^T Jv_k + Jw_k^T (R_k I_k R_k^T) Jw_k with the Jacobians of the link's centre of mass,
plus the armature on the diagonal.  The yardstick the float32 oracle's own rounding is measured against (tests/dof_dynamics_cases.py,
DESIGN.md section 22); it shares no code with the engine or the C oracle."""
import numpy as np

NL, ND = 24, 23


def _R(q):
    x, y, z, w = [float(v) for v in q]
    n = (x * x + y * y + z * z + w * w) ** 0.5
    x, y, z, w = x / n, y / n, z / n, w / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _axis_R(a, ang):
    a = np.asarray(a, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def mass_matrix(desc, q, link_factor=None):
    """M(q) + armature, float64 [23, 23].  DOF j is the joint of link j + 1.  link_factor [24]: masses and inertias scaled per link"""
    q = np.asarray(q, np.float64)
    f = np.ones(NL) if link_factor is None else np.asarray(link_factor, np.float64)
    R, p, a = [None] * NL, [None] * NL, [None] * NL
    path = [[] for _ in range(NL)]
    R[0], p[0] = _R(desc.base_quat), np.array([float(v) for v in desc.base_pos])
    for k in range(1, NL):                                   # parents come before their children in the descriptor
        par = int(desc.parent[k])
        assert par < k
        Rj = _R(desc.joint_quat[k])
        a[k] = R[par] @ Rj @ np.array([float(v) for v in desc.joint_axis[k]])
        R[k] = R[par] @ Rj @ _axis_R([float(v) for v in desc.joint_axis[k]], q[k - 1])
        p[k] = p[par] + R[par] @ np.array([float(v) for v in desc.joint_pos[k]])
        path[k] = path[par] + [k - 1]
    M = np.zeros((ND, ND))
    for k in range(1, NL):
        c = p[k] + R[k] @ np.array([float(v) for v in desc.link_com[k]])
        I6 = [float(v) for v in desc.link_inertia[k]]
        Il = np.array([[I6[0], I6[3], I6[4]], [I6[3], I6[1], I6[5]], [I6[4], I6[5], I6[2]]])
        Iw = R[k] @ Il @ R[k].T * f[k]
        Jv, Jw = np.zeros((3, ND)), np.zeros((3, ND))
        for j in path[k]:
            Jw[:, j] = a[j + 1]
            Jv[:, j] = np.cross(a[j + 1], c - p[j + 1])
        M += float(desc.link_mass[k]) * f[k] * (Jv.T @ Jv) + Jw.T @ Iw @ Jw
    return M + np.diag([float(v) for v in desc.armature])
