"""TEST INFRASTRUCTURE ONLY: the pose solver's law of DESIGN.md section 25 (include/seqdex.h sdx_solve_ik) in numpy, stated once and built
from a scene descriptor (include/seqdex.h sdx_scene_desc) alone.  dtype = float64 is the reference of tests/ik_cases.py; dtype = float32 is
the same statement in the kernel's storage precision, whose deviation from the float64 value is the yardstick for the kernel's own.  It
shares no code with the engine."""
import collections

import numpy as np

NL, ND, NA = 24, 23, 7
TASKS = ("base", "ff", "mf", "rf", "th")

# q [23]; err [6]: |position error|, |rotation error| of the base, |position error| of the four tips (0 where not selected); converged [5] bool;
# iters [5]; scaled [5], clamped [5]: whether the step limit / the joint limits changed any step of that task
Sol = collections.namedtuple("Sol", ["q", "err", "converged", "iters", "scaled", "clamped"])


def _vec(v, t):
    return np.array([float(x) for x in v], dtype=t)


def _qmul(a, b):
    """Hamilton product, xyzw"""
    av, bv = a[:3], b[:3]
    return np.concatenate([a[3] * bv + b[3] * av + np.cross(av, bv), [a[3] * b[3] - av @ bv]]).astype(a.dtype)


def _qconj(a):
    return np.concatenate([-a[:3], a[3:]])


def _qrot(q, v):
    u = q[:3]
    t = 2 * np.cross(u, v)
    return (v + q[3] * t + np.cross(u, t)).astype(q.dtype)


def fk(desc, q, dtype=np.float64):
    """origins p [24, 3], orientations r [24, 4] (xyzw) and world joint axes a [24, 3] (row 0 unused) of every link at the joint angles q [23]"""
    t = dtype
    q = np.asarray(q).astype(t)
    p, r, a = np.zeros((NL, 3), t), np.zeros((NL, 4), t), np.zeros((NL, 3), t)
    p[0], r[0] = _vec(desc.base_pos, t), _vec(desc.base_quat, t)
    for k in range(1, NL):                                   # parents come before their children in the descriptor
        par = int(desc.parent[k])
        assert par < k
        jq, ax = _vec(desc.joint_quat[k], t), _vec(desc.joint_axis[k], t)
        half = q[k - 1] / t(2)
        spin = np.concatenate([ax * np.sin(half), [np.cos(half)]]).astype(t)
        rk = _qmul(r[par], _qmul(jq, spin))
        r[k] = rk / np.sqrt(rk @ rk)
        p[k] = p[par] + _qrot(r[par], _vec(desc.joint_pos[k], t))
        a[k] = _qrot(r[par], _qrot(jq, ax))
    assert p.dtype == t and r.dtype == t and a.dtype == t
    return p, r, a


def rotation_error(target_quat, quat):
    """s 2 xyz(target (x) conj(current)), s = -1 if the product's w < 0 else +1"""
    d = _qmul(target_quat, _qconj(quat))
    return (-2 if d[3] < 0 else 2) * d[:3]


def tip_point(desc, p, r, f, offset):
    k = int(desc.fingertip_body[f])
    return p[k] + _qrot(r[k], offset)


def _dls(J, e, damping, t):
    """J^T (J J^T + damping^2 I)^-1 e through the Cholesky factor"""
    A = J @ J.T + damping * damping * np.eye(J.shape[0], dtype=t)
    L = np.linalg.cholesky(A)
    return (J.T @ np.linalg.solve(L.T, np.linalg.solve(L, e))).astype(t)


def _loop(q, dofs, lo, up, error, jacobian, done, damping, max_step, max_iters, t):
    """the loop both stages share.  Returns (q, error norms at q, converged, steps taken, any step scaled, any step clamped)"""
    it, scaled, clamped = 0, False, False
    while True:
        e, state = error(q)
        norms, ok = done(e)
        if ok or it >= max_iters:
            return q, norms, ok, it, scaled, clamped
        dq = _dls(jacobian(q, state), e, damping, t)
        m = np.abs(dq).max()
        if m > max_step:
            scaled = True
        dq = dq / max(t(1), m / max_step)
        nxt = q[dofs] + dq
        if (nxt < lo[dofs]).any() or (nxt > up[dofs]).any():
            clamped = True
        q = q.copy()
        q[dofs] = np.minimum(up[dofs], np.maximum(lo[dofs], nxt))
        assert q.dtype == t
        it += 1


def solve(desc, q0, base_pos, base_quat, tip_pos, params, lower=None, upper=None, dtype=np.float64):
    """one env.  q0 [23]; base_pos [3], base_quat [4] xyzw, tip_pos [4, 3] (None where params does not select the task); params: a
    seqdex_amd.ik.IkParams; lower / upper [23]: the limits (None: the descriptor's).  Every operand is cast to dtype first and every
    operation carried out in it."""
    t = dtype
    f32 = np.float32
    q = np.asarray(q0, f32).astype(t)
    lo = (_vec(desc.lower, f32) if lower is None else np.asarray(lower, f32)).astype(t)
    up = (_vec(desc.upper, f32) if upper is None else np.asarray(upper, f32)).astype(t)
    d_arm, d_fin, max_step = t(f32(params.damping_arm)), t(f32(params.damping_finger)), t(f32(params.max_step))
    pos_tol, rot_tol = t(f32(params.pos_tol)), t(f32(params.rot_tol))
    ee = int(desc.hand_base_body)
    err, conv, iters = np.zeros(6), np.zeros(5, bool), np.zeros(5, np.int64)
    scaled, clamped = np.zeros(5, bool), np.zeros(5, bool)
    if "base" in params.tasks:
        tp, tq = np.asarray(base_pos, f32).astype(t), np.asarray(base_quat, f32).astype(t)
        dofs = np.arange(NA)

        def error(q):
            p, r, a = fk(desc, q, t)
            return np.concatenate([tp - p[ee], rotation_error(tq, r[ee])]).astype(t), (p, a)

        def jacobian(q, state):
            p, a = state
            return np.stack([np.concatenate([np.cross(a[j + 1], p[ee] - p[j + 1]), a[j + 1]]) for j in dofs], 1).astype(t)

        def done(e):
            n = (np.sqrt(e[:3] @ e[:3]), np.sqrt(e[3:] @ e[3:]))
            return n, bool(pos_tol > 0 and rot_tol > 0 and n[0] <= pos_tol and n[1] <= rot_tol)      # (a tolerance of 0 is never met)

        q, n, conv[0], iters[0], scaled[0], clamped[0] = _loop(q, dofs, lo, up, error, jacobian, done, d_arm, max_step, params.max_iters, t)
        err[0:2] = n
    for f in range(4):
        if TASKS[1 + f] not in params.tasks:
            continue
        tc, off = np.asarray(tip_pos[f], f32).astype(t), np.asarray(params.tip_offset[f], f32).astype(t)
        dofs = np.arange(NA + 4 * f, NA + 4 * f + 4)

        def error(q):
            p, r, a = fk(desc, q, t)
            c = tip_point(desc, p, r, f, off)
            return (tc - c).astype(t), (p, a, c)

        def jacobian(q, state):
            p, a, c = state
            return np.stack([np.cross(a[j + 1], c - p[j + 1]) for j in dofs], 1).astype(t)

        def done(e):
            n = np.sqrt(e @ e)
            return (n,), bool(pos_tol > 0 and n <= pos_tol)

        q, n, conv[1 + f], iters[1 + f], scaled[1 + f], clamped[1 + f] = _loop(q, dofs, lo, up, error, jacobian, done, d_fin, max_step,
                                                                                 params.max_iters, t)
        err[2 + f] = n[0]
    assert q.dtype == t
    return Sol(q, err, conv, iters, scaled, clamped)
