"""Shared bodies of the operational-space control tests (include/seqdex.h sdx_osc_torques): tests/test_osc.py runs
them on the emulated simulator (tests/hipemu), tests/test_gpu_osc.py on the GPU.  A `backend` is (make, dev) as in
tests/dof_dynamics_cases.py, whose placing and drawing helpers are used here.  The reference is the law in numpy float64
(tests/helpers/osc_float64.py) fed with the engine's own dof_dynamics() and SDX_T_JAC_EEF; every bar is 4 x what the same law in numpy
float32 loses against float64 on the same inputs.  N = 3 everywhere (one env per workgroup: no pack size to straddle)."""
import ctypes as C

import numpy as np
import torch

import dof_dynamics_cases as D
from helpers import osc_float64 as O
from seqdex_amd import _abi
from seqdex_amd import torque_control as tc

f32 = np.float32
N, ND, NL, NA = D.N, D.ND, D.NL, 7
SEED = D.SEED
ARM = D.ARM
host = D.host
MARGIN = 4.0              # the kernel's bar over the float32 restatement's deviation (the margin DESIGN.md section 22 used for M)


def _effort(s):
    return np.array([float(v) for v in s._desc.effort])


def _gains(s, **kw):
    """all gains non-zero and different per coordinate, critically damped, the posture spring to the arm's mid-range"""
    base = dict(kp=[100.0, 120.0, 90.0, 80.0, 70.0, 60.0], kp_null=[10.0, 12.0, 9.0, 11.0, 8.0, 10.0, 7.0], q_null=D._mid(s)[:NA], damping=0.05,
                compensate_bias=True)
    base.update(kw)
    return tc.OscGains(**base)


def _draw_state(s, rng, n=N):
    q = D._draw_q(s, rng, n=n, spread=0.2)
    qd = np.concatenate([rng.uniform(-1.5, 1.5, (n, NA)), rng.uniform(-2.0, 2.0, (n, ND - NA))], 1).astype(f32)
    return q, qd


def _draw_dpose(rng, n=N):
    """position part of length <= 5 cm, rotation part of length <= 0.2 rad"""
    def ball(r):
        d = rng.normal(size=(n, 3))
        return d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.2 * r, r, (n, 1))
    return np.concatenate([ball(0.05), ball(0.2)], 1).astype(f32)


def _inputs(s):
    """what the helper is fed with: the engine's own mass, bias, Jacobian and DOF state"""
    n = s.num_envs
    dyn = D._dyn(s, drive=False)
    return dict(M=dyn.mass[:, :NA, :NA].copy(), b=dyn.bias[:, :NA].copy(), J=host(s.JAC_EEF).reshape(n, 6, NA), dof=D._dofs(s)[:, :NA])


def _call(s, dev, dpose, gains):
    u, w = s.osc_torques(dev(torch.from_numpy(np.ascontiguousarray(dpose, f32))), gains, wrench=True)
    return host(u), host(w)


def _law(inp, dpose, gains, effort, dtype, M=None):
    M = inp["M"] if M is None else M
    return [O.osc(M[e], inp["J"][e], inp["b"][e], inp["dof"][e, :, 0], inp["dof"][e, :, 1], dpose[e], gains, effort[:NA], dtype)
            for e in range(len(dpose))]


def _rel(a, ref):
    """largest |a - ref| of a row relative to the row's largest |ref|"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def _against_float64(s, dev, dpose, gains, what, M=None):
    """the engine's torques and wrench against the float64 law on the engine's own inputs; the bar: MARGIN x the float32 law's deviation.
    Returns (yardstick u, engine u, yardstick w, engine w, the float64 rows, the engine's u)."""
    effort = _effort(s)
    inp = _inputs(s)
    r64 = _law(inp, dpose, gains, effort, np.float64, M)
    r32 = _law(inp, dpose, gains, effort, np.float32, M)
    u, w = _call(s, dev, dpose, gains)
    n = len(dpose)
    assert np.isfinite(u).all() and np.isfinite(w).all(), what
    for e in range(n):                                                              # the clamp cannot hide a difference
        assert (np.abs(r64[e].u) < 0.9 * effort[:NA]).all(), (what, e, r64[e].u)
    yu = max(_rel(r32[e].u, r64[e].u) for e in range(n))
    yw = max(_rel(r32[e].wrench, r64[e].wrench) for e in range(n))
    du = max(_rel(u[e, :NA], r64[e].u) for e in range(n))
    dw = max(_rel(w[e], r64[e].wrench) for e in range(n))
    print("%s: torques: float32 law vs float64 %.3g, engine vs float64 %.3g (bar %.3g); wrench: %.3g, %.3g (bar %.3g); relative to the row's "
          "largest entry, max |u| %.3g N m" % (what, yu, du, MARGIN * yu, yw, dw, MARGIN * yw, max(np.abs(r.u).max() for r in r64)))
    assert 0 < yu < 1e-3 and 0 < yw < 1e-3, (what, yu, yw)                           # float32 rounding, not a modelling difference
    assert du <= MARGIN * yu, (what, du, yu)
    assert dw <= MARGIN * yw, (what, dw, yw)
    assert (u[:, NA:].view(np.uint32) == 0).all(), what
    return yu, du, yw, dw, r64, u


def _expect_value_error(fn, word):
    try:
        fn()
    except ValueError as err:
        assert word in str(err), err
    else:
        raise AssertionError("accepted a bad %s" % word)


# ------------------------------------------------------------------------------------------------------------------ 1. ABI
def case_abi(backend):
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        assert hasattr(s.lib, "sdx_osc_torques") and "sdx_osc_torques" in _abi.SDX_EXPORTS
        assert _abi.SDX_ABI_VERSION == 8 and len(_abi.T) == 56
        assert C.sizeof(_abi.OscAttr) == 4 * (6 + 6 + 7 + 7 + 7 + 1 + 1)
        dp, u, w = dev(torch.zeros(N, 6)), dev(torch.zeros(N, ND)), dev(torch.zeros(N, 6))
        P = lambda t: C.c_void_p(t.data_ptr())                                      # noqa: E731
        good = _gains(s).to_attr()
        call = s.lib.sdx_osc_torques
        assert call(None, C.byref(good), P(dp), P(u), P(w), None) == -1             # NULL handle
        for args, word in (((None, P(dp), P(u), P(w)), b"attr is NULL"), ((C.byref(good), None, P(u), P(w)), b"dpose_dev is NULL"),
                           ((C.byref(good), P(dp), None, P(w)), b"torques_dev is NULL")):
            assert call(s.h, *args, None) == -1
            assert b"sdx_osc_torques: " + word in s.lib.sdx_last_error(s.h), s.lib.sdx_last_error(s.h)
        for field, k in (("kp", 2), ("kd", 5), ("kp_null", 0), ("kd_null", 6)):
            for bad in (-1.0, float("nan"), float("inf")):
                a = _gains(s).to_attr()
                getattr(a, field)[k] = bad
                assert call(s.h, C.byref(a), P(dp), P(u), P(w), None) == -1, (field, bad)
                assert b"sdx_osc_torques: kp, kd, kp_null and kd_null" in s.lib.sdx_last_error(s.h)
        for bad in (-0.01, float("nan"), float("inf")):
            a = _gains(s).to_attr()
            a.damping = bad
            assert call(s.h, C.byref(a), P(dp), P(u), P(w), None) == -1, bad
            assert b"sdx_osc_torques: damping" in s.lib.sdx_last_error(s.h)
        a = _gains(s).to_attr()
        a.q_null[3] = float("nan")
        assert call(s.h, C.byref(a), P(dp), P(u), P(w), None) == -1
        assert call(s.h, C.byref(good), P(dp), P(u), None, None) == 0                # no wrench asked for
        assert call(s.h, C.byref(good), P(dp), P(u), P(w), None) == 0
        # the Python side: the tensor checks of apply_dof_forces
        g = _gains(s)
        for bad in (dev(torch.zeros(N, 7)), dev(torch.zeros(N, 6, dtype=torch.float64)), dev(torch.zeros(N, 12))[:, ::2], [0.0], None):
            _expect_value_error(lambda: s.osc_torques(bad, g), "dpose")
        for bad in (dev(torch.zeros(N, ND + 1)), dev(torch.zeros(N, ND, dtype=torch.float64)), dev(torch.zeros(N, 2 * ND))[:, ::2]):
            _expect_value_error(lambda: s.osc_torques(dp, g, out=bad), "out")
        if dp.device.type != "cpu":
            _expect_value_error(lambda: s.osc_torques(dp.cpu(), g), "dpose")
        try:
            s.osc_torques(dp, tc.OscGains(damping=-1.0))
        except Exception as err:                                                    # the library's own message
            assert "damping" in str(err)
        else:
            raise AssertionError("negative damping accepted")
        t1 = s.osc_torques(dp, g)
        t2, w2 = s.osc_torques(dp, g, wrench=True)
        assert tuple(t1.shape) == (N, ND) and tuple(w2.shape) == (N, 6) and t1.data_ptr() == t2.data_ptr()      # allocated once
        assert s.osc_torques(dp, g, wrench=True)[1].data_ptr() == w2.data_ptr()
        assert s.osc_torques(dp, g, out=u).data_ptr() == u.data_ptr()
        assert s.osc_torques(dp, good).data_ptr() == t1.data_ptr()                  # a ready OscAttr
        s.apply_dof_forces(t1, ARM)                                                 # the row is what apply_dof_forces takes
        s.apply_dof_forces()
    finally:
        s.close()


def case_gains_and_pose_error():
    """OscGains' defaults are critically damped; pose_error is the position difference and sign(w) 2 xyz of target (x) conj(current)"""
    g = tc.OscGains()
    assert g.kp == (100.0,) * 6 and g.kd == (20.0,) * 6 and g.kp_null == (10.0,) * 7 and g.compensate_bias is True and g.damping == 0.05
    np.testing.assert_allclose(g.kd_null, 2 * np.sqrt(10.0))
    assert tc.OscGains(kp=[1, 4, 9, 16, 25, 36]).kd == (2.0, 4.0, 6.0, 8.0, 10.0, 12.0)
    _expect_value_error(lambda: tc.OscGains(kp=[1.0, 2.0]), "kp")
    a = tc.OscGains(kd=3.0, q_null=range(7), compensate_bias=False).to_attr()
    assert list(a.kd) == [3.0] * 6 and list(a.q_null) == [float(i) for i in range(7)] and a.compensate_bias == 0

    def quat(axis, angle):
        ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
        return np.concatenate([ax * np.sin(angle / 2), [np.cos(angle / 2)]])

    def mul(a, b):
        av, bv = a[:3], b[:3]
        return np.concatenate([a[3] * bv + b[3] * av + np.cross(av, bv), [a[3] * b[3] - av @ bv]])

    rng = np.random.default_rng(5)
    cur = np.stack([quat(rng.normal(size=3), rng.uniform(0, 3)) for _ in range(N)])
    axes, angles = rng.normal(size=(N, 3)), np.array([0.15, 1.0, 3.5])              # (3.5 rad: w < 0, the short way round is the other sign)
    tgt = np.stack([mul(quat(axes[e], angles[e]), cur[e]) for e in range(N)])
    pos, tpos = rng.normal(size=(N, 3)), rng.normal(size=(N, 3))
    got = tc.pose_error(*[torch.from_numpy(a.astype(f32)) for a in (pos, cur, tpos, tgt)]).numpy()
    assert got.shape == (N, 6) and got.dtype == f32
    want = np.stack([axes[e] / np.linalg.norm(axes[e]) * 2 * np.sin(angles[e] / 2) * np.sign(np.cos(angles[e] / 2)) for e in range(N)])
    np.testing.assert_allclose(got[:, :3], (tpos - pos).astype(f32), rtol=0, atol=1e-6)
    np.testing.assert_allclose(got[:, 3:], want, rtol=0, atol=2e-6)
    same = tc.pose_error(*[torch.from_numpy(a.astype(f32)) for a in (pos, cur, pos, cur)]).numpy()
    np.testing.assert_allclose(same, 0.0, rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------ 2. against float64
def case_against_float64(backend):
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        rng = np.random.default_rng(123)
        q, qd = _draw_state(s, rng)
        D._place(s, dev, q, qd)
        return _against_float64(s, dev, _draw_dpose(rng), _gains(s), "osc against float64")[:4]
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 3. damping, near-singular
def case_near_singular(backend):
    """q[3] at its upper limit: the elbow nearly straight.  damping = 0.05 within the bar measured at this configuration, and damping = 0
    differs from it by more than that bar: the term is used"""
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        rng = np.random.default_rng(131)
        q, qd = _draw_state(s, rng)
        q[:, 3] = f32(D._limits(s)[1][3])
        D._place(s, dev, q, qd)
        dpose = _draw_dpose(rng)
        yu, du, yw, dw, r64, u = _against_float64(s, dev, dpose, _gains(s, damping=0.05), "near-singular arm, damping 0.05")
        u0, _ = _call(s, dev, dpose, _gains(s, damping=0.0))
        apart = min(_rel(u0[e, :NA], u[e, :NA]) for e in range(N))
        print("near-singular arm: damping 0 against 0.05 differ by %.3g of the row's largest entry = %.3g bars" % (apart, apart / (MARGIN * yu)))
        assert apart > MARGIN * yu, (apart, yu)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 4. identities
def case_identities(backend):
    """in float64 from the engine's outputs, damping = 0: (a) no posture gains, no compensation: J M7^-1 u == F; (b) kp = kd = 0:
    J M7^-1 u == 0.  Bars: MARGIN x the residual of the float32 law on the same draws."""
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        rng = np.random.default_rng(141)
        q, qd = _draw_state(s, rng)
        D._place(s, dev, q, qd)
        dpose = _draw_dpose(rng)
        inp, effort = _inputs(s), _effort(s)
        for name, gains in (("task only", _gains(s, damping=0.0, kp_null=0.0, kd_null=0.0, compensate_bias=False)),
                            ("null space only", _gains(s, damping=0.0, kp=0.0, kd=0.0, compensate_bias=False))):
            r64 = _law(inp, dpose, gains, effort, np.float64)
            r32 = _law(inp, dpose, gains, effort, np.float32)
            u, _ = _call(s, dev, dpose, gains)
            res32 = res = big = 0.0
            for e in range(N):
                assert (np.abs(r64[e].u) < 0.9 * effort[:NA]).all() and np.abs(r64[e].u).max() > 0, (name, r64[e].u)
                F = r64[e].F
                res32 = max(res32, float(np.abs(O.task_acceleration(inp["M"][e], inp["J"][e], r32[e].u) - F).max()))
                res = max(res, float(np.abs(O.task_acceleration(inp["M"][e], inp["J"][e], u[e, :NA]) - F).max()))
                big = max(big, float(np.abs(O.task_acceleration(inp["M"][e], inp["J"][e], r64[e].u_null if name != "task only" else r64[e].u)).max()))
            print("identity %s: |J M7^-1 u - F| float32 law %.3g, engine %.3g (bar %.3g); the term it cancels or meets is %.3g" % (
                name, res32, res, MARGIN * res32, big))
            assert res32 > 0 and res <= MARGIN * res32, (name, res, res32)
            assert big > 1000 * MARGIN * res32, (name, big, res32)                   # the identity is no accident of small numbers
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 5. exact parts
def case_exact(backend):
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        rng = np.random.default_rng(151)
        q, qd = _draw_state(s, rng)
        D._place(s, dev, q, qd)
        dpose = _draw_dpose(rng)
        effort = _effort(s)
        u, _ = _call(s, dev, dpose, _gains(s))
        assert (u[:, NA:].view(np.uint32) == 0).all(), "the hand's columns are +0.0"
        assert (u[:, :NA] != 0).all()
        zero = tc.OscGains(kp=0.0, kd=0.0, kp_null=0.0, kd_null=0.0, q_null=D._mid(s)[:NA], compensate_bias=False)
        u0, w0 = _call(s, dev, dpose, zero)
        assert (u0.view(np.uint32) == 0).all(), "all gains zero: the row is +0.0"
        assert (w0 == 0).all()
        # compensation on minus off == bias[0:7], within one ulp of the larger term
        on, _ = _call(s, dev, dpose, _gains(s, compensate_bias=True))
        off, _ = _call(s, dev, dpose, _gains(s, compensate_bias=False))
        bias = D._dyn(s, mass=False, drive=False).bias[:, :NA]
        assert np.abs(bias).max() > 1.0
        ulp = np.spacing(np.maximum(np.maximum(np.abs(on[:, :NA]), np.abs(off[:, :NA])), np.abs(bias))).astype(np.float64)
        err = np.abs(on[:, :NA].astype(np.float64) - off[:, :NA] - bias) / ulp
        print("exact parts: compensation on - off against bias[0:7]: %.2f ulp of the larger term at most, largest |bias| %.3g N m" % (
            err.max(), np.abs(bias).max()))
        assert (err <= 1.0).all(), err.max()
        # beyond the effort limit: exactly +-effort
        stiff = _gains(s, kp=1.0e4, kd=0.0)                                         # some entries beyond the limit, some inside it
        r64 = _law(_inputs(s), dpose, stiff, effort, np.float64)
        u64 = np.stack([r.u for r in r64])
        over = np.abs(u64) > 1.01 * effort[:NA]
        inside = np.abs(u64) < 0.99 * effort[:NA]
        big, _ = _call(s, dev, dpose, stiff)
        print("exact parts: %d arm entries beyond the effort limit, %d inside it" % (int(over.sum()), int(inside.sum())))
        assert over.sum() >= 3 and inside.sum() >= 3
        np.testing.assert_array_equal(big[:, :NA][over], (np.sign(u64) * effort[:NA])[over].astype(f32))
        np.testing.assert_allclose(big[:, :NA][inside], u64[inside], rtol=0, atol=1e-4 * np.abs(u64).max())   # (untouched by the clamp; how close is case 2's matter)
        assert (big[:, NA:].view(np.uint32) == 0).all()
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 6. randomization
def case_randomization(backend):
    """link mass factors 0.7 .. 1.5 in SDX_T_DR_LINK: the helper fed with the scaled M (dof_dynamics() with randomization on) is met within
    the bar, the unscaled M is many bars away"""
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        rng = np.random.default_rng(161)
        q, qd = _draw_state(s, rng)
        D._place(s, dev, q, qd)
        dpose = _draw_dpose(rng)
        plain = _inputs(s)                                                          # before randomization is on: the scene's masses
        gains = _gains(s)
        D._dr_on(s, dev, link_factor=np.linspace(0.7, 1.5, NL, dtype=f32))
        yu, du, yw, dw, r64, u = _against_float64(s, dev, dpose, gains, "osc with link mass factors")
        scaled = _inputs(s)
        assert np.abs(scaled["M"] - plain["M"]).max() > 0.05
        unscaled = _law(dict(scaled, M=plain["M"], b=plain["b"]), dpose, gains, _effort(s), np.float64)
        away = min(_rel(u[e, :NA], unscaled[e].u) for e in range(N))
        print("osc with link mass factors: the unscaled expectation is %.3g away = %.0f bars" % (away, away / (MARGIN * yu)))
        assert away > 100 * MARGIN * yu, (away, yu)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 7. closed loop
def _closed_loop(backend, kp, seconds):
    """the arm under osc_torques, the hand on its PD drives, through the unchanged physics step.  Returns (errors [steps + 1, 2, N]: position
    (m) and rotation (rad) error norms before every step and after the last, |u| / effort [steps, N, 7])"""
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        q = np.tile(D._mid(s).astype(f32), (N, 1))
        D._place(s, dev, q)
        ee = int(s._desc.hand_base_body)
        rb = s.RB.reshape(N, -1, 13)
        pos0, quat0 = rb[:, ee, 0:3].clone(), rb[:, ee, 3:7].clone()
        half = 0.5 * 0.15
        ry = torch.tensor([0.0, np.sin(half), 0.0, np.cos(half)], dtype=torch.float32)
        c = quat0.cpu()
        tq = torch.stack([ry[3] * c[:, 0] + ry[1] * c[:, 2], ry[3] * c[:, 1] + ry[1] * c[:, 3], ry[3] * c[:, 2] - ry[1] * c[:, 0],
                          ry[3] * c[:, 3] - ry[1] * c[:, 1]], -1)                    # (0, sy, 0, cy) (x) current
        target_quat = dev(tq.contiguous())
        target_pos = pos0 + dev(torch.tensor([0.04, 0.0, 0.04]))
        gains = tc.OscGains(kp=kp, kd=2.0 * np.sqrt(kp), kp_null=10.0, kd_null=2.0 * np.sqrt(10.0), q_null=q[0, :NA], compensate_bias=True)
        effort = _effort(s)[:NA]
        steps = int(round(seconds / float(s._desc.dt)))
        errs, load = [], []
        for i in range(steps + 1):
            rb = s.RB.reshape(N, -1, 13)
            dpose = tc.pose_error(rb[:, ee, 0:3], rb[:, ee, 3:7], target_pos, target_quat)
            d = host(dpose)
            errs.append([np.linalg.norm(d[:, :3], axis=1), np.linalg.norm(d[:, 3:], axis=1)])
            if i == steps:
                break
            u = s.osc_torques(dpose, gains)
            load.append(np.abs(host(u)[:, :NA]) / effort)
            s.apply_dof_forces(u, ARM)
            s.simulate()
        assert (host(s.CONTACT).reshape(N, D.NB, 3)[:, :NL] == 0).all(), "something touches the robot"
        return np.array(errs), np.array(load), float(s._desc.dt)
    finally:
        s.close()


def case_closed_loop(backend):
    """kp = 100, kd = 20 (critically damped, omega = 10 / s): after 1 s the analytic error is (1 + 10) e^-10 = 0.05 % of the initial one;
    both errors below 5 %, no arm torque at its limit after the first ten steps; kp tripled is closer at t = 0.25 s"""
    errs, load, dt = _closed_loop(backend, 100.0, 1.0)
    at = lambda t: int(round(t / dt))                                               # noqa: E731
    e0 = errs[0]
    np.testing.assert_allclose(e0[0], np.hypot(0.04, 0.04), rtol=1e-4)
    np.testing.assert_allclose(e0[1], 2 * np.sin(0.075), rtol=1e-4)
    for t in (0.25, 0.5, 1.0):
        print("closed loop, kp 100: t = %.2f s: position error %.3g m (%.2f %%), rotation error %.3g rad (%.2f %%)" % (
            t, errs[at(t)][0].max(), 100 * (errs[at(t)][0] / e0[0]).max(), errs[at(t)][1].max(), 100 * (errs[at(t)][1] / e0[1]).max()))
    print("closed loop, kp 100: largest |u| / effort %.3g in the first ten steps, %.3g after them" % (load[:10].max(), load[10:].max()))
    stiff, _, _ = _closed_loop(backend, 300.0, 0.25)
    k = at(0.25)
    print("closed loop at t = 0.25 s: kp 100: %.3g m, %.3g rad; kp 300: %.3g m, %.3g rad" % (
        errs[k][0].max(), errs[k][1].max(), stiff[k][0].max(), stiff[k][1].max()))
    assert (errs[-1][0] < 0.05 * e0[0]).all() and (errs[-1][1] < 0.05 * e0[1]).all(), (errs[-1], e0)
    assert (load[10:] < 1.0).all(), load[10:].max()
    assert (stiff[k][0] < errs[k][0]).all() and (stiff[k][1] < errs[k][1]).all(), (stiff[k], errs[k])


# ------------------------------------------------------------------------------------------------------------------ 8. independence
def case_independence(backend):
    """a call leaves SDX_T_DOF, SDX_T_TARGETS and SDX_T_JAC_EEF bit for bit; a run that calls every step and never applies the result is a
    run without the calls"""
    make, dev = backend
    rng = np.random.default_rng(181)
    s = make(N, seed=SEED)
    try:
        q, qd = _draw_state(s, rng)
    finally:
        s.close()
    dpose = _draw_dpose(rng)

    def run(calls):
        s = make(N, seed=SEED)
        try:
            D._place(s, dev, q, (0.2 * qd).astype(f32))
            out = []
            for _ in range(3):
                if calls:
                    before = [host(t).view(np.uint32) for t in (s.DOF, s.TARGETS, s.JAC_EEF)]
                    u, _ = _call(s, dev, dpose, _gains(s))
                    assert np.abs(u[:, :NA]).max() > 1.0
                    for name, b, t in zip(("DOF", "TARGETS", "JAC_EEF"), before, (s.DOF, s.TARGETS, s.JAC_EEF)):
                        np.testing.assert_array_equal(host(t).view(np.uint32), b, err_msg=name)
                s.simulate()
                out.append([host(t).view(np.uint32) for t in (s.DOF, s.ROOT, s.RB, s.JAC_EEF, s.CONTACT)])
            return out
        finally:
            s.close()

    a, b = run(True), run(False)
    for i in range(3):
        for name, x, y in zip(("DOF", "ROOT", "RB", "JAC_EEF", "CONTACT"), a[i], b[i]):
            np.testing.assert_array_equal(x, y, err_msg="%s, step %d" % (name, i))
    assert (a[2][0] != a[0][0]).any()


def case_n_against_2n(backend, randomize):
    make, dev = backend
    outs = []
    for n in (N, 2 * N):
        s = make(n, seed=SEED)
        try:
            r = np.random.default_rng(192)
            q, qd = _draw_state(s, r, n=2 * N)
            dpose = _draw_dpose(r, n=2 * N)
            if randomize:
                D._dr_on(s, dev, link_factor=np.linspace(0.8, 1.3, NL, dtype=f32))
            D._place(s, dev, q[:n], qd[:n])
            outs.append(_call(s, dev, dpose[:n], _gains(s)))
        finally:
            s.close()
    for name, a, b in zip(("torques", "wrench"), *outs):
        np.testing.assert_array_equal(a.view(np.uint32), b[:N].view(np.uint32), err_msg=name)
        assert np.abs(a).max() > 0
