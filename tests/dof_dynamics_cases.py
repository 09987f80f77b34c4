"""Shared bodies of the joint-torque tests (include/seqdex.h sdx_apply_dof_forces / sdx_dof_dynamics):
tests/test_dof_dynamics.py runs them on the emulated simulator (tests/hipemu), tests/test_gpu_dof_dynamics.py on the GPU.  A `backend` is
(make, dev): make(n, **desc) builds a simulator, dev(tensor) moves a host tensor to where its tensors live.  The references are the
unchanged C oracle (oracle/physics_oracle.py), a float64 numpy CRBA (tests/helpers/crba_float64.py) for the oracle's own rounding, the
numpy formula of the drive, and equivalences between two runs of the engine.  N = 3 everywhere."""
import ctypes as C

import numpy as np
import torch

import state_snapshot_cases as SC
from helpers import crba_float64
from oracle import physics_oracle as po
from seqdex_amd import _abi
from seqdex_amd import domain_randomization as dr
from seqdex_amd import torque_control as tc

f32 = np.float32
SEED = 22
N = 3
NB, A0, NF, NL, ND = _abi.BODIES, _abi.ACTOR_BRICK0, _abi.NFREE, _abi.NLINK, _abi.NDOF
NEVER = 10 ** 9
ALL = (1 << ND) - 1
ARM = (1 << 7) - 1
K_SOFT = 1e-3            # the gain that turns a DOF of the oracle into a torque source: kp = k, kd = -h k, target = q + u / k


def host(t):
    return t.detach().cpu().numpy().copy()


def _limits(s):
    return np.asarray(s.scene.lower, np.float64), np.asarray(s.scene.upper, np.float64)


def _mid(s):
    lo, up = _limits(s)
    return 0.5 * (lo + up)


def _place(s, dev, q, qd=None, targets=None):
    """joint state and targets of every env ([n, 23] each); the free bricks far from the robot"""
    n = s.num_envs
    dof = np.zeros((n, ND, 2), f32)
    dof[:, :, 0] = q
    if qd is not None:
        dof[:, :, 1] = qd
    s.DOF.copy_(dev(torch.from_numpy(dof.reshape(-1, 2))))
    tg = np.ascontiguousarray(q if targets is None else targets, f32)
    s.TARGETS.copy_(dev(torch.from_numpy(np.broadcast_to(tg, (n, ND)).copy())))
    root = host(s.ROOT).reshape(n, _abi.ACTORS, 13)
    root[:, A0:A0 + NF, 0] += 5.0
    s.ROOT.copy_(dev(torch.from_numpy(root.reshape(-1, 13))))
    s.WARM_COUNT.zero_()
    s.refresh_kinematics()
    return root, dof


def _dofs(s):
    return host(s.DOF).reshape(s.num_envs, ND, 2)


def _dyn(s, **kw):
    d = s.dof_dynamics(**kw)
    return tc.DofDynamics(*[None if t is None else host(t) for t in d])


def _draw_q(s, rng, n=N, spread=None):
    lo, up = _limits(s)
    if spread is None:
        return (lo + (up - lo) * rng.uniform(0.1, 0.9, (n, ND))).astype(f32)
    return (_mid(s) + rng.uniform(-spread, spread, (n, ND))).astype(f32)


def _dr_on(s, dev, link_factor=None, gain_scale=None):
    s.set_randomization(dr.identity_desc(NEVER))
    if link_factor is not None:
        lk = host(s.DR_LINK)
        lk[:, 0, :] = link_factor
        s.DR_LINK.copy_(dev(torch.from_numpy(lk)))
    if gain_scale is not None:
        dd = host(s.DR_DOF)
        dd[:, 0, :] *= f32(gain_scale[0])
        dd[:, 1, :] *= f32(gain_scale[1])
        s.DR_DOF.copy_(dev(torch.from_numpy(dd)))
    return host(s.DR_DOF)


# ------------------------------------------------------------------------------------------------------------------ 1. ABI
def case_abi(backend):
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        assert hasattr(s.lib, "sdx_apply_dof_forces") and hasattr(s.lib, "sdx_dof_dynamics")
        assert "sdx_apply_dof_forces" in _abi.SDX_EXPORTS and "sdx_dof_dynamics" in _abi.SDX_EXPORTS
        assert _abi.SDX_ABI_VERSION == 8 and len(_abi.T) == 56
        u = dev(torch.zeros(N, ND))
        out = dev(torch.zeros(N, ND))
        assert s.lib.sdx_apply_dof_forces(None, C.c_void_p(u.data_ptr()), 0, None) == -1               # NULL handle
        assert s.lib.sdx_dof_dynamics(None, None, C.c_void_p(out.data_ptr()), None, None) == -1
        assert s.lib.sdx_apply_dof_forces(s.h, C.c_void_p(u.data_ptr()), 1 << ND, None) == -1          # mask bit 23
        assert b"sdx_apply_dof_forces: drive_off_mask" in s.lib.sdx_last_error(s.h)
        assert s.lib.sdx_apply_dof_forces(s.h, None, 1 << 31, None) == -1
        assert s.lib.sdx_dof_dynamics(s.h, None, None, None, None) == -1                               # all outputs NULL
        assert b"sdx_dof_dynamics: mass_dev, bias_dev and drive_dev are all NULL" in s.lib.sdx_last_error(s.h)
        assert s.lib.sdx_apply_dof_forces(s.h, C.c_void_p(u.data_ptr()), ALL, None) == 0
        assert s.lib.sdx_apply_dof_forces(s.h, None, 0, None) == 0                                     # clears
        # the Python side: the checks of apply_rigid_body_forces
        for bad in (dev(torch.zeros(N, ND + 1)), dev(torch.zeros(N, ND, dtype=torch.float64)), dev(torch.zeros(N, 2 * ND))[:, ::2], [0.0]):
            try:
                s.apply_dof_forces(bad)
            except ValueError as err:
                assert "forces" in str(err)
            else:
                raise AssertionError("a bad forces tensor was accepted")
        for bad in ([ND], [-1], 1 << 40):
            try:
                s.apply_dof_forces(u, bad)
            except ValueError as err:
                assert "drive_off" in str(err)
            else:
                raise AssertionError("accepted drive_off = %r" % (bad,))
        try:
            s.apply_dof_forces(u, 1 << ND)
        except Exception as err:                                                                       # the library's own message
            assert "drive_off_mask" in str(err)
        else:
            raise AssertionError("mask bit 23 accepted")
        s.apply_dof_forces(u, [0, 5, 22])
        s.apply_dof_forces(None, ARM)
        s.apply_dof_forces()
        d = s.dof_dynamics(mass=False, drive=False)
        assert d.mass is None and d.drive is None and tuple(d.bias.shape) == (N, ND)
        d2 = s.dof_dynamics()
        assert tuple(d2.mass.shape) == (N, ND, ND) and d2.bias.data_ptr() == d.bias.data_ptr()         # allocated once
        assert s.dof_dynamics().mass.data_ptr() == d2.mass.data_ptr()
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 2. off and zero
def case_off_and_zero(backend, golden_dir, n, randomize):
    """three steps from the contact-rich P1 state, warm start on: no call == apply_dof_forces(zeros, 0) every step (the FORCE instantiation)
    and, from step 2 on, a run that had a one-shot call at step 1 == a run whose step-1 result was copied in and that never called"""
    make, dev = backend
    acts = SC.actions(n, 3, seed=11)

    def start():
        s = SC.make_scene_sim(backend, golden_dir, n, warm_start=0.8)
        if randomize:
            s.set_randomization(dr.identity_desc(NEVER))
        return s

    a = start()
    try:
        base = SC.run(a, dev, acts)
        assert int(base[-1]["NCONTACTS"].min()) > 100
    finally:
        a.close()
    b = start()
    try:
        z = np.zeros((n, ND), f32)
        z[:, ::2] = -0.0                                                          # negative zeros are zeros too
        zu = dev(torch.from_numpy(z))
        for i, act in enumerate(acts):
            b.apply_dof_forces(zu, 0)
            b.step(dev(act))
            SC.assert_records_equal(b, base[i], SC.record(b), "zero DOF forces, step %d" % i)
    finally:
        b.close()
    c, d = start(), start()
    try:
        u = np.zeros((n, ND), f32)
        u[:, 1], u[:, 3], u[:, 9] = 30.0, -20.0, 0.05
        c.apply_dof_forces(dev(torch.from_numpy(u)), [5, 12])
        c.step(dev(acts[0]))
        first = SC.record(c)
        assert (first["DOF"] != base[0]["DOF"]).any(), "the one-shot call moved nothing"
        st = c.snapshot()
        st.save()
        st.restore(sim=d)                                                         # the step-1 result, copied into a simulator that never called
        for i in (1, 2):
            c.step(dev(acts[i]))
            d.step(dev(acts[i]))
            SC.assert_records_equal(c, SC.record(d), SC.record(c), "after the one-shot call, step %d" % i)
        st.close()
    finally:
        c.close()
        d.close()


# ------------------------------------------------------------------------------------------------------------------ 3. mass matrix
def case_mass_matrix(backend, link_factor=None):
    """three random q inside the limits.  Reference: oracle.physics_oracle.mass_matrix(desc, q, 0.0) (H at h = 0 is M + armature).  Bar:
    the oracle's own float32 deviation from the float64 CRBA of tests/helpers/crba_float64.py over these configurations, as the largest
    |dH_ij| / sqrt(M_ii M_jj), times 4 (fma contraction plus fk_wave0's path sums against the oracle's recursion), entrywise times
    sqrt(M_ii M_jj).  Returns (oracle deviation, engine deviation from the oracle), both relative."""
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        rng = np.random.default_rng(31)
        q = _draw_q(s, rng)
        _place(s, dev, q)
        desc = s._desc
        fac = None
        if link_factor is not None:
            fac = np.asarray(link_factor, f32)
            _dr_on(s, dev, link_factor=fac)
            desc = s.scene.to_desc()                                              # the oracle's descriptor: masses and inertias scaled
            for k in range(NL):
                desc.link_mass[k] = f32(desc.link_mass[k]) * fac[k]
                for r in range(6):
                    desc.link_inertia[k][r] = f32(desc.link_inertia[k][r]) * fac[k]
        M = _dyn(s, bias=False, drive=False).mass
        assert M.shape == (N, ND, ND)
        worst_o = worst_e = 0.0
        rel_o, rows = [], []
        for e in range(N):
            H = po.mass_matrix(desc, q[e], 0.0)[0].astype(np.float64)
            M64 = crba_float64.mass_matrix(s._desc, q[e], fac)
            scale = np.sqrt(np.outer(np.diag(M64), np.diag(M64)))
            rel_o.append(np.abs(H - M64) / scale)
            rows.append((H, scale))
        worst_o = float(np.max(rel_o))
        assert 0 < worst_o < 1e-5, worst_o                                         # float32 rounding, not a modelling difference
        for e in range(N):
            np.testing.assert_array_equal(M[e].view(np.uint32), M[e].T.copy().view(np.uint32), err_msg="M == M.T bitwise, env %d" % e)
            H, scale = rows[e]
            rel = np.abs(M[e].astype(np.float64) - H) / scale
            worst_e = max(worst_e, float(rel.max()))
        print("mass matrix (factor %s): oracle vs float64 %.3g, engine vs oracle %.3g (bar %.3g), relative to sqrt(M_ii M_jj)" % (
            "on" if fac is not None else "off", worst_o, worst_e, 4 * worst_o))
        for e in range(N):
            H, scale = rows[e]
            assert (np.abs(M[e].astype(np.float64) - H) <= 4 * worst_o * scale).all(), (e, worst_e, worst_o)
        if fac is not None:                                                        # the factors matter: far beyond the bar without them
            H0 = po.mass_matrix(s._desc, q[0], 0.0)[0].astype(np.float64)
            assert (np.abs(M[0] - H0) / rows[0][1]).max() > 1000 * 4 * worst_o
        return worst_o, worst_e
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 4. bias
def _oracle_bias(desc, root, q, qd, h):
    """-H (qd' - qd) / h from one oracle step of a robot without drive, damping or velocity limit, H = mass_matrix(desc, q, h)"""
    n = q.shape[0]
    dof = np.zeros((n, ND, 2), f32)
    dof[:, :, 0], dof[:, :, 1] = q, qd
    r = root.copy()
    po.simulate(desc, r, dof, np.ascontiguousarray(q, f32))
    out = np.zeros((n, ND))
    for e in range(n):
        H = po.mass_matrix(desc, q[e], h)[0].astype(np.float64)
        out[e] = -H @ ((dof[e, :, 1].astype(np.float64) - qd[e].astype(np.float64)) / h)
    return out


def case_bias(backend):
    """bias against the unchanged oracle: kp = kd = 0, no damping, one substep, no velocity limit, nothing in reach - one oracle step gives
    bias = -H (qd' - qd) / h.  q = mid-range +- 0.2, arm |qd| <= 1.5 rad/s, hand |qd| <= 2 rad/s.  Bar: 4 x the quadratic defect of the
    recovered vector - a quadratic form is homogeneous of degree 2 and even: the larger of max |b(qd) - 4 b(qd / 2)| and
    max |b(qd) - b(-qd)| over these draws - measured here on the oracle.  bias(qd = 0) == 0 exactly.
    Returns (defect, engine's largest difference, largest |bias|)."""
    make, dev = backend
    over = dict(kp=[0.0] * ND, kd=[0.0] * ND, robot_angular_damping=0.0, substeps=1, vel_limit=[1e6] * ND)
    s = make(N, seed=SEED, **over)
    try:
        rng = np.random.default_rng(41)
        q = _draw_q(s, rng, spread=0.2)
        qd = np.concatenate([rng.uniform(-1.5, 1.5, (N, 7)), rng.uniform(-2.0, 2.0, (N, ND - 7))], 1).astype(f32)
        root, _ = _place(s, dev, q, qd)
        h = float(s._desc.dt)
        b1 = _oracle_bias(s._desc, root, q, qd, h)
        bh = _oracle_bias(s._desc, root, q, (0.5 * qd).astype(f32), h)             # (halving a float32 is exact)
        bm = _oracle_bias(s._desc, root, q, -qd, h)
        defect = float(max(np.abs(b1 - 4.0 * bh).max(), np.abs(b1 - bm).max()))    # homogeneous of degree 2, and even
        got = _dyn(s, mass=False, drive=False).bias.astype(np.float64)
        diff = float(np.abs(got - b1).max())
        print("bias: oracle's quadratic defect %.3g N m, engine - oracle max %.3g N m (bar %.3g), largest |bias| %.3g N m" % (
            defect, diff, 4 * defect, np.abs(b1).max()))
        assert 1.0 < np.abs(b1).max() < 20.0 and 0 < defect < 1e-3, (np.abs(b1).max(), defect)
        assert diff <= 4 * defect, (diff, defect)
        _place(s, dev, q)                                                          # qd = 0
        np.testing.assert_array_equal(_dyn(s, mass=False, drive=False).bias, 0.0)
        return defect, diff, float(np.abs(b1).max())
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 5. drive
def case_drive(backend, randomize):
    """the clamped PD torque against the numpy formula t = kp (tgt - q) - (kd + h kp) qd in float64 from the float32 operands: entries beyond
    the effort limit are exactly +-effort, the rest within 2 ulp.  The velocities have the sign of q - tgt, so that the two products
    do not cancel and an ulp of the result is no smaller than an ulp of either.  Some arm DOFs are driven beyond 200 N m, some hand DOFs
    beyond 5 N m.  With randomization on the gains are the env's SDX_T_DR_DOF rows (scaled away from the scene's)."""
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        rng = np.random.default_rng(51)
        d = s._desc
        effort = np.array([f32(v) for v in d.effort], f32)
        kp, kd = np.array([f32(v) for v in d.kp], f32), np.array([f32(v) for v in d.kd], f32)
        if randomize:
            rows = _dr_on(s, dev, gain_scale=(1.3, 0.7))
            kp_e, kd_e = rows[:, 0, :], rows[:, 1, :]
            assert (kp_e != kp).all()
        else:
            kp_e, kd_e = np.tile(kp, (N, 1)), np.tile(kd, (N, 1))
        q = _draw_q(s, rng, spread=0.1)
        off = rng.uniform(0.01, 0.05, (N, ND)) * rng.choice([-1.0, 1.0], (N, ND))
        over = np.zeros((N, ND), bool)
        over[:, [0, 2, 5, 8, 13, 20]] = True                                       # beyond the limit: 3 x effort / kp away
        off[over] = (3.0 * effort / kp)[None, :].repeat(N, 0)[over] * np.sign(off[over])
        tgt = (q + off).astype(f32)
        qd = (-np.sign(tgt.astype(np.float64) - q) * rng.uniform(0.05, 0.5, (N, ND))).astype(f32)
        _place(s, dev, q, qd, tgt)
        h = f32(d.dt) / f32(int(d.substeps))
        t = kp_e.astype(np.float64) * (tgt.astype(np.float64) - q) - (kd_e.astype(np.float64) + float(h) * kp_e) * qd
        clamped = np.abs(t) > effort * 1.001
        assert clamped[:, :7].any() and clamped[:, 7:].any() and (~clamped).sum() > N * ND // 2
        assert (np.abs(t[:, :7])[clamped[:, :7]] > 200).all() and (np.abs(t[:, 7:])[clamped[:, 7:]] > 5).all()
        assert (np.abs(t[~clamped]) < 0.9 * np.tile(effort, (N, 1))[~clamped]).all()
        got = _dyn(s, mass=False, bias=False).drive
        want = np.clip(t, -effort, effort)
        np.testing.assert_array_equal(got[clamped], want[clamped].astype(f32))
        ulp = np.spacing(np.abs(want).astype(f32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want) / ulp
        print("drive (randomize %s): %d clamped entries exact, the rest within %.2f ulp" % (randomize, int(clamped.sum()), err[~clamped].max()))
        assert (err[~clamped] <= 2.0).all(), err[~clamped].max()
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 6. actuation
def _soft_desc(s, mask, substeps, hand_gains=None):
    """the oracle's descriptor: the DOFs of `mask` are torque sources (kp = k, kd = -h k: constant torque k (tgt - q0), nothing on the diagonal
    of H); hand_gains (kp, kd): the gains of the others"""
    d = s.scene.to_desc(substeps=substeps)
    h = f32(d.dt) / f32(substeps)
    for j in range(ND):
        if (mask >> j) & 1:
            d.kp[j], d.kd[j] = f32(K_SOFT), -h * f32(K_SOFT)
        elif hand_gains is not None:
            d.kp[j], d.kd[j] = f32(hand_gains[0][j]), f32(hand_gains[1][j])
    return d


def _actuate(backend, mask, u, q, qd, substeps=None, randomize=False):
    """one simulate() of the engine with apply_dof_forces(u, mask) beside one oracle step in which u is stated through targets: q + u / k on
    the DOFs of mask (soft gains), q + u / kp on the others (their PD drive).  Returns (engine dof, oracle dof, start dof)."""
    make, dev = backend
    kw = {} if substeps is None else dict(substeps=substeps)
    s = make(N, seed=SEED, **kw)
    try:
        nsub = int(s._desc.substeps)
        gains = None
        if randomize:
            rows = _dr_on(s, dev, gain_scale=(1.2, 0.8))
            gains = (rows[0, 0, :], rows[0, 1, :])                                 # (the same rows in every env: one oracle descriptor)
        root, dof = _place(s, dev, q, qd)
        desc = _soft_desc(s, mask, nsub, gains)
        kpo = np.array([float(v) for v in desc.kp])
        tg = (q.astype(np.float64) + u.astype(np.float64) / kpo).astype(f32)
        o_root, o_dof = root.copy(), dof.copy()
        _, o_contact, _, _ = po.simulate(desc, o_root, o_dof, tg)
        s.apply_dof_forces(dev(torch.from_numpy(u)), mask)
        s.simulate()
        g = _dofs(s)
        assert (host(s.CONTACT).reshape(N, NB, 3)[:, :NL] == 0).all() and (o_contact[:, :NL] == 0).all(), "something touches the robot"
        return g, o_dof, dof
    finally:
        s.close()


def _assert_dof_bars(g, o, what):
    dq, dv = np.abs(g[..., 0] - o[..., 0]), np.abs(g[..., 1] - o[..., 1])
    print("%s: |dq| max %.3g rad, |dqd| max %.3g rad/s, largest |qd'| %.3g rad/s" % (what, dq.max(), dv.max(), np.abs(o[..., 1]).max()))
    np.testing.assert_allclose(g[..., 0], o[..., 0], rtol=1e-4, atol=1e-4, err_msg=what)       # the DOF bars of test_one_step_teacher_forcing
    np.testing.assert_allclose(g[..., 1], o[..., 1], rtol=1e-3, atol=2e-3, err_msg=what)


def _torques(desc, q, rng, arm=40.0, hand=150.0):
    """u = M(q) a for random joint accelerations a (arm / hand bounds in rad/s^2): torques that move every DOF by a comparable dt a, well
    inside the effort and velocity limits"""
    a = np.concatenate([rng.uniform(-arm, arm, (N, 7)), rng.uniform(-hand, hand, (N, ND - 7))], 1)
    u = np.stack([crba_float64.mass_matrix(desc, q[e]) @ a[e] for e in range(N)])
    assert (np.abs(u) < 0.9 * np.array([float(v) for v in desc.effort])).all(), np.abs(u).max(0)
    return u.astype(f32)


def _start_state(backend, rng):
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        q = _draw_q(s, rng, spread=0.2)
        return s.scene.to_desc(), np.array([float(v) for v in s._desc.effort]), q
    finally:
        s.close()


def _below_vel_limit(desc, dof):
    return (np.abs(dof[..., 1]) < 0.95 * np.array([float(v) for v in desc.vel_limit])).all()


def case_actuation_all_off(backend):
    """(a) all 23 drives off, u within the effort limits, one substep"""
    rng = np.random.default_rng(61)
    desc, effort, q = _start_state(backend, rng)
    qd = rng.uniform(-0.2, 0.2, (N, ND)).astype(f32)
    u = _torques(desc, q, rng)
    g, o, start = _actuate(backend, ALL, u, q, qd, substeps=1)
    _assert_dof_bars(g, o, "actuation (a) all drives off")
    assert np.abs(o[..., 1] - start[..., 1]).max() > 1.0 and _below_vel_limit(desc, o)      # the torques move the robot, no limit cuts in


def case_actuation_arm_off(backend, randomize):
    """(b) / (d) the arm's drives off, the hand on its PD drive (at rest on its targets), shipped substeps; on the hand DOFs u reaches the oracle
    as the target shift u / kp.  randomize: the hand's gains are the env's SDX_T_DR_DOF rows, the arm's rows are the gains that are dropped"""
    rng = np.random.default_rng(62)
    desc, effort, q = _start_state(backend, rng)
    qd = np.zeros((N, ND), f32)
    qd[:, :7] = rng.uniform(-0.2, 0.2, (N, 7))
    u = _torques(desc, q, rng, hand=0.0)
    u[:, 7:] = rng.uniform(-0.5, 0.5, (N, ND - 7))                                 # (N m: a tenth of the hand's effort limit, on top of its PD drive)
    g, o, start = _actuate(backend, ARM, u, q, qd, randomize=randomize)
    _assert_dof_bars(g, o, "actuation (%s) arm drives off%s" % ("d" if randomize else "b", ", randomization on" if randomize else ""))
    assert np.abs(o[:, :7, 1] - start[:, :7, 1]).max() > 0.5 and np.abs(o[:, 7:, 1]).max() > 0.1 and _below_vel_limit(desc, o)


def case_actuation_clamp(backend):
    """(c) u = 3 x effort on one DOF equals u = effort bit for bit, and matches the oracle (whose drive clamps the same torque)"""
    rng = np.random.default_rng(63)
    _, effort, q = _start_state(backend, rng)
    qd = np.zeros((N, ND), f32)
    u3, u1 = np.zeros((N, ND), f32), np.zeros((N, ND), f32)
    for e, j in enumerate((1, 3, 10)):
        u3[e, j], u1[e, j] = 3 * effort[j] * (-1) ** e, effort[j] * (-1) ** e
    g3, o3, _ = _actuate(backend, ALL, u3, q, qd, substeps=1)
    g1, _, _ = _actuate(backend, ALL, u1, q, qd, substeps=1)
    np.testing.assert_array_equal(g3.view(np.uint32), g1.view(np.uint32))
    _assert_dof_bars(g3, o3, "actuation (c) 3 x effort")


# ------------------------------------------------------------------------------------------------------------------ 7. round trip
def case_round_trip(backend):
    """qd = 0, all drives off, shipped substeps: u = inverse_dynamics(dof_dynamics(), a) gives dqd = dt a within atol 2e-3 after one step
    (the damping factor 1 - h 0.01 per substep is inside the bar)"""
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        rng = np.random.default_rng(71)
        q = _draw_q(s, rng, spread=0.2)
        _place(s, dev, q)
        a = np.concatenate([rng.uniform(-2, 2, (N, 7)), rng.uniform(-5, 5, (N, ND - 7))], 1).astype(f32)
        dyn = s.dof_dynamics(drive=False)
        u = tc.inverse_dynamics(dyn, dev(torch.from_numpy(a))).contiguous()
        assert (np.abs(host(u)) < np.array([float(v) for v in s._desc.effort])).all()
        s.apply_dof_forces(u, ALL)
        s.simulate()
        g = _dofs(s)
        want = float(s._desc.dt) * a.astype(np.float64)
        print("round trip: |dqd - dt a| max %.3g rad/s on |dt a| max %.3g" % (np.abs(g[..., 1] - want).max(), np.abs(want).max()))
        assert (host(s.CONTACT).reshape(N, NB, 3)[:, :NL] == 0).all()
        np.testing.assert_allclose(g[..., 1], want, rtol=0, atol=2e-3)
        assert np.abs(want).max() > 10 * 2e-3
    finally:
        s.close()


def case_pd_torques():
    """torque_control.pd_torques restates morb.py:1292,1297: clip(p (targets - q) - d qd, -clip, clip), with numbers or tensors"""
    rng = np.random.default_rng(75)
    q, qd, tg = [rng.uniform(-1, 1, (N, ND)).astype(f32) for _ in range(3)]
    want = np.clip(f32(3.0) * (tg - q) - f32(0.1) * qd, -0.5, 0.5)
    got = tc.pd_torques(torch.from_numpy(q), torch.from_numpy(qd), torch.from_numpy(tg), 3.0, 0.1, 0.5).numpy()
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7)
    assert (np.abs(got) == f32(0.5)).any() and (np.abs(got) < f32(0.5)).any()
    p, d, c = [torch.from_numpy(rng.uniform(0.5, 2.0, ND).astype(f32)) for _ in range(3)]
    got = tc.pd_torques(torch.from_numpy(q), torch.from_numpy(qd), torch.from_numpy(tg), p, d, c).numpy()
    want = np.clip(p.numpy() * (tg - q) - d.numpy() * qd, -c.numpy(), c.numpy())
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7)
    try:
        tc.inverse_dynamics(tc.DofDynamics(None, torch.zeros(N, ND), None), torch.zeros(N, ND))
    except ValueError as err:
        assert "mass" in str(err)
    else:
        raise AssertionError("inverse_dynamics without a mass matrix")


# ------------------------------------------------------------------------------------------------------------------ 8. one-shot, independence
def case_independence(backend):
    """the pending DOF forces have a slot of their own: the force-perturbation sampler (which replaces the wrench at every step) and
    sdx_apply_rigid_body_forces leave them alone, a snapshot save / restore between the call and the launch does not touch them, and
    the step after the launch is a step without them"""
    make, dev = backend
    rng = np.random.default_rng(81)
    desc, effort, q = _start_state(backend, rng)
    u_host = _torques(desc, q, rng)

    def run(sampler, wrench, snap, apply=True, steps=2):
        s = make(N, seed=SEED)
        try:
            s.RESET.zero_()
            _place(s, dev, q)
            s.PREV_TARGETS.copy_(s.TARGETS)
            keep = []
            if sampler:
                keep = [dev(torch.zeros(N, NB, 3)), dev(torch.zeros(N))]
                s.set_force_perturbation(_abi.ForcePerturbAttr(2.0, 1.0, 1.0, 0.99, 0.08), keep[0], keep[1])
            out = []
            for i in range(steps):
                if apply and i == 0:
                    s.apply_dof_forces(dev(torch.from_numpy(u_host)), ARM)
                    if wrench:
                        s.apply_rigid_body_forces(dev(torch.zeros(N, NB, 3)), None, "env")
                        s.apply_rigid_body_forces()
                    if snap:
                        st = s.snapshot()
                        st.save()
                        st.restore()
                        st.close()
                s.step(dev(torch.zeros(N, ND)))
                out.append(_dofs(s))
            if sampler:
                assert (host(keep[0]) != 0).any(), "the sampler never pushed"
            return out
        finally:
            s.close()

    plain = run(False, False, False)
    never = run(False, False, False, apply=False)
    assert np.abs(plain[0][..., 1] - never[0][..., 1]).max() > 0.5               # the torques act
    for name, got in (("sampler on", run(True, False, False)), ("wrench calls", run(False, True, False)), ("snapshot", run(False, False, True))):
        for i in range(2):
            np.testing.assert_array_equal(got[i].view(np.uint32), plain[i].view(np.uint32), err_msg="%s, step %d" % (name, i))
    # consumed: the second step of `plain` is a step without DOF forces from the first step's result
    s = make(N, seed=SEED)
    try:
        s.RESET.zero_()
        _place(s, dev, q)
        s.PREV_TARGETS.copy_(s.TARGETS)
        s.apply_dof_forces(dev(torch.from_numpy(u_host)), ARM)
        s.apply_dof_forces()                                                       # cleared before the launch: nothing acts
        s.step(dev(torch.zeros(N, ND)))
        np.testing.assert_array_equal(_dofs(s).view(np.uint32), never[0].view(np.uint32))
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 9. N against 2 N (GPU)
def case_n_against_2n(backend, randomize):
    make, dev = backend
    rng = np.random.default_rng(91)
    outs = []
    for n in (N, 2 * N):
        s = make(n, seed=SEED)
        try:
            r = np.random.default_rng(92)
            q = _draw_q(s, r, n=2 * N)[:n]
            qd = r.uniform(-1, 1, (2 * N, ND)).astype(f32)[:n]
            tg = (q + r.uniform(-0.05, 0.05, (2 * N, ND)).astype(f32)[:n]).astype(f32)
            if randomize:
                _dr_on(s, dev, link_factor=np.linspace(0.8, 1.3, NL, dtype=f32), gain_scale=(1.1, 0.9))
            _place(s, dev, q, qd, tg)
            outs.append(_dyn(s))
        finally:
            s.close()
    for name, a, b in zip(("mass", "bias", "drive"), *outs):
        np.testing.assert_array_equal(a.view(np.uint32), b[:N].view(np.uint32), err_msg=name)
        assert np.abs(a).max() > 0
