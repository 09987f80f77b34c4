"""Shared bodies of the external-wrench tests (include/seqdex.h sdx_apply_rigid_body_forces / sdx_set_force_perturbation, DESIGN.md section
21): tests/test_rigid_body_forces.py runs them on the emulated simulator (tests/hipemu), tests/test_gpu_rigid_body_forces.py on the GPU.
A `backend` is (make, dev): make(n, **desc) builds a simulator, dev(tensor) moves a host tensor to where its tensors live.  The C
oracle has no external forces: the expected values are closed forms, equivalences between two runs of the engine, and the numpy
restatement of the sampler in tests/helpers/force_perturb_restatement.py."""
import numpy as np
import torch

import state_snapshot_cases as SC
from helpers import force_perturb_restatement as fr
from seqdex_amd import _abi
from seqdex_amd import domain_randomization as dr
from seqdex_amd.sim import SdxError

f32 = np.float32
SEED = 22
NB, B0, A0, NF, NL, ND = _abi.BODIES, _abi.BODY_BRICK0, _abi.ACTOR_BRICK0, _abi.NFREE, _abi.NLINK, _abi.NDOF
NEVER = 10 ** 9


def host(t):
    return t.detach().cpu().numpy().copy()


def perturb_attr(scale=2.0, lo=0.001, hi=0.1, decay=0.99, interval=0.08):
    return _abi.ForcePerturbAttr(scale, lo, hi, decay, interval)


def target_brick(e):
    return int(fr.target_brick(e))


def brick_mass(s, e, i):
    """mass of free brick i of env e as the physics sees it, randomization off"""
    d = s._desc
    return float(d.brick_mass[d.brick_type[i]]) * (float(d.seg_mass_scale) if i == target_brick(e) else 1.0)


def quat_R(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def wrench_tensors(s, dev, rows):
    """[N, 165, 3] with rows {(env, body): vector}"""
    t = np.zeros((s.num_envs, NB, 3), f32)
    for (e, b), v in rows.items():
        t[e, b] = v
    return dev(torch.from_numpy(t))


# ------------------------------------------------------------------------------------------------------------------ 1. ABI
def case_abi_errors(backend):
    make, dev = backend
    s = make(2, seed=SEED)
    try:
        assert hasattr(s.lib, "sdx_apply_rigid_body_forces") and hasattr(s.lib, "sdx_set_force_perturbation")
        F = dev(torch.zeros(2, NB, 3))
        p = dev(torch.zeros(2))
        s.apply_rigid_body_forces(F, None, "env")
        s.apply_rigid_body_forces(None, F, "local")
        s.apply_rigid_body_forces()                                               # clears the pending wrench
        rc = s.lib.sdx_apply_rigid_body_forces(s.h, None, None, 2, None)
        assert rc == -1 and b"sdx_apply_rigid_body_forces: space" in s.lib.sdx_last_error(s.h)
        for bad in (dev(torch.zeros(2, NB, 4)), dev(torch.zeros(2, NB, 3, dtype=torch.float64)), dev(torch.zeros(2, NB, 6))[:, :, :3], [0.0]):
            try:
                s.apply_rigid_body_forces(bad)
            except ValueError as err:
                assert "forces" in str(err)
            else:
                raise AssertionError("a bad forces tensor was accepted")
        try:
            s.apply_rigid_body_forces(F, space="world")
        except ValueError as err:
            assert "space" in str(err)
        else:
            raise AssertionError("a bad space was accepted")
        nan, inf = float("nan"), float("inf")
        for kw, word in ((dict(scale=nan), "finite"), (dict(scale=inf), "finite"), (dict(lo=nan), "finite"), (dict(decay=inf), "finite"),
                         (dict(interval=nan), "finite"), (dict(lo=0.0), "0 < lo <= hi <= 1"), (dict(lo=0.2, hi=0.1), "0 < lo <= hi <= 1"),
                         (dict(hi=1.5), "0 < lo <= hi <= 1"), (dict(decay=0.0), r"decay must lie in \(0, 1\]"), (dict(decay=1.01), "decay must lie"),
                         (dict(interval=0.0), "decay_interval must be > 0"), (dict(interval=-1.0), "decay_interval")):
            try:
                s.set_force_perturbation(perturb_attr(**kw), F, p)
            except SdxError as err:
                import re
                assert re.search(r"error -1: sdx_set_force_perturbation: .*%s" % word, str(err)), (kw, str(err))
            else:
                raise AssertionError("accepted %r" % (kw,))
        try:
            s.set_force_perturbation(perturb_attr(), None, None)
        except SdxError as err:
            assert "error -1" in str(err) and "NULL" in str(err)
        else:
            raise AssertionError("NULL buffers accepted")
        s.set_force_perturbation(perturb_attr(scale=0.0), F, p)                   # off, whatever else it says
        s.set_force_perturbation(None)
        assert _abi.SDX_ABI_VERSION == 8 and len(_abi.T) == 56
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 2. off and zero
def case_off_and_zero(backend, golden_dir, n, randomize):
    """three steps from the contact-rich P1 state, warm start on: no call == an all-zero wrench every step (the FORCE instantiation) ==,
    from step 2 on, a run that had a one-shot wrench at step 1 against a run whose step-1 result was copied in"""
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
        z = np.zeros((n, NB, 3), f32)
        z[:, ::2] = -0.0                                                          # negative zeros are zeros too
        zf, zt = dev(torch.from_numpy(z)), dev(torch.zeros(n, NB, 3))
        got = []
        for i, act in enumerate(acts):
            if i == 0:
                b.apply_rigid_body_forces(zf, None, "env")
            elif i == 1:
                b.apply_rigid_body_forces(None, zf, "local")
            else:
                b.apply_rigid_body_forces(zf, zt, "local")
            b.step(dev(act))
            got.append(SC.record(b))
        for i in range(3):
            SC.assert_records_equal(b, base[i], got[i], "zero wrench, step %d" % i)
    finally:
        b.close()
    c, d = start(), start()
    try:
        rows = {(e, B0 + i): (0.3, -0.2, 0.5) for e in range(n) for i in range(0, NF, 5)}
        rows.update({(e, 3): (1.0, 2.0, -1.0) for e in range(n)})
        c.apply_rigid_body_forces(wrench_tensors(c, dev, rows), None, "env")
        c.step(dev(acts[0]))
        first = SC.record(c)
        differs = (first["ROOT"] != base[0]["ROOT"]).any() and (first["DOF"] != base[0]["DOF"]).any()
        assert differs, "the one-shot wrench moved nothing"
        st = c.snapshot()
        st.save()
        st.restore(sim=d)                                                         # the step-1 result, copied into a simulator that never saw a wrench
        for i in (1, 2):
            c.step(dev(acts[i]))
            d.step(dev(acts[i]))
            SC.assert_records_equal(c, SC.record(d), SC.record(c), "after the one-shot wrench, step %d" % i)
        st.close()
    finally:
        c.close()
        d.close()


# ------------------------------------------------------------------------------------------------------------------ 3. free flight
TILT = np.array([np.sin(0.2) * np.cos(0.35), np.sin(0.2) * np.sin(0.35), np.cos(0.2) * np.sin(0.35), np.cos(0.2) * np.cos(0.35)])   # tilt 0.4 about x, then yaw 0.7
LIFTED = (0, 1, 2, 5, 6, 9)       # free bricks lifted clear of everything (0, 1, 2: the target bricks of envs 0, 1, 2)
FIXED = NF + 3                    # a fixed brick


def _parked_pose(s):
    sc = s.scene
    return np.concatenate([np.array(sc.arm_prepare_pose, f32), 0.5 * (np.array(sc.finger_reset_unscaled, f32) + 1) * (sc.upper[7:] - sc.lower[7:])
                           + sc.lower[7:]]).astype(f32)


def _free_flight_sim(backend, n):
    make, dev = backend
    s = make(n, seed=SEED, seg_mass_scale=2.5)
    pose = _parked_pose(s)
    dof = np.zeros((n, ND, 2), f32)
    dof[:, :, 0] = pose
    s.DOF.copy_(dev(torch.from_numpy(dof.reshape(-1, 2))))
    s.TARGETS.copy_(dev(torch.from_numpy(np.tile(pose, (n, 1)))))
    root = host(s.ROOT).reshape(n, _abi.ACTORS, 13)
    q = (TILT / np.linalg.norm(TILT)).astype(f32)
    for k, i in enumerate(LIFTED):
        root[:, A0 + i, 0:3] = (2.0 + 0.5 * k, 1.5, 3.0)
        root[:, A0 + i, 3:7] = q
        root[:, A0 + i, 7:13] = 0
    return s, root, q


def _fly(s, dev, root, forces, torques, space):
    n = s.num_envs
    s.ROOT.copy_(dev(torch.from_numpy(root.reshape(-1, 13))))
    s.WARM_COUNT.zero_()
    s.apply_rigid_body_forces(forces, torques, space)
    s.simulate()
    return host(s.ROOT).reshape(n, _abi.ACTORS, 13)


def case_free_flight(backend, n=3):
    """bricks lifted clear of everything, one step: dv = (g + F / m) h substeps (velocity rtol 1e-5, position rtol 1e-4 atol 1e-6: the bars of
    test_free_fall_and_invariants), F = -m g leaves the velocity unchanged, dw = R diag(1 / I) R^T tau h substeps, ENV against LOCAL on a
    yawed and tilted brick, NULL forces with torques and the reverse, the target brick with seg_mass_scale = 2.5, a fixed brick's row ignored"""
    make, dev = backend
    s, root, q = _free_flight_sim(backend, n)
    try:
        d = s._desc
        nsub, h = int(d.substeps), float(d.dt) / int(d.substeps)
        g = np.array([float(v) for v in d.gravity])
        R = quat_R(q.astype(np.float64) / np.linalg.norm(q.astype(np.float64)))
        steps_sum = nsub * (nsub + 1) // 2
        assert float(d.seg_mass_scale) == 2.5
        # ---- forces in the env frame, torques NULL.  Brick 6 carries -m g, the fixed brick a large force
        frc = {}
        for e in range(n):
            for i in LIFTED:
                m = brick_mass(s, e, i)
                frc[(e, B0 + i)] = -m * g if i == 6 else np.array([0.7 + 0.1 * i, -1.1, 20.0 + e]) * m
            frc[(e, B0 + FIXED)] = (50.0, 50.0, 50.0)
            frc[(e, 24)] = (9.0, 9.0, 9.0)                                       # the object actor's body: cannot move
        F = wrench_tensors(s, dev, frc)
        r1 = _fly(s, dev, root, F, None, "env")
        for e in range(n):
            for i in LIFTED:
                a = g + np.asarray(frc[(e, B0 + i)], np.float64) / brick_mass(s, e, i)
                v, dp = r1[e, A0 + i, 7:10], r1[e, A0 + i, 0:3] - root[e, A0 + i, 0:3]
                if i == 6:
                    np.testing.assert_allclose(v, 0.0, atol=1e-5 * np.abs(g).max() * h * nsub, err_msg="F = -m g")
                else:
                    np.testing.assert_allclose(v, a * h * nsub, rtol=1e-5, err_msg="velocity env %d brick %d" % (e, i))
                    np.testing.assert_allclose(dp, a * h * h * steps_sum, rtol=1e-4, atol=1e-6, err_msg="position env %d brick %d" % (e, i))
                np.testing.assert_array_equal(r1[e, A0 + i, 10:13], 0.0)         # no torque: no spin, the orientation stays
                np.testing.assert_array_equal(r1[e, A0 + i, 3:7], q)
        np.testing.assert_array_equal(r1[:, A0 + FIXED], root[:, A0 + FIXED])   # the fixed brick's row is ignored
        np.testing.assert_array_equal(r1[:, 1], root[:, 1])                      # ... and the object actor's
        # the target brick really is 2.5 times as heavy: same force per scene mass on bricks 1 (target of env 1) gives 1 / 2.5 of the push
        assert abs(brick_mass(s, 1, 1) / brick_mass(s, 0, 1) - 2.5) < 1e-6
        # ---- torques in the env frame, forces NULL: a brick at rest.  Small enough that the brick turns by < 1e-4 rad between the substeps
        # (the closed form holds R fixed): rtol 2e-4 of the largest component
        trq = {}
        for e in range(n):
            for i in LIFTED:
                I = np.array([float(v) for v in d.brick_inertia[d.brick_type[i]]]) * (brick_mass(s, e, i) / float(d.brick_mass[d.brick_type[i]]))
                trq[(e, B0 + i)] = np.array([0.8, -0.5, 1.0]) * I.min() * 2.0    # ~ 0.02 rad/s after the step
        T = wrench_tensors(s, dev, trq)
        r2 = _fly(s, dev, root, None, T, "env")

        def dw_expected(e, i, tau_world):
            I = np.array([float(v) for v in d.brick_inertia[d.brick_type[i]]]) * (brick_mass(s, e, i) / float(d.brick_mass[d.brick_type[i]]))
            return R @ ((R.T @ tau_world) / I) * h * nsub

        for e in range(n):
            for i in LIFTED:
                want = dw_expected(e, i, np.asarray(trq[(e, B0 + i)], np.float64))
                assert 0.005 < np.abs(want).max() < 0.1
                np.testing.assert_allclose(r2[e, A0 + i, 10:13], want, rtol=0, atol=2e-4 * np.abs(want).max(), err_msg="spin env %d brick %d" % (e, i))
                np.testing.assert_allclose(r2[e, A0 + i, 7:10], g * h * nsub, rtol=1e-5, atol=1e-9)     # gravity only
        # ---- LOCAL: the same rows read in the body's axes = the rotated rows in the env's axes
        loc_f = {k: v for k, v in frc.items() if k[1] != B0 + 6}
        r3 = _fly(s, dev, root, wrench_tensors(s, dev, loc_f), T, "local")
        rot_f = {k: R @ np.asarray(v, np.float64) for k, v in loc_f.items()}
        rot_t = {k: R @ np.asarray(v, np.float64) for k, v in trq.items()}
        r4 = _fly(s, dev, root, wrench_tensors(s, dev, rot_f), wrench_tensors(s, dev, rot_t), "env")
        for e in range(n):
            for i in LIFTED:
                if i == 6:
                    continue
                a = g + rot_f[(e, B0 + i)] / brick_mass(s, e, i)
                np.testing.assert_allclose(r3[e, A0 + i, 7:10], a * h * nsub, rtol=1e-5, atol=1e-7, err_msg="LOCAL velocity env %d brick %d" % (e, i))
                want = dw_expected(e, i, rot_t[(e, B0 + i)])
                np.testing.assert_allclose(r3[e, A0 + i, 10:13], want, rtol=0, atol=2e-4 * np.abs(want).max(), err_msg="LOCAL spin")
                np.testing.assert_allclose(r3[e, A0 + i, 7:13], r4[e, A0 + i, 7:13], rtol=1e-5, atol=1e-7)
                assert np.abs(r3[e, A0 + i, 7:10] - r1[e, A0 + i, 7:10]).max() > 1e-3      # ... and not the unrotated ones
        # ---- forgotten: the next launch is plain free fall again
        r5 = host(s.ROOT).reshape(n, _abi.ACTORS, 13)
        s.simulate()
        r6 = host(s.ROOT).reshape(n, _abi.ACTORS, 13)
        for i in LIFTED:
            np.testing.assert_allclose(r6[:, A0 + i, 7:10] - r5[:, A0 + i, 7:10], np.tile(g * h * nsub, (n, 1)), rtol=1e-4, atol=1e-6)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 4. gravity equivalence
DG = np.array([3.5, -4.0, 4.5])          # all three components non-zero; 50 x the bars on a free brick after two steps needs >= 3 m/s^2
LIFT = (4, 17, 33, 50)


def case_gravity_equivalence(backend, golden_dir, n):
    """A: randomization on (identity rows), SDX_T_DR_GRAVITY = g + dg.  B: gravity g, F = m_b dg on every free brick.  Two steps from the P1
    state with a few bricks lifted.  Brick poses and velocities agree within the brick bars of test_one_step_teacher_forcing (>= 99 % within
    2e-5 m, at most 2 beyond 1e-4, none beyond 1e-3; velocities 2e-3 for >= 98 %); a run with neither differs from B by >= 50 x those bars
    on the lifted bricks."""
    make, dev = backend

    def start():
        s = SC.make_scene_sim(backend, golden_dir, n, steps=0)
        root = host(s.ROOT).reshape(n, _abi.ACTORS, 13)
        for i in LIFT:
            root[:, A0 + i, 2] += 1.0
            root[:, A0 + i, 7:13] = 0
        s.ROOT.copy_(dev(torch.from_numpy(root.reshape(-1, 13))))
        return s

    def bricks(s):
        return host(s.ROOT).reshape(n, _abi.ACTORS, 13)[:, A0:A0 + NF]

    out = {}
    for run in "ABC":
        s = start()
        try:
            g = np.array([float(v) for v in s._desc.gravity])
            if run == "A":
                s.set_randomization(dr.identity_desc(NEVER))
                s.DR_GRAVITY.copy_(dev(torch.from_numpy((g + DG).astype(f32))))
            F = wrench_tensors(s, dev, {(e, B0 + i): brick_mass(s, e, i) * DG for e in range(n) for i in range(NF)})
            for _ in range(2):
                if run == "B":
                    s.apply_rigid_body_forces(F, None, "env")
                s.simulate()
            out[run] = bricks(s)
            assert int(host(s.NCONTACTS).min()) > 100                           # contact-rich
        finally:
            s.close()
    a, b, c = out["A"], out["B"], out["C"]
    dp = np.abs(a[..., 0:7] - b[..., 0:7]).max(-1)
    dv = np.abs(a[..., 7:13] - b[..., 7:13]).max(-1)
    print("gravity equivalence: pose max %.3g, within 2e-5: %.4f, beyond 1e-4: %d; velocity within 2e-3: %.4f, max %.3g" % (
        dp.max(), (dp < 2e-5).mean(), int((dp >= 1e-4).sum()), (dv < 2e-3).mean(), dv.max()))
    assert (dp >= 1e-4).sum() <= 2 and dp.max() < 1e-3 and (dp < 2e-5).mean() >= 0.99
    assert (dv < 2e-3).mean() >= 0.98
    lifted = list(LIFT)
    assert np.abs(c[:, lifted, 0:3] - b[:, lifted, 0:3]).max(-1).min() >= 50 * 2e-5
    assert np.abs(c[:, lifted, 7:10] - b[:, lifted, 7:10]).max(-1).min() >= 50 * 2e-3


# ------------------------------------------------------------------------------------------------------------------ 5. robot links
ARM_LINK = 5


def case_robot_links(backend, space, link_mass_factor=None):
    """substeps = 1, the robot at rest on its targets, nothing near it.  Env 0: a wrench on an arm link, env 1: on a fingertip link, env 2:
    on both.  tau = J^T w in float64 from SDX_T_JACOBIAN, whose linear rows are the velocity of the link's FRAME ORIGIN (include/seqdex.h:
    `[N, 23, 6, 23]` for links 1..23, the rows of k_kinematics: a_j x (o_k - o_j)), so the force at the centre of mass
    goes there with the couple (c_k - o_k) x F.  Run X: targets shifted by tau_j / kp_j, no wrench; run Y: the wrench.  The joint
    velocities agree to rtol 1e-3, atol 2e-3 (the project's joint-velocity bar); the run with neither differs by >= 50 x that."""
    make, dev = backend
    n = 3

    def start():
        s = make(n, seed=SEED, substeps=1)
        pose = _parked_pose(s)
        pose[7:] = 0.5 * (s.scene.lower[7:] + s.scene.upper[7:])
        dof = np.zeros((n, ND, 2), f32)
        dof[:, :, 0] = pose
        s.DOF.copy_(dev(torch.from_numpy(dof.reshape(-1, 2))))
        s.TARGETS.copy_(dev(torch.from_numpy(np.tile(pose, (n, 1)))))
        root = host(s.ROOT).reshape(n, _abi.ACTORS, 13)
        root[:, A0:A0 + NF, 0] += 5.0                                            # the free bricks: far from the robot
        s.ROOT.copy_(dev(torch.from_numpy(root.reshape(-1, 13))))
        if link_mass_factor is not None:
            s.set_randomization(dr.identity_desc(NEVER))
            lk = host(s.DR_LINK)
            lk[:, 0, :] = link_mass_factor
            s.DR_LINK.copy_(dev(torch.from_numpy(lk)))
        s.refresh_kinematics()
        return s, pose

    def dofs(s):
        return host(s.DOF).reshape(n, ND, 2)

    s, pose = start()
    try:
        d = s._desc
        kp, effort = np.array([float(v) for v in d.kp]), np.array([float(v) for v in d.effort])
        J = host(s.JACOBIAN).astype(np.float64)                                   # [n, 23, 6, 23]: link k is row k - 1
        rb = host(s.RB).astype(np.float64)
        tip = int(d.fingertip_body[0])
        assert 7 < tip < NL
        # wrenches in the chosen space, sized (below) for |dqd| >= 0.1 rad/s with the drive far from its effort limit
        w_arm = (np.array([180.0, -120.0, 150.0]), np.array([24.0, 15.0, -18.0]))
        w_tip = (np.array([7.5, -6.0, 9.0]), np.array([0.3, -0.24, 0.36]))
        plan = {0: {ARM_LINK: w_arm}, 1: {tip: w_tip}, 2: {ARM_LINK: w_arm, tip: w_tip}}
        frc, trq, tau = {}, {}, np.zeros((n, ND))
        for e, links in plan.items():
            for k, (F, T) in links.items():
                frc[(e, k)], trq[(e, k)] = F, T
                R = quat_R(rb[e, k, 3:7]) if space == "local" else np.eye(3)
                Fw, Tw = R @ F, R @ T
                com = quat_R(rb[e, k, 3:7]) @ np.array([float(v) for v in d.link_com[k]])      # c_k - o_k
                w = np.concatenate([Fw, Tw + np.cross(com, Fw)])
                tau[e] += J[e, k - 1].T @ w
        shift = tau / kp
        print("robot links: |tau| / effort max per env", (np.abs(tau) / effort).max(-1))
        assert (np.abs(kp * shift) < 0.5 * effort).all(), "the effort limit must stay inactive"
        F, T = wrench_tensors(s, dev, frc), wrench_tensors(s, dev, trq)
        # run Y: the wrench
        s.apply_rigid_body_forces(F, T, space)
        s.simulate()
        y = dofs(s)
        assert (host(s.CONTACT).reshape(n, NB, 3)[:, :NL] == 0).all(), "something touches the robot"
    finally:
        s.close()
    x_sim, _ = start()
    try:
        x_sim.TARGETS.copy_(dev(torch.from_numpy((np.tile(pose, (n, 1)) + shift).astype(f32))))
        x_sim.simulate()
        x = dofs(x_sim)
        assert (host(x_sim.CONTACT).reshape(n, NB, 3)[:, :NL] == 0).all()
    finally:
        x_sim.close()
    o_sim, _ = start()
    try:
        o_sim.simulate()
        o = dofs(o_sim)
    finally:
        o_sim.close()
    err = np.abs(y[..., 1] - x[..., 1])
    print("robot links (%s, factor %s): |dqd| max %.3g, X - Y max %.3g" % (space, link_mass_factor, np.abs(y[..., 1]).max(), err.max()))
    np.testing.assert_allclose(y[..., 1], x[..., 1], rtol=1e-3, atol=2e-3)
    np.testing.assert_array_equal(o[..., 1], 0.0)                                  # at rest on its targets: nothing moves without the wrench
    for e in range(n):
        moved = np.abs(y[e, :, 1]) >= 0.1
        assert moved.any(), (e, y[e, :, 1])
        j = int(np.abs(y[e, :, 1]).argmax())                                       # the joint the wrench moves most
        assert abs(y[e, j, 1] - o[e, j, 1]) >= 50 * (2e-3 + 1e-3 * abs(y[e, j, 1])), (e, y[e, :, 1])
    return y


# ------------------------------------------------------------------------------------------------------------------ 6. the sampler
def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, f32))).astype(np.float64)


class Pushes:
    """a GraspSim simulator with the sampler on and the host's view of the two caller-owned tensors"""

    def __init__(self, backend, n, attr, randomize=False, **kw):
        self.make, self.dev = backend
        self.n, self.attr = n, attr
        self.s = self.make(n, seed=SEED, **kw)
        self.s.RESET.zero_()
        self.F = self.dev(torch.zeros(n, NB, 3))
        self.p = self.dev(torch.zeros(n))
        self.steps = 0
        d = self.s._desc
        self.mass = np.array([f32(d.brick_mass[d.brick_type[target_brick(e)]]) * f32(d.seg_mass_scale) for e in range(n)], f32)
        if randomize:
            self.s.set_randomization(dr.identity_desc(NEVER))
            bk = host(self.s.DR_BRICK)
            bk[:, 0, :] = np.linspace(0.7, 1.6, NF, dtype=f32)[None, :] + f32(0.01) * np.arange(n, dtype=f32)[:, None]
            self.s.DR_BRICK.copy_(self.dev(torch.from_numpy(bk)))
            self.mass = np.array([self.mass[e] * bk[e, 0, target_brick(e)] for e in range(n)], f32)
        self.s.set_force_perturbation(attr, self.F, self.p)

    def close(self):
        self.s.close()

    def call(self, reset=None):
        """one sdx_pre_physics + sdx_post_physics (the step counter moves) checked against the restatement; returns (pushed, z)"""
        n, s = self.n, self.s
        reset = np.zeros(n, bool) if reset is None else np.asarray(reset, bool)
        F0, p0 = host(self.F), host(self.p)
        s.RESET.copy_(self.dev(torch.from_numpy(reset.astype(np.int64))))
        s.pre_physics(self.dev(torch.zeros(n, ND)))
        F1, p1 = host(self.F), host(self.p)
        wF, wp, pushed, z = fr.step(self.attr, SEED, self.steps, F0, p0, reset, self.mass, float(s._desc.dt))
        # probabilities: 2 ulp where drawn, untouched elsewhere
        assert (np.abs(p1.astype(np.float64) - wp) <= 2 * _ulp(wp))[reset].all(), (p1, wp)
        np.testing.assert_array_equal(p1[~reset], p0[~reset])
        # the push decision: exact.  (An env whose drawn probability lies within 2 ulp of u' could go either way: none does in these runs)
        body = B0 + fr.target_brick(np.arange(n))
        decayed = wF.copy()
        for e in np.nonzero(pushed)[0]:
            decayed[e, body[e]] = np.nan
        mask = ~np.isnan(decayed)
        np.testing.assert_array_equal(F1[mask].view(np.uint32), wF[mask].view(np.uint32), err_msg="reset, then decay by one rounded factor")
        for e in range(n):
            row, want = F1[e, body[e]].astype(np.float64), wF[e, body[e]].astype(np.float64)
            if pushed[e]:
                scale = float(self.mass[e]) * float(f32(self.attr.force_scale))
                tol = 2 * _ulp(z[e]) * scale + 2 * _ulp(want)                    # 2 ulp per gaussian draw, one rounding per product
                assert (np.abs(row - want) <= tol).all(), (e, row, want, tol)
                assert (row != 0).all()
        s.post_physics()
        self.steps += 1
        return pushed, z


def case_sampler(backend, n, randomize=False):
    attr = perturb_attr(scale=2.0, lo=0.2, hi=0.7, decay=0.93, interval=0.05)
    t = Pushes(backend, n, attr, randomize)
    try:
        s = t.s
        # the initial draw: every env, 2 ulp; the forces are left alone
        want = fr.prob_draw(attr, SEED, n, 0)
        got = host(t.p)
        assert (np.abs(got.astype(np.float64) - want) <= 2 * _ulp(want)).all() and (got >= f32(0.2)).all() and (got <= f32(0.7)).all()
        assert len(set(got.tolist())) == n
        np.testing.assert_array_equal(host(t.F), 0.0)
        # rows the caller writes on other bodies only decay
        extra = np.zeros((n, NB, 3), f32)
        extra[:, 4] = (1.5, -2.5, 0.125)
        extra[:, B0 + 40] = (0.3, 0.2, -0.7)
        extra[:, NB - 1] = (-3.0, 1.0, 2.0)
        t.F.copy_(t.dev(torch.from_numpy(extra)))
        total = np.zeros(n, int)
        resets = [None, None, np.arange(n) % 3 == 1, None, np.arange(n) % 3 == 0, None, None, None]
        for r in resets:
            pushed, _ = t.call(r)
            total += pushed
        assert total.sum() >= n and (total < len(resets)).any()                  # pushes happened, and not everywhere every time
        F = host(t.F)
        kept = np.arange(n) % 3 == 2                  # the envs no reset zeroed
        assert kept.any() and (F[kept, NB - 1] != 0).all() and (np.abs(F[kept, NB - 1]) < np.abs(extra[kept, NB - 1])).all()
        assert (F[~kept, NB - 1] == 0).all() and (F[~kept, 4] == 0).all()
        # sdx_reset_idx: rows of the masked envs <- 0, their probability redrawn, nobody else touched (no decay either)
        F0, p0 = host(t.F), host(t.p)
        m = np.zeros(n, np.uint8)
        m[[0, n - 1]] = 1
        s.reset_idx(t.dev(torch.from_numpy(m)))
        F1, p1 = host(t.F), host(t.p)
        mb = m.astype(bool)
        np.testing.assert_array_equal(F1[mb], 0.0)
        np.testing.assert_array_equal(F1[~mb].view(np.uint32), F0[~mb].view(np.uint32))
        np.testing.assert_array_equal(p1[~mb], p0[~mb])
        want = fr.prob_draw(attr, SEED, n, t.steps)
        assert (np.abs(p1.astype(np.float64) - want) <= 2 * _ulp(want))[mb].all()
    finally:
        t.close()


def _push_trace(t, calls, resets=()):
    out = []
    for i in range(calls):
        r = np.arange(t.n) % 4 == 2 if i in resets else None
        reset = np.zeros(t.n, np.int64) if r is None else r.astype(np.int64)
        t.s.RESET.copy_(t.dev(torch.from_numpy(reset)))
        t.s.pre_physics(t.dev(torch.zeros(t.n, ND)))
        t.s.post_physics()
        out.append((host(t.F), host(t.p)))
    return out


def case_sampler_independent_of_n(backend, n_small, n_large):
    attr = perturb_attr(scale=1.5, lo=0.3, hi=0.6, decay=0.9, interval=0.1)
    traces = []
    for n in (n_small, n_large):
        t = Pushes(backend, n, attr)
        try:
            traces.append(_push_trace(t, 4, resets=(2,)))
        finally:
            t.close()
    for (Fa, pa), (Fb, pb) in zip(*traces):
        np.testing.assert_array_equal(Fa.view(np.uint32), Fb[:n_small].view(np.uint32))
        np.testing.assert_array_equal(pa.view(np.uint32), pb[:n_small].view(np.uint32))
    assert (traces[0][-1][0] != 0).any()


def case_sampler_snapshot(backend, n):
    """save_all and copies of the two caller-owned tensors; steps; restore_all and the copies back: the pushes repeat bit for bit"""
    attr = perturb_attr(scale=2.0, lo=0.3, hi=0.6, decay=0.95, interval=0.08)
    t = Pushes(backend, n, attr)
    try:
        _push_trace(t, 2)
        st = t.s.snapshot()
        st.save()
        F0, p0 = t.F.clone(), t.p.clone()
        first = _push_trace(t, 4, resets=(1,))
        st.restore()
        t.F.copy_(F0)
        t.p.copy_(p0)
        second = _push_trace(t, 4, resets=(1,))
        for (Fa, pa), (Fb, pb) in zip(first, second):
            np.testing.assert_array_equal(Fa.view(np.uint32), Fb.view(np.uint32))
            np.testing.assert_array_equal(pa.view(np.uint32), pb.view(np.uint32))
        assert any((a[0] != b[0]).any() for a, b in zip(first[:-1], first[1:]))
        st.close()
    finally:
        t.close()


def case_step_applies_the_pushes(backend, n):
    """through sdx_step: a pushed target brick in free flight gains F / m h substeps beside gravity, and a caller's own wrench for that step is
    replaced by the task's tensor"""
    make, dev = backend
    attr = perturb_attr(scale=30.0, lo=1.0, hi=1.0, decay=1.0, interval=0.08)       # every env is pushed at every step
    t = Pushes(backend, n, attr, seg_mass_scale=2.5)
    try:
        s = t.s
        d = s._desc
        nsub, h = int(d.substeps), float(d.dt) / int(d.substeps)
        g = np.array([float(v) for v in d.gravity])
        pose = _parked_pose(s)
        dof = np.zeros((n, ND, 2), f32)
        dof[:, :, 0] = pose
        s.DOF.copy_(dev(torch.from_numpy(dof.reshape(-1, 2))))
        s.TARGETS.copy_(dev(torch.from_numpy(np.tile(pose, (n, 1)))))
        s.PREV_TARGETS.copy_(dev(torch.from_numpy(np.tile(pose, (n, 1)))))
        root = host(s.ROOT).reshape(n, _abi.ACTORS, 13)
        for e in range(n):
            root[e, A0 + target_brick(e), 0:3] = (2.0, 1.5, 3.0)
            root[e, A0 + target_brick(e), 7:13] = 0
        s.ROOT.copy_(dev(torch.from_numpy(root.reshape(-1, 13))))
        other = wrench_tensors(s, dev, {(e, B0 + target_brick(e)): (0.0, 0.0, 500.0) for e in range(n)})
        s.apply_rigid_body_forces(other, None, "env")                                # replaced by rb_forces in the step below
        s.step(dev(torch.zeros(n, ND)))
        F = host(t.F)
        r1 = host(s.ROOT).reshape(n, _abi.ACTORS, 13)
        for e in range(n):
            b = target_brick(e)
            assert (F[e, B0 + b] != 0).all() and (np.delete(F[e], B0 + b, axis=0) == 0).all()
            a = g + F[e, B0 + b].astype(np.float64) / float(t.mass[e])
            np.testing.assert_allclose(r1[e, A0 + b, 7:10], a * h * nsub, rtol=1e-5, atol=1e-6)
        # a reset through sdx_step: rows a caller added are zeroed in exactly the resetting env (decay 1: they stay elsewhere)
        t.F[:, 5] = 1.25
        flags = np.zeros(n, np.int64)
        flags[1] = 1
        s.RESET.copy_(dev(torch.from_numpy(flags)))
        s.step(dev(torch.zeros(n, ND)))
        F = host(t.F)
        assert (F[1, 5] == 0).all() and (F[[0, 2], 5] == f32(1.25)).all()
        assert all((F[e, B0 + target_brick(e)] != 0).all() for e in range(n))
    finally:
        t.close()
