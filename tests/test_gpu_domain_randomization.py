"""GPU: domain randomization on the MI355X: the randomization variant of k_physics with the scene's rows is
bit-identical to the default kernel, per-env rows act as per-env scene constants (C oracle), free fall follows the sampled gravity, the
sampler's statistics and its independence of N, and the task classes / train_rlgames --randomize end to end."""
import os

import numpy as np
import pytest
import yaml

torch = pytest.importorskip("torch")

from seqdex_amd import domain_randomization as dr   # noqa: E402
from test_domain_randomization import _state, shipped   # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sim(n, **kw):
    from seqdex_amd.sim import SdxSim
    return SdxSim(n, device="cuda:0", seed=22, **kw)


def _load(s, root, dof, tg):
    s.ROOT.copy_(torch.as_tensor(root.reshape(s.ROOT.shape)).cuda())
    s.DOF.copy_(torch.as_tensor(dof.reshape(s.DOF.shape)).cuda())
    s.TARGETS.copy_(torch.as_tensor(tg).cuda())
    s.WARM_COUNT.zero_()
    s.refresh_kinematics()


def test_identity_rows_bit_identical_n1024():
    n = 1024
    a, b = _sim(n), _sim(n)
    b.set_randomization(dr.identity_desc())
    g = torch.Generator().manual_seed(3)
    for _ in range(20):
        act = (torch.rand(n, 23, generator=g) * 2 - 1).cuda()
        a.step(act)
        b.step(act)
    torch.cuda.synchronize()
    for name in ("ROOT", "DOF", "OBS", "REW", "RB", "CONTACT"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert int(b.DR_FRAME[0]) == 20 and int(a.DR_FRAME[0]) == 0      # one GraspSim step = one physics launch
    a.close()
    b.close()


def test_per_env_rows_match_oracle_n8():
    """8 envs with 8 distinct parameter rows in one launch = the C oracle run per env with those values as scene constants"""
    from oracle import physics_oracle as po
    from seqdex_amd.scene import load_scene
    scene = load_scene()
    n = 8
    root, dof, tg = _state(scene, n)
    s = _sim(n, warm_start=0.0)
    _load(s, root, dof, tg)
    s.set_randomization(dr.identity_desc())
    base = s._desc
    rng = np.random.default_rng(5)
    fb, kpf, kdf = rng.uniform(0.3, 1.5, n), rng.uniform(0.6, 1.4, n), rng.uniform(0.5, 2.0, n)
    up, lmf, bmf = rng.uniform(-0.06, 0.0, n), rng.uniform(0.6, 1.4, n), rng.uniform(0.5, 1.5, n)
    grav = [0.1, -0.2, -8.5]
    dof_rows = np.zeros((n, 4, 23), np.float32)
    descs = []
    for e in range(n):
        dof_rows[e, 0] = np.float32(base.kp) * f32(kpf[e])
        dof_rows[e, 1] = np.float32(base.kd) * f32(kdf[e])
        dof_rows[e, 2] = np.float32(base.lower)
        dof_rows[e, 3] = np.float32(base.upper) + f32(up[e])
        d = type(base).from_buffer_copy(base)
        d.friction = f32(0.5) * (f32(base.friction) * f32(fb[e]) + f32(base.friction))
        d.kp[:], d.kd[:], d.upper[:] = dof_rows[e, 0].tolist(), dof_rows[e, 1].tolist(), dof_rows[e, 3].tolist()
        for k in range(24):
            d.link_mass[k] = np.float32(base.link_mass[k]) * f32(lmf[e])
            d.link_inertia[k][:] = (np.float32(list(base.link_inertia[k])) * f32(lmf[e])).tolist()
        for t in range(8):
            d.brick_mass[t] = np.float32(base.brick_mass[t]) * f32(bmf[e])
            d.brick_inertia[t][:] = (np.float32(list(base.brick_inertia[t])) * f32(bmf[e])).tolist()
        d.gravity[:] = grav
        descs.append(d)
    s.DR_DOF.copy_(torch.as_tensor(dof_rows).cuda())
    s.DR_LINK[:, 0] = torch.as_tensor(lmf, dtype=torch.float32)[:, None].cuda()
    s.DR_BRICK[:, 0] = torch.as_tensor(bmf, dtype=torch.float32)[:, None].cuda()
    s.DR_BRICK[:, 1] = (torch.as_tensor(np.float32(base.friction) * fb.astype(np.float32)))[:, None].cuda()
    s.DR_GRAVITY.copy_(torch.tensor(grav).cuda())
    o = [(root[e:e + 1].copy(), dof[e:e + 1].copy()) for e in range(n)]
    v1 = None
    for it in range(8):
        s.simulate()
        torch.cuda.synchronize()
        g_root = s.ROOT.cpu().numpy().reshape(n, 142, 13)
        g_dof = s.DOF.cpu().numpy().reshape(n, 23, 2)
        for e in range(n):
            po.simulate(descs[e], o[e][0], o[e][1], tg[e:e + 1])
            np.testing.assert_allclose(g_root[e, 9, 7:10], o[e][0][0, 9, 7:10], atol=2e-5)
            np.testing.assert_allclose(g_root[e, 10:13, 0:3], o[e][0][0, 10:13, 0:3], atol=2e-5)
            np.testing.assert_allclose(g_dof[e, :, 0], o[e][1][0, :, 0], atol=1e-5)
            np.testing.assert_allclose(g_dof[e, :, 1], o[e][1][0, :, 1], atol=5e-5)
        if it == 0:
            v1 = g_root[:, 9, 7].copy()
    # sliding: the first step's deceleration orders the envs by their averaged friction
    assert np.all(np.diff(v1[np.argsort(fb)]) < 0)
    for _ in range(30):
        s.simulate()
    g_dof = s.DOF.cpu().numpy().reshape(n, 23, 2)
    np.testing.assert_array_equal(g_dof[:, 8, 0], dof_rows[:, 3, 8])          # each stops at its own upper limit
    s.close()


def test_free_fall_follows_sampled_gravity():
    from seqdex_amd.scene import load_scene
    from test_physics_oracle import base_state
    scene = load_scene()
    root, dof, tg = base_state(scene, 2)
    s = _sim(2)
    _load(s, root, dof, tg)
    p = {"frequency": 1, "sim_params": {"gravity": {"range": [0.0, 1.0], "operation": "additive", "distribution": "gaussian"}}}
    s.set_randomization(p)
    g = s.DR_GRAVITY.cpu().numpy()
    assert np.all(g != np.float32(s._desc.gravity))
    z0 = root[:, 9, 2].copy()
    for k in range(1, 4):
        s.simulate()
        r = s.ROOT.cpu().numpy().reshape(2, 142, 13)
        h, m = np.float32(s._desc.dt) / s._desc.substeps, s._desc.substeps * k
        np.testing.assert_allclose(r[:, 9, 7:10], np.tile(m * h * g, (2, 1)), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(r[:, 9, 2] - z0, h * h * g[2] * m * (m + 1) / 2, rtol=2e-4)
    s.close()


def test_sampler_statistics_n4096():
    n = 4096
    p = shipped("grasp_sim")["task"]["randomization_params"]
    s = _sim(n)
    s.DR_FRAME[0] = 50000                      # past every schedule_steps: s = 1
    s.set_randomization(p)
    d = s._desc
    kp = s.DR_DOF[:, 0].cpu().numpy() / np.float32(d.kp)
    lo = s.DR_DOF[:, 2].cpu().numpy() - np.float32(d.lower)
    lm = s.DR_LINK[:, 0].cpu().numpy()
    lf = s.DR_LINK[:, 1].cpu().numpy()
    bm = s.DR_BRICK[:, 0].cpu().numpy()
    bf = s.DR_BRICK[:, 1].cpu().numpy()
    # loguniform [0.75, 1.5]: log factor uniform on [log .75, log 1.5] (KS distance)
    x = np.sort(np.log(kp.ravel().astype(np.float64)))
    a0, a1 = np.log(0.75), np.log(1.5)
    assert x.min() >= a0 - 1e-6 and x.max() <= a1 + 1e-6
    assert np.abs(np.arange(1, x.size + 1) / x.size - (x - a0) / (a1 - a0)).max() < 0.01
    # gaussian additive [0, 0.01]: mean 0, standard deviation 0.01
    assert abs(lo.mean()) < 4 * 0.01 / np.sqrt(lo.size) and abs(lo.std() / 0.01 - 1) < 0.01
    # uniform [0.5, 1.5]
    for u in (lm, bm):
        assert u.min() >= 0.5 and u.max() <= 1.5 and abs(u.mean() - 1.0) < 4 * (1 / np.sqrt(12)) / np.sqrt(u.size)
    # friction on the 250-bucket grid of [0.7, 1.3] x scene friction, every bucket hit
    grid = np.array([f32(0.7) + (f32(1.3) - f32(0.7)) * f32(k) / f32(250) for k in range(250)], np.float32) * np.float32(d.friction)
    for f in (lf, bf):
        assert np.isin(f, grid).all() and np.unique(f).size == 250
    # the same seed gives the same samples; env e's samples do not depend on N
    t = _sim(256)
    t.DR_FRAME[0] = 50000
    t.set_randomization(p)
    for name in ("DR_DOF", "DR_LINK", "DR_BRICK", "DR_GRAVITY"):
        ref = getattr(s, name).cpu()
        assert torch.equal(getattr(t, name).cpu(), ref[:256] if ref.dim() > 1 else ref), name
    t.close()
    s.close()


@pytest.mark.parametrize("task", ["BlockAssemblyGraspSim", "BlockAssemblyInsertSim", "BlockAssemblyOrient", "BlockAssemblySearch"])
def test_train_rlgames_randomize(task, tmp_path):
    """train_rlgames --randomize for two epochs: the tasks randomize at create (frame 0: the scene's values under the linear schedule) and
    re-sample the envs that reset once frame > 0 (frequency lowered to 1 and episodes to 4 steps so that this happens within the run)"""
    from seqdex_amd.config import get_args
    from seqdex_amd.train_rlgames import build
    name = {"BlockAssemblyGraspSim": "grasp_sim", "BlockAssemblyInsertSim": "insert_sim", "BlockAssemblyOrient": "orient",
            "BlockAssemblySearch": "search"}[task]
    cfg = shipped(name)
    cfg["task"]["randomization_params"]["frequency"] = 1
    cfg_env = tmp_path / "env.yaml"
    cfg_env.write_text(yaml.safe_dump(cfg))
    args = get_args(["--task=%s" % task, "--num_envs=64", "--max_iterations", "2", "--headless", "--randomize", "--episode_length", "4",
                     "--cfg_env", str(cfg_env), "--logdir", str(tmp_path)])
    t, env, agent, logdir, rank = build(args, minibatch_size=64)   # (InsertSim ships minibatch 4096 > 64 envs x horizon 8)
    s = t.sim
    assert t.randomize and t.randomization_report["randomized"]
    kp0 = np.float32(s._desc.kp)
    assert np.all(s.DR_DOF[:, 0].cpu().numpy() == kp0)            # frame 0
    agent.train()
    torch.cuda.synchronize()
    assert int(s.DR_FRAME[0]) > 0
    assert (s.DR_DOF[:, 0].cpu().numpy() != kp0).any()
    assert (s.DR_GRAVITY.cpu().numpy() != np.float32(s._desc.gravity)).any()
    assert np.isfinite(s.OBS.cpu().numpy()).all()
    s.close()


def test_brick_mass_factor_reaches_contact_impulses():
    """known answer for the brick mass factor: two free bricks collide in zero gravity (SDX_T_DR_GRAVITY = 0); the contact impulses are
    equal and opposite, so the momentum computed with each env's own brick masses (factor x scene mass) is conserved, and the struck brick
    leaves faster the heavier the striker is.  (The engine's net contact force tensor holds the hand links only - what the tasks read,
    GS:1159-1162 - so a resting brick's contact force is not observable through it.)"""
    from seqdex_amd.scene import load_scene
    from test_physics_oracle import base_state
    scene = load_scene()
    n = 4
    root, dof, tg = base_state(scene, n)
    floor_top = scene.statics[6]["center"][2] + scene.statics[6]["half"][2]
    root[:, 9, 0:3] = [0.25, 0.19, floor_top + 0.1]   # inside the bin, clear of floor and hand: brick 0 flies at brick 1, 0.1 m along x
    root[:, 10, 0:3] = [0.35, 0.19, floor_top + 0.1]
    root[:, 9, 7] = 1.0
    s = _sim(n, warm_start=0.0)
    _load(s, root, dof, tg)
    s.set_randomization(dr.identity_desc())
    fa = torch.tensor([0.5, 1.0, 1.5, 2.0])    # striker's mass factor per env; the struck brick keeps factor 1
    s.DR_BRICK[:, 0, 0] = fa.cuda()
    s.DR_GRAVITY.zero_()
    d = s._desc
    ma = np.float32(d.brick_mass[d.brick_type[0]]) * fa.numpy()
    mb = np.float32(d.brick_mass[d.brick_type[1]])
    for _ in range(15):
        s.simulate()
    r = s.ROOT.cpu().numpy().reshape(n, 142, 13)
    va, vb = r[:, 9, 7:10], r[:, 10, 7:10]
    assert (vb[:, 0] > 0.05).all(), (va, vb)                            # the collision happened in every env
    p = ma[:, None] * va + mb * vb
    np.testing.assert_allclose(p, np.stack([ma * 1.0, 0 * ma, 0 * ma], 1), rtol=2e-3, atol=2e-3 * float(ma.max()))
    assert np.all(np.diff(vb[:, 0]) > 0)                                 # heavier striker, faster struck brick
    s.close()
