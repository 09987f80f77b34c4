"""-m gpu: external forces and torques on rigid bodies and the random pushes on the target brick through the compiled
gfx950 kernels: k_physics<512 | SDX_PHYS_FORCE>, k_physics<512 | SDX_PHYS_DR | SDX_PHYS_FORCE> and k_force_perturb.  The bodies are
tests/rigid_body_force_cases.py, shared with the emulated run of tests/test_rigid_body_forces.py; N = 3 (odd, no multiple of 4: the
sampler's scalar tail) unless a case says otherwise, N = 64 (a multiple of 4: 16-byte accesses only) where noted.

- off and zero at N = 3 and N = 64; free flight; gravity equivalence; robot links against J^T w (ENV, LOCAL, a link mass factor);
- the sampler against the restatement at N = 3 and N = 64, independence of N, snapshots, through sdx_step;
- its statistics at N = 4 096;  train_rlgames --force_scale end to end."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import rigid_body_force_cases as K          # noqa: E402
from helpers import force_perturb_restatement as fr      # noqa: E402


def _make(n, **kw):
    from seqdex_amd.sim import SdxSim
    return SdxSim(n, device="cuda:0", **kw)


BACKEND = (_make, lambda t: t.cuda())


def test_argument_errors():
    K.case_abi_errors(BACKEND)


@pytest.mark.parametrize("n,randomize", [(3, False), (3, True), (64, False), (64, True)])
def test_off_and_zero_wrench_are_bit_identical(golden_dir, n, randomize):
    K.case_off_and_zero(BACKEND, golden_dir, n, randomize)


def test_free_flight_closed_forms():
    K.case_free_flight(BACKEND, 3)


def test_gravity_equivalence_on_piles(golden_dir):
    K.case_gravity_equivalence(BACKEND, golden_dir, 3)


@pytest.mark.parametrize("space,factor", [("env", None), ("local", None), ("env", 1.4), ("local", 0.7)])
def test_robot_links_against_the_jacobian(space, factor):
    K.case_robot_links(BACKEND, space, factor)


@pytest.mark.parametrize("n,randomize", [(3, False), (3, True), (64, False)])
def test_sampler_against_the_restatement(n, randomize):
    K.case_sampler(BACKEND, n, randomize)


def test_sampler_independence_of_n_and_snapshot():
    K.case_sampler_independent_of_n(BACKEND, 8, 16)
    K.case_sampler_snapshot(BACKEND, 3)


def test_step_applies_the_pushes_and_replaces_the_callers_wrench():
    K.case_step_applies_the_pushes(BACKEND, 3)


def test_sampler_statistics_n4096():
    """sdx_pre_physics only, 8 calls, prob_lo = prob_hi = 0.25, no decay: the share of pushed envs and the mean and standard deviation of every
    component of z within five standard errors (the bars of test_gpu_domain_randomization.py::test_sampler_statistics_n4096): se(share) =
    sqrt(p (1 - p) / n), se(mean) = 1 / sqrt(n_z), se(std) = sqrt(1 / (2 n_z)) for n_z standard normals"""
    n, calls, p = 4096, 8, 0.25
    attr = K.perturb_attr(scale=3.0, lo=p, hi=p, decay=1.0, interval=0.08)
    t = K.Pushes(BACKEND, n, attr)
    try:
        s = t.s
        body = torch.as_tensor(K.B0 + fr.target_brick(np.arange(n)), device="cuda:0")
        env = torch.arange(n, device="cuda:0")
        zero = torch.zeros(n, K.ND, device="cuda:0")
        assert (K.host(t.p) == np.float32(p)).all()
        prev = t.F[env, body].clone()
        pushed, zs = 0, []
        for _ in range(calls):
            s.pre_physics(zero)
            s.post_physics()                                                      # (moves the step counter: the next call draws anew)
            row = t.F[env, body].clone()
            new = (row != prev).any(-1)                                           # decay 1: only a push changes the row
            pushed += int(new.sum())
            zs.append((row[new].double() / (torch.as_tensor(t.mass, device="cuda:0")[new].double()[:, None] * 3.0)).cpu().numpy())
            prev = row
        total = n * calls
        share = pushed / total
        z = np.concatenate(zs)
        nz = z.shape[0]
        print("pushes: share %.4f (want %.2f, 5 se %.4f); z mean %s std %s (5 se %.4f / %.4f)" % (
            share, p, 5 * (p * (1 - p) / total) ** 0.5, z.mean(0), z.std(0), 5 / nz ** 0.5, 5 / (2 * nz) ** 0.5))
        assert abs(share - p) <= 5 * (p * (1 - p) / total) ** 0.5
        assert (np.abs(z.mean(0)) <= 5 / nz ** 0.5).all()
        assert (np.abs(z.std(0) - 1.0) <= 5 / (2 * nz) ** 0.5).all()
        other = t.F.clone()
        other[env, body] = 0
        assert not other.any()                                                    # nothing but target-brick rows is ever written
    finally:
        t.close()


def test_train_rlgames_force_scale_end_to_end(tmp_path):
    """train_rlgames --task=BlockAssemblyGraspSim --force_scale 2.0 at 64 envs for 2 epochs: it finishes, task.rb_forces is non-zero only
    on target-brick rows, no contact was lost (contact_results_valid of bench.py: CONTACT_STATS[1] == CONTACT_STATS[3] == 0)"""
    from seqdex_amd.config import get_args
    from seqdex_amd.train_rlgames import build
    args = get_args(["--task=BlockAssemblyGraspSim", "--num_envs=64", "--max_iterations", "2", "--headless", "--force_scale", "2.0",
                     "--logdir", str(tmp_path)])
    t, env, agent, logdir, rank = build(args, minibatch_size=64)
    s = t.sim
    try:
        assert t.force_scale == 2.0 and t.rb_forces.shape == (64, K.NB, 3) and t.random_force_prob.shape == (64,)
        prob = t.random_force_prob.cpu().numpy()
        assert (prob >= np.float32(0.001)).all() and (prob <= np.float32(0.1)).all()
        agent.train()
        torch.cuda.synchronize()
        F = t.rb_forces.cpu().numpy()
        assert np.isfinite(F).all() and np.isfinite(s.REW.cpu().numpy()).all() and np.isfinite(s.OBS.cpu().numpy()).all()
        body = K.B0 + fr.target_brick(np.arange(64))
        rows = F[np.arange(64), body].copy()
        assert (rows != 0).any(), "no env was ever pushed"
        F[np.arange(64), body] = 0
        assert not F.any(), "rb_forces is non-zero outside the target bricks' rows"
        cs = s.CONTACT_STATS.cpu().numpy()
        assert cs[1] == 0 and cs[3] == 0, cs
    finally:
        s.close()
