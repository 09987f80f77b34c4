"""-m gpu: observation and action noise (include/seqdex.h sdx_set_noise) through the compiled gfx950 kernel.

- known operand and isolation at N = 3 for GraspSim (396 columns: the 16-byte path, 297 threads = one full and one partial workgroup) and
  Search (186 columns: column by column, a 2-column tail, 141 threads), and one N = 64 case; the bodies are tests/noise_cases.py, shared
  with the emulated run of tests/test_observation_action_noise.py;
- mean and standard deviation of the white and the correlated part of both shipped blocks at N = 4 096;
- train_rlgames --randomize end to end with the frame past the schedule."""
import numpy as np
import pytest
import yaml

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import noise_cases as K          # noqa: E402
from test_observation_action_noise import shipped      # noqa: E402


def _make(n, **kw):
    from seqdex_amd.sim import SdxSim
    return SdxSim(n, device="cuda:0", **kw)


BACKEND = (_make, lambda t: t.cuda())
COMBOS = [(K.GAUSSIAN, K.ADDITIVE, "linear-mid"), (K.GAUSSIAN, K.SCALING, "none"), (K.UNIFORM, K.ADDITIVE, "constant"),
          (K.UNIFORM, K.SCALING, "linear-mid")]


@pytest.mark.parametrize("kind,n", [("grasp", 3), ("search", 3), ("grasp", 64)])
def test_known_operand(kind, n):
    t = K.Tracked(BACKEND, kind, n)
    try:
        for distribution, operation, schedule in COMBOS:
            K.case_known_operand(t, distribution, operation, schedule)
    finally:
        t.close()


@pytest.mark.parametrize("kind,n,extra", [("grasp", 3, ()), ("search", 3, ("TVALUE_OBS",))])
def test_observation_noise_touches_obs_clamped_only(kind, n, extra):
    K.case_isolation(BACKEND, kind, n, 10, extra=extra)


def test_zero_operand_is_bit_identical_to_noise_off():
    K.case_zero_operand(BACKEND, "grasp", 3, shipped("grasp_sim"))


def test_refresh_actions_and_independence_of_n():
    K.case_refresh(BACKEND, 4, False)
    K.case_actions_not_reclamped(BACKEND, 3)
    K.case_independent_of_n(BACKEND, 8, 16)


N_STAT = 4096


@pytest.fixture(scope="module")
def stat_sim():
    """an Orient simulator that never steps: sdx_pre_physics with no reset flag set and sdx_post_physics leave zero actions and 124
    never-written observation columns, which then hold the additive operand itself"""
    t = K.Tracked(BACKEND, "orient", N_STAT)
    t.s.RESET.zero_()
    yield t
    t.close()


@pytest.mark.parametrize("block", ["observations", "actions"])
@pytest.mark.parametrize("part", ["white", "corr", "uniform-white"])
def test_statistics(stat_sim, block, part):
    """sample mean and standard deviation of one part of one shipped block past its schedule, five standard errors each.  For n independent
    draws of standard deviation sd and kurtosis k: se(mean) = sd / sqrt(n), se(std) = sd sqrt((k - 1) / (4 n)); k = 3 (normal), 1.8 (uniform)."""
    t = stat_sim
    y = shipped("grasp_sim")[block]
    sigma_w, sigma_c = y["range"][1], y["range_correlated"][1]
    if part == "white":
        a, mean, sd, kurt = K.attr(K.GAUSSIAN, K.ADDITIVE, (0.0, sigma_w), (0.0, 0.0), 1, K.STEPS), 0.0, sigma_w, 3.0
    elif part == "corr":
        a, mean, sd, kurt = K.attr(K.GAUSSIAN, K.ADDITIVE, (0.0, 0.0), (0.0, sigma_c), 1, K.STEPS), 0.0, sigma_c, 3.0
    else:
        lo, hi = -sigma_w, 3.0 * sigma_w
        a, mean, sd, kurt = K.attr(K.UNIFORM, K.ADDITIVE, (lo, hi), (0.0, 0.0), 1, K.STEPS), 0.5 * (lo + hi), (hi - lo) / 12 ** 0.5, 1.8
    t.randomize(50000)                                                # past schedule_steps: s = 1
    t.s.set_noise(**{block: a})
    if block == "actions":
        t.pre_physics(t.dev(torch.zeros(N_STAT, 23)))
        x = K.host(t.s.ACTIONS).astype(np.float64).ravel()
    else:
        t.post_physics()
        x = K.host(t.s.OBS_CLAMPED)[:, K.NEVER_WRITTEN["orient"]].astype(np.float64).ravel()
    n = x.size
    assert n == N_STAT * (23 if block == "actions" else 124)
    se_mean, se_std = sd / n ** 0.5, sd * ((kurt - 1.0) / (4.0 * n)) ** 0.5
    print("%s %s: n %d mean %.3e (want %.3e, 5 se %.3e) std %.6e (want %.6e, 5 se %.3e)" % (block, part, n, x.mean(), mean, 5 * se_mean, x.std(), sd, 5 * se_std))
    assert abs(x.mean() - mean) <= 5 * se_mean
    assert abs(x.std() - sd) <= 5 * se_std
    if part == "uniform-white":
        assert x.min() >= np.float32(lo) and x.max() <= np.float32(hi)


def test_train_rlgames_randomize_applies_both_blocks(tmp_path):
    """train_rlgames --randomize for two epochs, the frame past the schedule: the report lists both blocks, what the agent is handed is
    finite and carries the noise (frequency 1 and 4-step episodes: refreshes happen within the run)"""
    from seqdex_amd.config import get_args
    from seqdex_amd.train_rlgames import build
    with open(tmp_path / "env.yaml", "w") as f:
        import os
        cfg = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "seqdex_amd", "cfg",
                                               "allegro_hand_block_assembly_grasp_sim.yaml")))
        cfg["task"]["randomization_params"]["frequency"] = 1
        yaml.safe_dump(cfg, f)
    args = get_args(["--task=BlockAssemblyGraspSim", "--num_envs=64", "--max_iterations", "2", "--headless", "--randomize", "--episode_length", "4",
                     "--cfg_env", str(tmp_path / "env.yaml"), "--logdir", str(tmp_path)])
    t, env, agent, logdir, rank = build(args, minibatch_size=64)
    s = t.sim
    try:
        noise = t.randomization_report["noise"]
        assert set(noise) == {"observations", "actions"} and noise["actions"]["range"] == [0.0, 0.05]
        assert "observations" in t.randomization_report["noop"]        # parse() keeps its report shape
        s.DR_FRAME[0] = 50000
        agent.train()
        torch.cuda.synchronize()
        assert int(s.DR_FRAME[1]) > 50000                              # a refresh happened: the schedule factor is 1 now
        obs, clean = s.OBS_CLAMPED.cpu().numpy(), s.OBS.cpu().numpy()
        assert np.isfinite(obs).all() and np.isfinite(s.ACTIONS.cpu().numpy()).all() and np.isfinite(s.REW.cpu().numpy()).all()
        d = obs - np.clip(clean, -s._desc.clip_obs, s._desc.clip_obs)
        assert (d != 0).mean() > 0.9 and np.abs(d).max() < 0.05           # sigma 0.002 + 0.001: noise, not garbage
    finally:
        s.close()
