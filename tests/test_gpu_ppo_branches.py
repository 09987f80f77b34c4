"""-m gpu: the PPO update on every path (persistent kernel, hipGraph of the multi-kernel step, GEMM step with fused heads and with the
13-launch head section, and the GEMM step on every trunk-product path: k_gemm by switch and by minibatch size, transposed copies instead of
k_gemm_tt, the 128 x 128 tile, ragged minibatches; each handle says through gemm_paths() which it took) against oracle/ppo_oracle.py
on data that takes every branch of the loss (tests/helpers/ppo_branch_data.py),
at the defaults and with one configuration switch moved at a time; minibatch 2 and 8; the rollout's GAE, advantage normalisation and
episode statistics at their edges.

Every update test first asserts, on the oracle alone, that the data is branch-rich (at least 8 row decisions on every side of the ratio
clip x advantage sign, of the value clip of both value heads and of the mu bound; at least 3 steps on either side of grad_norm for both
optimisers, 3 raised and 3 lowered learning rates) and that no decision lies within ten times the parity bounds of its boundary.

Bounds of the update comparison: those of test_gpu_ppo_parity.test_update_matches_autograd_adam, unchanged.  Two additions: sum_b_loss
like the other loss sums; sum_entropy to 23 * 2e-4 (23 logstd elements, each held to the parameter bound).  The fp32 oracle lands within
6e-5 of the same oracle run in float64 in every case (profiles/ppo_branch_tests_bounds.txt): none of the cases is ill-conditioned."""
import copy
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from helpers import ppo_branch_data as BD  # noqa: E402
from oracle.ppo_oracle import census_summary  # noqa: E402
from test_gpu_ppo_parity import make_pair, rollout  # noqa: E402

# path -> (envs, minibatch, variables around sdxp_create, update_impl(), gemm_paths()).  "persistent" sets nothing: the handle's own choice.
# update_impl() only says "gemm"; gemm_paths() shows that the handle honoured its switch: nt = 0 is k_gemm as the trunk (sdx_gemm.h),
# tt = 0 the fp32 weight gradient from transposed copies (k_gemm_nt<0, EPI_TN>), nt_tile 2 the 128 x 128 tile of k_gemm_nt / k_gemm_tt.
# 72 = 64 + 8 rows: ragged in both tile shapes.  A minibatch of 12 is no multiple of 8: the handle declines NT by itself
NT = dict(nt=1, tt=1, fused_heads=1, nt_tile=0, bf16=0)
PATHS = {"persistent": (16, 4, None, "persistent", None),
         "graph": (16, 4, {"SDXP_UPDATE_IMPL": "graph"}, "graph", None),
         "gemm": (48, 48, None, "gemm", NT),
         "gemm_13_launch_heads": (48, 48, {"SDXP_BIGMB_FUSED_HEADS": "0"}, "gemm", dict(NT, fused_heads=0)),
         "gemm_k_gemm_trunk": (48, 48, {"SDXP_BIGMB_NT": "0"}, "gemm", dict(NT, nt=0, tt=0)),
         "gemm_k_gemm_by_size": (48, 12, None, "gemm", dict(NT, nt=0, tt=0)),
         "gemm_nt_transposed_copies": (48, 48, {"SDXP_BIGMB_TT": "0"}, "gemm", dict(NT, tt=0)),
         "gemm_wide_tile": (48, 48, {"SDXP_NT_TILE": "2"}, "gemm", dict(NT, nt_tile=2)),
         "gemm_wide_tile_ragged": (72, 72, {"SDXP_NT_TILE": "2"}, "gemm", dict(NT, nt_tile=2)),
         "gemm_ragged": (72, 72, None, "gemm", NT)}
# the trunk-product paths run the two cases that reach the trunk differently (cv_normalize_input = 0 changes which staged input the central
# value reads); the other switches live in the heads, which the first four paths cover in every case
TRUNK_PATHS = [p for p in PATHS if p not in ("persistent", "graph", "gemm", "gemm_13_launch_heads")]
TRUNK_CASES = ["defaults", "cv_normalize_input_0"]
CASES = {"defaults": {}, "clip_value_0": dict(clip_value=0), "truncate_grads_0": dict(truncate_grads=0),
         "normalize_advantage_0": dict(normalize_advantage=0), "cv_normalize_input_0": dict(cv_normalize_input=0),
         "entropy_coef_0.02": dict(entropy_coef=0.02), "bounds_loss_coef_0.05": dict(bounds_loss_coef=0.05)}
@functools.lru_cache(maxsize=None)
def reference(n, minibatch, case):
    """oracle side of one (shape, case), computed once and shared by the paths; nothing in it is written afterwards"""
    over = CASES[case]
    orc0, ds = BD.branch_dataset(n, minibatch, **over)
    orc = copy.deepcopy(orc0)
    work = {k: v.clone() for k, v in ds.items()}
    st = orc.update(work)
    return dict(orc0=orc0, ds=ds, adv=work["advantages"], mus_after=work["mus"], st=st, orc=orc,
                summary=census_summary(st["census"]), over=over)


def run_case(path, case, n=None, minibatch=None, expect_impl="path"):
    pn, pmb, env, impl, gemm_paths = PATHS[path]
    n, mb = n or pn, minibatch or pmb
    ref = reference(n, mb, case)
    over, st, orc, summary = ref["over"], ref["st"], ref["orc"], ref["summary"]
    print("census", summary)
    bad = BD.census_violations(summary, clip_value=bool(over.get("clip_value", 1)), minibatch=mb)
    assert not bad, "the data of this case is not branch-rich and unambiguous on the oracle alone:\n  " + "\n  ".join(bad)
    assert np.mean(st["b"]) > 0.1
    if expect_impl == "path":      # k_update_persistent has no entropy term: such a handle declines it
        expect_impl = "graph" if (impl == "persistent" and (over.get("entropy_coef", 0.0) != 0.0 or mb != 4)) else impl
    with BD.env_around_create(env):
        agent, _ = make_pair(n, minibatch=mb, cv_minibatch=mb, mini_epochs=1, cv_mini_epochs=1, **over)
    try:
        if expect_impl is not None:
            assert agent.update_impl() == expect_impl, agent.update_impl()
        if expect_impl == impl:
            assert agent.gemm_paths() == gemm_paths, agent.gemm_paths()
        T = agent.t
        T["AC_PARAMS"].copy_(ref["orc0"].ac_flat().cuda())
        T["CV_PARAMS"].copy_(ref["orc0"].cv_flat().cuda())
        ds0 = rollout(agent, ref["orc0"], n, torch.Generator().manual_seed(11))
        if not over.get("normalize_advantage", 1):     # finish_rollout leaves the raw GAE values
            np.testing.assert_allclose(T["ADVANTAGES"].cpu().numpy(), (ds0["returns"] - ds0["values"]).numpy(), rtol=2e-4, atol=2e-4)
        if not over.get("cv_normalize_input", 1):      # act's stored values and get_values are the bare network's
            with torch.no_grad():
                bare = ref["orc0"].cv(ds0["states"]).squeeze(-1)
                last = torch.randn(n, 564, generator=torch.Generator().manual_seed(12))
                bare_last = ref["orc0"].cv(last).squeeze(-1)
            np.testing.assert_allclose(T["MB_VALUES"].cpu().numpy().reshape(-1), bare.numpy(), rtol=2e-4, atol=2e-4)
            np.testing.assert_allclose(agent.get_values(last.cuda()).cpu().numpy(), bare_last.numpy(), rtol=2e-4, atol=2e-4)
        BD.push_dataset(agent, ref["ds"], ref["adv"])
        agent.update()
        agent.update_status()
        torch.cuda.synchronize()
        c = agent.ctrl()
        nsteps = n * 8 // mb
        assert c.n_mb == nsteps and c.ac_t == nsteps and c.cv_t == nsteps and c.ac_pending == 0
        got = dict(a=c.sum_a_loss / nsteps, c=c.sum_c_loss / nsteps, cv=c.sum_cv_loss / nsteps, b=c.sum_b_loss / nsteps,
                   kl=c.sum_kl / nsteps, entropy=c.sum_entropy / nsteps, lr=c.ac_lr, gnorm=c.ac_gnorm, cv_gnorm=c.cv_gnorm)
        want = dict(a=np.mean(st["a"]), c=np.mean(st["c"]), cv=np.mean(st["cv"]), b=np.mean(st["b"]), kl=np.mean(st["kl"]),
                    entropy=np.mean(st["entropy"]), lr=orc.lr, gnorm=st["gnorm"][-1], cv_gnorm=st["cv_gnorm"][-1])
        ac, cv = T["AC_PARAMS"].cpu().numpy(), T["CV_PARAMS"].cpu().numpy()
        d_ac, d_cv = np.abs(ac - orc.ac_flat().numpy()).max(), np.abs(cv - orc.cv_flat().numpy()).max()
        print("figures", path, case, n, mb, {k: (float(got[k]), float(want[k])) for k in got}, "max |d ac|", d_ac, "max |d cv|", d_cv)
        for k in ("a", "c", "cv", "b"):
            np.testing.assert_allclose(got[k], want[k], rtol=2e-3, atol=2e-4, err_msg=k)
        np.testing.assert_allclose(got["kl"], want["kl"], rtol=5e-3, atol=1e-5)
        np.testing.assert_allclose(got["entropy"], want["entropy"], rtol=0, atol=23 * 2e-4)
        np.testing.assert_allclose(got["lr"], want["lr"], rtol=1e-6)
        np.testing.assert_allclose(got["gnorm"], want["gnorm"], rtol=2e-3)
        np.testing.assert_allclose(got["cv_gnorm"], want["cv_gnorm"], rtol=2e-3)
        assert d_ac < 2e-4, d_ac
        assert d_cv < 5e-4, d_cv
        if over.get("cv_normalize_input", 1):
            np.testing.assert_allclose(T["CV_RMS_MEAN"].cpu().numpy(), orc.rms.mean.numpy(), rtol=1e-6, atol=1e-7)
            np.testing.assert_allclose(T["CV_RMS_VAR"].cpu().numpy(), orc.rms.var.numpy(), rtol=1e-5, atol=1e-7)
            assert abs(c.rms_count - float(orc.rms.count)) < 1e-9
        else:                                          # the statistics keep their initial values
            assert (T["CV_RMS_MEAN"].cpu().numpy() == 0.0).all() and (T["CV_RMS_VAR"].cpu().numpy() == 1.0).all()
            assert c.rms_count == 1.0
        np.testing.assert_allclose(T["MB_MUS"].cpu().numpy().reshape(-1, 23), ref["mus_after"].numpy(), rtol=1e-3, atol=1e-3)
    finally:
        agent.close()


@pytest.mark.parametrize("case,path", [(c, p) for p in PATHS for c in (TRUNK_CASES if p in TRUNK_PATHS else CASES)])
def test_update_on_branch_rich_data(case, path):
    """one update phase (one mini-epoch: 32 minibatches of 4 or of 12, 8 of 48 or of 72) against torch.autograd + Adam, one switch moved at a time.
    entropy_coef != 0 under "persistent": the handle must decline the persistent kernel (which has no entropy term) and say "graph".
    (While k_head and the persistent kernel dropped the term, this case gave on both small-minibatch paths sum_entropy / steps 32.6356
    against 32.7070 and max |d ac| 9.7e-3 against the bound 2e-4.)"""
    run_case(path, case)


@pytest.mark.parametrize("minibatch", [2, 8])
def test_update_minibatch_2_and_8_take_the_graph_step(minibatch):
    """MB_SWITCH instantiates the multi-kernel step for minibatch 2 and 8 as well; the persistent kernel is compiled for 4 only, so the handle
    says "graph" with no variable set"""
    run_case("persistent", "defaults", n=16, minibatch=minibatch)


def test_entropy_term_counts_once_across_ranks():
    """world_size 2, minibatch 4: every rank's dlogstd carries -entropy_coef, the factor exchange SUMS the ranks' dlogstd and the apply
    divides the summed gradient by world_size, so the term enters once.  Two emulated ranks with the same data: the rebuilt (summed)
    logstd gradient is twice the single-rank one, whose difference from an entropy_coef = 0 handle is exactly -entropy_coef, and after
    the apply both land on the same logstd."""
    from seqdex_amd.ppo import SdxPPO, make_config
    n, coef = 16, 0.02
    ref = reference(16, 4, "defaults")

    def agent_of(world, entropy_coef):
        cfg = make_config(n, world_size=world)
        cfg.entropy_coef = entropy_coef
        ag = SdxPPO(n, config=cfg, seed=3)
        ag.t["AC_PARAMS"].copy_(ref["orc0"].ac_flat().cuda())
        ag.t["CV_PARAMS"].copy_(ref["orc0"].cv_flat().cuda())
        rollout(ag, ref["orc0"], n, torch.Generator().manual_seed(11))
        BD.push_dataset(ag, ref["ds"], ref["adv"])
        return ag
    e0, e1, w2 = agent_of(1, 0.0), agent_of(1, coef), agent_of(2, coef)
    try:
        o = ref["orc0"]
        lo = sum(p.numel() for p in o.actor.parameters())          # offset of logstd in the flat layout (ac_flat)
        sl = slice(lo, lo + 23)
        for ag in (e0, e1):
            ag.backward(0, -1)
            ag.backward(0, 0)
        w2.backward_factors(-1)
        w2.backward_factors(0)
        w2.t["FACTORS_ALL"].copy_(torch.stack([w2.t["FACTORS"], w2.t["FACTORS"]]))
        w2.grads_from_factors()
        torch.cuda.synchronize()
        g0, g1, gw = (ag.t["AC_GRADS"].cpu().numpy()[sl].astype(np.float64) for ag in (e0, e1, w2))
        assert np.abs(g0).max() > 1e-3
        np.testing.assert_allclose(g1 - g0, -coef, rtol=0, atol=1e-6)
        np.testing.assert_allclose(gw, 2.0 * g1, rtol=0, atol=2e-6)
        e1.apply(0); e1.apply(1)
        w2.apply(0, float("-inf")); w2.apply(1)
        torch.cuda.synchronize()
        np.testing.assert_allclose(w2.t["AC_PARAMS"].cpu().numpy()[sl], e1.t["AC_PARAMS"].cpu().numpy()[sl], rtol=0, atol=1e-6)
        assert np.abs(e1.t["AC_PARAMS"].cpu().numpy()[sl]).max() > 1e-4                # (logstd starts at 0: the step happened)
    finally:
        for ag in (e0, e1, w2):
            ag.close()


# ---------------------------------------------------------------------------------------------------------------- rollout edges
def _gae_numpy(rew, val, done, last_v, last_done, gamma=0.99, tau=0.95):
    """float64 restatement of discount_values; arrays [N, H] (env-major), done[e, t] = the flag stored before step t"""
    N, H = rew.shape
    adv = np.zeros((N, H))
    last = np.zeros(N)
    for t in reversed(range(H)):
        nonterminal = 1.0 - (last_done if t == H - 1 else done[:, t + 1])
        nextv = last_v if t == H - 1 else val[:, t + 1]
        delta = rew[:, t] + gamma * nextv * nonterminal - val[:, t]
        last = delta + gamma * tau * nonterminal * last
        adv[:, t] = last
    return adv, adv + val


@pytest.mark.parametrize("horizon", [8, 1])
def test_gae_and_advantage_normalisation_edges(horizon):
    """200 envs x horizon 8 = 1600 values: not a multiple of k_adv_norm's 1024 threads, both strided loops run twice for some threads and
    once for others; horizon 1: only the t == H-1 branch of k_gae.  Envs 0..3: done at every step, never done, done only at the last stored
    step, last_dones set; the rest 15 % random.  Once with last_dones, once with None."""
    from seqdex_amd.ppo import SdxPPO, make_config
    n, H = 200, horizon
    cfg = make_config(n)
    cfg.horizon = H
    agent = SdxPPO(n, config=cfg, seed=3)
    try:
        g = torch.Generator().manual_seed(21)
        rew = torch.rand(n, H, generator=g) * 2 - 0.5
        val = torch.randn(n, H, generator=g)
        done = (torch.rand(n, H, generator=g) < 0.15).float()
        last_v = torch.randn(n, generator=g)
        last_done = (torch.rand(n, generator=g) < 0.15).long()
        done[0] = 1.0; done[1] = 0.0; done[2] = 0.0; done[2, H - 1] = 1.0; done[3] = 0.0
        last_done[0] = 1; last_done[1] = 0; last_done[2] = 0; last_done[3] = 1
        T = agent.t
        T["MB_REWARDS"].copy_(rew.cuda()); T["MB_VALUES"].copy_(val.cuda()); T["MB_DONES"].copy_(done.cuda())
        for ld in (last_done, None):
            agent.discount_values(last_v.cuda(), None if ld is None else ld.cuda())
            torch.cuda.synchronize()
            adv, ret = _gae_numpy(rew.double().numpy(), val.double().numpy(), done.double().numpy(), last_v.double().numpy(),
                                  np.zeros(n) if ld is None else ld.double().numpy())
            np.testing.assert_allclose(T["RETURNS"].cpu().numpy(), ret.reshape(-1), rtol=2e-4, atol=2e-4)
            np.testing.assert_allclose(T["ADVANTAGES"].cpu().numpy(), adv.reshape(-1), rtol=2e-4, atol=2e-4)
            agent.prepare_dataset()
            torch.cuda.synchronize()
            a = adv.reshape(-1)
            np.testing.assert_allclose(T["ADVANTAGES"].cpu().numpy(), (a - a.mean()) / (a.std(ddof=1) + 1e-8), rtol=2e-3, atol=2e-3)
    finally:
        agent.close()


def test_episode_statistics_over_two_rollouts():
    """games_cnt / games_sum_rew / games_sum_len (float atomics of k_store_rewards) against a numpy count over two scripted 8-step rollouts
    of 300 envs (two blocks).  Rewards are small integers: the sums are exact in any order.  The statistics restart with every rollout
    (act at t = 0) while the running episode reward / length of an env that was not done carries over into the second rollout."""
    from seqdex_amd.ppo import SdxPPO, make_config
    n, H = 300, 8
    agent = SdxPPO(n, config=make_config(n), seed=3)
    try:
        g = torch.Generator().manual_seed(31)
        cur_rew, cur_len = np.zeros(n), np.zeros(n)
        carried = 0
        for ro in range(2):
            cnt = sum_rew = sum_len = 0.0
            for t in range(H):
                obs, st = torch.randn(n, 396, generator=g), torch.randn(n, 564, generator=g)
                rew = torch.randint(0, 4, (n,), generator=g).float()
                done = (torch.rand(n, generator=g) < 0.1).long()
                if t == 0:
                    done[:8] = 0
                done[0] = 1                                    # env 0: done after every step; env 1: never
                done[1] = 0
                agent.act(t, obs.cuda(), st.cuda(), None, torch.zeros(n, 23).cuda())
                agent.store_rewards(t, rew.cuda(), done.cuda() if (ro, t) != (1, 3) else None)     # None: nobody is done
                d = done.numpy().astype(bool) if (ro, t) != (1, 3) else np.zeros(n, bool)
                cur_rew += rew.numpy(); cur_len += 1
                if ro == 1:
                    carried += int((d & (cur_len > t + 1)).sum())      # episodes that began in the first rollout
                cnt += d.sum(); sum_rew += cur_rew[d].sum(); sum_len += cur_len[d].sum()
                cur_rew[d] = 0; cur_len[d] = 0
            torch.cuda.synchronize()
            c = agent.ctrl()
            assert cnt > 20
            assert (c.games_cnt, c.games_sum_rew, c.games_sum_len) == (cnt, sum_rew, sum_len), (ro, c.games_cnt, c.games_sum_rew, c.games_sum_len)
        assert carried > 20
    finally:
        agent.close()
