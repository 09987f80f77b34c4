"""closed-form checks that pin oracle/ppo_oracle.py (PARITY UNPINNED vs rl_games, see its header)."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from oracle.ppo_oracle import DEFAULT_CFG, PPOOracle, RunningMeanStd, census_summary  # noqa: E402


def small_cfg(**kw):
    c = dict(DEFAULT_CFG)
    c.update(obs_dim=12, state_dim=8, act_dim=3, units=[16, 8, 8], minibatch=4, mini_epochs=2)
    c.update(kw)
    return c


def test_gae_hand_computed():
    o = PPOOracle(small_cfg())
    r = torch.tensor([[1.0], [2.0], [3.0]]); v = torch.tensor([[0.5], [0.4], [0.3]])
    d = torch.tensor([[0.0], [0.0], [1.0]])                # done flag stored BEFORE step t (PS:347)
    adv, ret = o.gae(r, v, d, torch.tensor([0.2]), torch.tensor([0.0]))
    g, lam = 0.99, 0.95
    a2 = 3.0 + g * 0.2 - 0.3
    a1 = 2.0 + g * 0.3 * 0.0 - 0.4                          # next step (t=2) starts a new episode: no bootstrap
    a0 = 1.0 + g * 0.4 - 0.5 + g * lam * a1
    np.testing.assert_allclose(adv.squeeze(1).numpy(), [a0, a1, a2], rtol=1e-6)
    np.testing.assert_allclose(ret.numpy(), (adv + v).numpy())


def test_neglogp_matches_torch_normal():
    mu, ls = torch.randn(5, 3), torch.randn(3) * 0.1
    x = torch.randn(5, 3)
    want = -torch.distributions.Normal(mu, ls.exp()).log_prob(x).sum(-1)
    got = PPOOracle.neglogp(x, mu, ls.exp().expand_as(mu), ls)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-5)


def test_running_mean_std_single_merge_closed_form():
    """one merge of a 4-sample batch into the prior (count 1, mean 0, var 1).  rl_games feeds the UNBIASED batch
    variance into the parallel-variance formula (m_b = var_unbiased * batch_count), reproduced here."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4, 6, generator=g) * 3 + 1
    r = RunningMeanStd(6)
    r.update(x)
    xb = x.double().mean(0)
    ss = ((x.double() - xb) ** 2).sum(0)
    np.testing.assert_allclose(r.mean.numpy(), (4 * xb / 5).numpy(), rtol=1e-12)
    np.testing.assert_allclose(r.var.numpy(), ((1.0 + (4.0 / 3.0) * ss + xb ** 2 * 4.0 / 5.0) / 5.0).numpy(), rtol=1e-12)
    assert float(r.count) == 5.0
    y = r(x)
    assert float(y.abs().max()) <= 5.0


def test_update_first_step_is_plain_clipped_adam():
    """first minibatch: ratio == 1 -> a_loss grad = -A * dlogp; Adam's first step moves every touched weight by ~lr."""
    torch.manual_seed(0)
    c = small_cfg(adaptive_lr=False, mini_epochs=1)
    o = PPOOracle(c)
    n = 4
    obs, st = torch.randn(n, 12), torch.randn(n, 8)
    r = o.act(obs, st, torch.randn(n, 3))
    ds = dict(obs=obs, states=st, actions=r["actions"], mus=r["mus"].clone(), sigmas=r["sigmas"].clone(),
              neglogp=r["neglogp"], values=r["values"], returns=r["values"] + torch.tensor([1.0, -1.0, 0.5, -0.5]))
    before = o.ac_flat().clone()
    stats = o.update(ds)
    delta = (o.ac_flat() - before).abs()
    assert stats["kl"][0] < 1e-4                                  # KL of a policy with itself (only the 1e-5 epsilons)
    assert delta.max() <= c["lr"] * 1.0001 and delta.max() > 0.5 * c["lr"]
    assert abs(stats["a"][0]) < 1e-6 + abs(float((-(ds["advantages"])).mean()))   # ratio == 1: a_loss = -A
    assert stats["gnorm"][0] > 0


def test_adaptive_lr_rule():
    c = small_cfg()
    o = PPOOracle(c)
    o.lr = 3e-4
    # the legacy schedule (PS:306-312): kl > 2*thr -> lr/1.5 ; kl < thr/2 -> lr*1.5 ; clamp [1e-6, 1e-2]
    for kl, want in [(0.05, 3e-4 / 1.5), (0.001, 3e-4 * 1.5), (0.02, 3e-4)]:
        lr = 3e-4
        if kl > 2 * c["kl_threshold"]:
            lr = max(lr / 1.5, 1e-6)
        if kl < 0.5 * c["kl_threshold"]:
            lr = min(lr * 1.5, 1e-2)
        assert math.isclose(lr, want)


def _small_dataset(o, n=8, seed=1):
    g = torch.Generator().manual_seed(seed)
    obs, st = torch.randn(n, 12, generator=g), torch.randn(n, 8, generator=g)
    r = o.act(obs, st, torch.randn(n, 3, generator=g))
    return dict(obs=obs, states=st, actions=r["actions"], mus=r["mus"].clone(), sigmas=r["sigmas"].clone(), neglogp=r["neglogp"],
                values=r["values"], returns=r["values"] + torch.randn(n, generator=g))


def test_entropy_term_gradient_is_minus_coef_on_logstd_only():
    """ac_loss with the entropy of the policy, sum_a(0.5 + 0.5 log 2 pi + logstd_a): against the same loss without it the gradient
    differs by exactly -entropy_coef on every logstd component and by nothing anywhere else."""
    o = PPOOracle(small_cfg())
    with torch.no_grad():
        o.logstd.copy_(torch.tensor([0.3, -0.2, 0.1]))
    ent = PPOOracle.entropy(o.logstd)
    np.testing.assert_allclose(float(ent), sum(0.5 + 0.5 * math.log(2 * math.pi) + x for x in (0.3, -0.2, 0.1)), rtol=1e-6)
    np.testing.assert_allclose(float(ent), float(torch.distributions.Normal(torch.zeros(3), o.logstd.exp()).entropy().sum()), rtol=1e-6)
    obs = torch.randn(4, 12)
    grads = []
    for coef in (0.0, 0.02):
        for p in o.ac_params:
            p.grad = None
        mu, v = o.actor(obs), o.critic(obs).squeeze(-1)
        a = ((mu * o.logstd.exp()) ** 2).sum(-1).mean()                  # any loss that touches every parameter
        PPOOracle.ac_loss(a, (v ** 2).mean(), 1.0, PPOOracle.entropy(o.logstd), coef, mu.abs().sum(-1).mean(), 1e-3).backward()
        grads.append([p.grad.clone() for p in o.ac_params])
    for p, g0, g1 in zip(o.ac_params, *grads):
        want = torch.full_like(g0, -0.02) if p is o.logstd else torch.zeros_like(g0)
        np.testing.assert_allclose((g1 - g0).numpy(), want.numpy(), rtol=0, atol=1e-8)


def test_update_carries_the_entropy_coefficient():
    """update() with entropy_coef: the first step's logstd moves the way -entropy_coef says when nothing else acts on it (advantage 0)"""
    c = small_cfg(adaptive_lr=False, mini_epochs=1, minibatch=8, entropy_coef=0.02, normalize_advantage=False)
    o = PPOOracle(c)
    ds = _small_dataset(o)
    ds["returns"] = ds["values"].clone()                               # advantage 0: the policy loss has no gradient
    st = o.update(ds)
    np.testing.assert_allclose(o.logstd.detach().numpy(), c["lr"], rtol=1e-4)       # Adam's first step: -lr * sign(g), g = -0.02
    np.testing.assert_allclose(st["entropy"][0], 3 * (0.5 + 0.5 * math.log(2 * math.pi)), rtol=1e-6)


def test_truncate_grads_off_is_plain_adam_on_the_unscaled_gradient():
    c = small_cfg(adaptive_lr=False, mini_epochs=1, minibatch=8, truncate_grads=False, grad_norm=1e-3)
    o, twin = PPOOracle(c), PPOOracle(c)
    ds = _small_dataset(o)
    ds2 = {k: v.clone() for k, v in ds.items()}
    # the same step by hand on the twin: the oracle's loss, torch.optim.Adam, no clipping anywhere
    adv = PPOOracle.normalize_advantages(ds2["returns"], ds2["values"])
    mu = twin.actor(ds2["obs"]); sigma = torch.exp(twin.logstd).expand_as(mu)
    ratio = torch.exp(ds2["neglogp"] - PPOOracle.neglogp(ds2["actions"], mu, sigma, twin.logstd))
    a_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 0.9, 1.1)).mean()
    c_loss = twin._critic_loss(ds2["values"], twin.critic(ds2["obs"]).squeeze(-1), ds2["returns"]).mean()
    b_loss = (torch.clamp_min(mu - 1.1, 0.0) ** 2 + torch.clamp_max(mu + 1.1, 0.0) ** 2).sum(-1).mean()
    (a_loss + 0.5 * c_loss + 1e-3 * b_loss).backward()
    norm = torch.sqrt(sum((p.grad ** 2).sum() for p in twin.ac_params))
    torch.optim.Adam(twin.ac_params, lr=c["lr"], eps=1e-8).step()
    st = o.update(ds)
    assert float(norm) > 100 * c["grad_norm"]                          # clipping would have scaled the gradient by < 0.01
    np.testing.assert_allclose(st["gnorm"][0], float(norm), rtol=1e-5)  # the norm is still reported
    np.testing.assert_allclose(o.ac_flat().numpy(), twin.ac_flat().numpy(), rtol=0, atol=1e-7)
    # and with truncation on the same step differs: Adam's epsilon makes the scale visible
    on = PPOOracle(small_cfg(adaptive_lr=False, mini_epochs=1, minibatch=8, grad_norm=1e-3))
    on.update({k: v.clone() for k, v in ds2.items()})
    assert np.abs(on.ac_flat().numpy() - twin.ac_flat().numpy()).max() > 1e-6


def test_cv_normalize_input_off_is_the_bare_network():
    o = PPOOracle(small_cfg(cv_normalize_input=False))
    st = torch.randn(6, 8) * 3
    with torch.no_grad():
        bare = o.cv(st).squeeze(-1)
    np.testing.assert_array_equal(o.values(st).numpy(), bare.numpy())
    np.testing.assert_array_equal(o.act(torch.randn(6, 12), st, torch.zeros(6, 3))["values"].numpy(), bare.numpy())
    on = PPOOracle(small_cfg())                                        # default: mean 0, var 1 is still x / sqrt(1 + 1e-5) clamped to +-5
    with torch.no_grad():
        want = on.cv(torch.clamp(st / math.sqrt(1 + 1e-5), -5, 5)).squeeze(-1)
    np.testing.assert_allclose(on.values(st).numpy(), want.numpy(), rtol=1e-6, atol=1e-7)
    assert np.abs(on.values(st).numpy() - on.cv(st).squeeze(-1).detach().numpy()).max() > 1e-4


def test_census_counts_hand_made_rows():
    """one minibatch whose decisions are known by construction"""
    c = small_cfg(adaptive_lr=True, mini_epochs=1, minibatch=8, normalize_advantage=False)
    o = PPOOracle(c)
    ds = _small_dataset(o)
    with torch.no_grad():
        v = o.critic(ds["obs"]).squeeze(-1)
    ds["neglogp"] = ds["neglogp"] + torch.tensor([0.25, 0.25, -0.25, -0.25, 0.0, 0.0, 0.0, 0.0])      # ratio = exp(shift)
    dr = torch.tensor([1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0])                                 # = advantage
    ds["values"] = v + torch.tensor([0.0, 0.05, -0.05, 0.0, 0.3, 0.3, -0.3, -0.3])                   # critic: 4 inside, 4 outside
    ds["returns"] = ds["values"] + dr
    s = census_summary(o.update(ds)["census"])
    r = s["rows"]
    assert (r["ratio_above_adv_pos"], r["ratio_above_adv_neg"], r["ratio_below_adv_pos"], r["ratio_below_adv_neg"], r["ratio_inside"]) == (1, 1, 1, 1, 4)
    # v below the stored value by 0.3: clipped value = stored - 0.1; return above (dr > 0): the unclipped error is larger (c1), below: c2
    assert (r["critic_clip_inside"], r["critic_clip_outside_c1"], r["critic_clip_outside_c2"]) == (4, 2, 2)
    assert r["mu_above"] == 0 and r["mu_below"] == 0
    assert s["steps"]["lr_raised"] == 1 and s["steps"]["lr_lowered"] == 0           # KL of the policy with itself
    np.testing.assert_allclose(s["margins"]["ratio"], 0.1, atol=1e-4)               # the ratio-1 rows are 0.1 from both ends
    np.testing.assert_allclose(s["margins"]["critic_clip"], 0.05, atol=1e-5)


@pytest.mark.parametrize("n,minibatch,case", [(16, 4, "defaults"), (16, 2, "defaults"), (16, 8, "defaults"), (48, 48, "defaults"),
                                               (16, 4, "clip_value_0"), (48, 48, "clip_value_0"), (48, 12, "defaults"), (72, 72, "defaults")])
def test_branch_rich_data_census_on_the_oracle_alone(n, minibatch, case):
    """the data of tests/test_gpu_ppo_branches.py (tests/helpers/ppo_branch_data.py) is decided on the CPU: its census has every class of
    decision often enough and none close to its boundary.  (The GPU tests assert the same for every case before they compare.)"""
    from helpers import ppo_branch_data as BD
    over = dict(clip_value=0) if case == "clip_value_0" else {}
    orc, ds = BD.branch_dataset(n, minibatch, **over)
    s = census_summary(orc.update(ds)["census"])
    bad = BD.census_violations(s, clip_value=not over, minibatch=minibatch)
    assert not bad, bad
