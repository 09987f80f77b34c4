"""Branch-rich PPO update data for tests/test_gpu_ppo_branches.py (test infrastructure).

The common rollout of tests/test_gpu_ppo_parity.py (library initialisation, randn observations) leaves most branches of the loss cold:
the ratio is 1, the stored values are the value head's own, |mu| stays far below the soft bound 1.1.  Here the dataset is steered, on
the device and in the oracle's copy identically, so that one short update takes every branch several times, and so that no decision
lies so close to its boundary that the device and the oracle could take different sides (oracle/ppo_oracle.py census_summary()).

Everything that decides the data runs on the CPU: the networks are the oracle's own (torch initialisation under a seed, four policy-head
biases moved beyond +-1.1) and are copied INTO the library's parameter buffers, the steering (branch_dataset) draws from a seeded
generator and from the oracle's own outputs.  So tests/test_ppo_oracle.py checks the census of the committed seeds without a GPU, and
tools/ppo_branch_census.py records it for every case (profiles/ppo_branch_tests_bounds.txt).
"""
import copy
import os

import torch

from oracle.ppo_oracle import DEFAULT_CFG, PPOOracle

# policy-head biases beyond the soft bound, both signs (the trunk's contribution to mu stays below 0.6: every element stays on its side)
MU_BIAS = {0: 1.9, 5: -1.9, 11: 2.2, 22: -2.2}

# ambiguity margins: ten times what the parity tests allow between device and oracle for the quantity the decision is taken on
MARGINS = dict(ratio=1e-3, critic_clip=2e-3, cv_clip=2e-3, kl=5e-2, mu=1e-3)
MIN_ROWS, MIN_STEPS = 8, 3
ROW_CLASSES = ("ratio_below_adv_neg", "ratio_below_adv_pos", "ratio_above_adv_neg", "ratio_above_adv_pos", "ratio_inside",
               "critic_clip_inside", "critic_clip_outside_c1", "critic_clip_outside_c2",
               "cv_clip_inside", "cv_clip_outside_c1", "cv_clip_outside_c2", "mu_above", "mu_below")
STEP_CLASSES = ("ac_norm_above", "ac_norm_below", "cv_norm_above", "cv_norm_below", "lr_raised", "lr_lowered")


def oracle_config(minibatch, mini_epochs, **over):
    """oracle configuration of a library configuration: sdxp_config field names, the oracle's keys"""
    oc = dict(DEFAULT_CFG)
    oc.update(minibatch=minibatch, mini_epochs=mini_epochs)
    for k, v in over.items():
        if k in ("clip_value", "truncate_grads", "normalize_advantage", "cv_normalize_input", "adaptive_lr"):
            oc[k] = bool(v)
        elif k in ("cv_minibatch", "cv_mini_epochs", "mixed_precision"):
            continue
        else:
            assert k in oc, k
            oc[k] = v
    return oc


def make_oracle(oc, seed=0):
    """the oracle with torch's initialisation (the library's own: U(+-1/sqrt(fan_in)), zero biases) and MU_BIAS"""
    orc = PPOOracle(oc, seed=seed)
    with torch.no_grad():
        for a, b in MU_BIAS.items():
            orc.actor.head.bias[a] = b
    return orc


def oracle_rollout(orc, n, g, steps=8):
    """test_gpu_ppo_parity.rollout without the library: the same draws from `g` in the same order, the same dataset"""
    H = steps
    obs_l, st_l, rew_l, done_l = [], [], [], []
    buf = dict(actions=[], mus=[], sigmas=[], neglogp=[], values=[])
    for t in range(H):
        obs = torch.randn(n, 396, generator=g).clamp(-5, 5)
        st = torch.randn(n, 564, generator=g).clamp(-5, 5) * 2
        eps = torch.randn(n, 23, generator=g)
        dones = (torch.rand(n, generator=g) < 0.15).long()
        rew = torch.rand(n, generator=g)
        r = orc.act(obs, st, eps)
        for k in buf:
            buf[k].append(r[k])
        obs_l.append(obs); st_l.append(st); rew_l.append(rew); done_l.append(dones.float())
    last_st = torch.randn(n, 564, generator=g)
    last_done = (torch.rand(n, generator=g) < 0.15).long()
    adv, ret = orc.gae(torch.stack(rew_l), torch.stack(buf["values"]), torch.stack(done_l), orc.values(last_st), last_done.float())
    flat = lambda x: torch.stack(x).transpose(0, 1).reshape(n * H, *x[0].shape[1:]).contiguous()
    return dict(obs=flat(obs_l), states=flat(st_l), actions=flat(buf["actions"]), mus=flat(buf["mus"]).clone(),
                sigmas=flat(buf["sigmas"]).clone(), neglogp=flat(buf["neglogp"]), values=flat(buf["values"]),
                returns=ret.transpose(0, 1).reshape(-1).contiguous())


# kinds of a row; blocks of max(8, minibatch) rows cycle through (loud, raise), (loud, lower), (quiet, raise), (quiet, lower)
INSIDE, INSIDE_CRITIC, OUT_C1 = 0, 1, 2
AC_QUIET_ERR, CV_QUIET_ERR = 0.1, 0.2


def _value_design(kind, dr, vc, vv, e):
    """stored value of a row whose critic / central-value outputs are vc / vv when the row is visited.  INSIDE: both heads within e_clip of
    it where they are close enough to each other, else the central value within and the critic clearly outside; INSIDE_CRITIC: the
    critic within.  OUT_C1: both heads
    beyond e_clip on the side away from the return (return = stored + dr), so the unclipped error is the larger one: c1 > c2.
    quiet rows (kind None): both heads beyond e_clip on the side of the return, so the clipped error is the larger one and the row has
    no value gradient: c2 > c1.  Every choice keeps 0.01 from the clip boundary and the return 0.02 from where c1 == c2."""
    lo, hi = min(vc, vv), max(vc, vv)
    if kind is None:
        cands = [lo - 0.4] if dr > 0 else [hi + 0.4]
    elif kind == OUT_C1:
        cands = [hi + 0.3] if dr > 0 else [lo - 0.3]
    else:
        cands = [0.5 * (lo + hi)] if hi - lo <= e else []
        cands += [(vc if kind == INSIDE_CRITIC else vv) + 0.005 * u for u in sorted(range(-17, 18), key=lambda u: abs(abs(u) - 10))]
    for vo in cands:
        ok = True
        for v in (vc, vv):
            d = v - vo
            if abs(abs(d) - e) < 0.01:
                ok = False
            if abs(d) > e:                                  # outside: how far is the return from the point where c1 == c2
                vclip = vo + (e if d > 0 else -e)
                if abs((vo + dr) - 0.5 * (v + vclip)) < 0.02:
                    ok = False
        if ok:
            return vo
    raise AssertionError("no stored value keeps both heads away from their boundaries: %r" % ((kind, dr, vc, vv),))


def branch_dataset(n, minibatch, seed=5, **over):
    """oracle (before the update) + steered dataset for `n` envs x horizon 8, one mini-epoch; CPU only.

    The update is walked minibatch by minibatch on a copy of the oracle.  Before a minibatch's step its rows get, from what the networks
    give for them at that moment (new neglogp, mu, critic value v_c, central value v_v):
      stored neglogp = new neglogp + one of {-0.25, 0, +0.25}: ratio exp(-+0.25) outside [0.9, 1.1], or 1;
      stored value   = _value_design(...), return = stored value + dr with dr from {+-0.3, +-0.7} (quiet rows +-3: the two heads can be 2 apart), fixed per row in
                       advance, so the batch statistics of the advantage are known before the walk;
      stored mu      = mu (KL about 1e-4: the adaptive rule raises the rate) or mu + 0.1 (KL 0.115: it lowers it), per block.
    Quiet blocks hold only rows without policy gradient (ratio clipped on the side where max(L1, L2) is the constant one) and without
    value gradient: gradient norms below grad_norm.  Loud blocks mix the other cases at random under `seed`.
    clip_value off: the stored value only enters through the advantage, so the return itself is put next to the critic's output (policy
    side quiet) or next to the central value's (that optimiser quiet), block by block."""
    e = DEFAULT_CFG["e_clip"]
    oc = oracle_config(minibatch, 1, **over)
    orc = make_oracle(oc)
    ds = oracle_rollout(orc, n, torch.Generator().manual_seed(11))
    walker = copy.deepcopy(orc)
    g = torch.Generator().manual_seed(seed)
    R = ds["neglogp"].shape[0]
    block = max(8, minibatch)
    bidx = torch.arange(R) // block
    shifted = bidx % 2 == 1
    pick = lambda vals: torch.tensor(vals)[torch.randint(len(vals), (R,), generator=g)]
    dr = pick([-0.7, -0.3, 0.3, 0.7])
    if oc["clip_value"]:      # blocks: loud, loud, quiet, quiet (both optimisers), the adaptive rule alternating
        ac_quiet = cv_quiet = bidx % 4 >= 2
        dr = torch.where(ac_quiet, torch.where(torch.arange(R) % 2 == 0, 3.0, -3.0), dr)
    else:                     # without the value clip no return silences both value heads: one optimiser quiet per block, L A C A C A C L.
        # Minibatches up to 8 have no block with a quiet central value (L A L A ...): its gradient norm falls below grad_norm only for
        # errors under 0.05, and Adam turns the rounding of so small an error into steps along d v / d theta: from a 1e-7 perturbation
        # of the parameters the oracle's own central values then drift apart by 0.7 within 32 steps (2e-4 without such blocks)
        pat = torch.tensor([0, 1, 2, 1, 2, 1, 2, 0] if minibatch > 8 else [0, 1, 0, 1, 0, 1, 0, 1])[bidx % 8]
        ac_quiet, cv_quiet = pat == 1, pat == 2
    kind = torch.randint(3, (R,), generator=g)
    # sign of the (normalised) advantage = sign(dr - mean): rows of a block with a quiet policy take the ratio side that has no gradient
    adv_sign = torch.sign(dr - (dr.mean() if oc["normalize_advantage"] else 0.0))
    shift = torch.where(ac_quiet, 0.25 * adv_sign, pick([-0.25, 0.0, 0.25]))
    work = dict(ds)
    work.update(values=ds["values"].clone(), neglogp=ds["neglogp"].clone(), mus=ds["mus"].clone(), sigmas=ds["sigmas"].clone())
    work["returns"] = work["values"] + dr
    final = {k: work[k].clone() for k in ("values", "returns", "neglogp", "mus")}
    for i in range(R // minibatch):
        sl = slice(i * minibatch, (i + 1) * minibatch)
        with torch.no_grad():
            mu = walker.actor(ds["obs"][sl])
            sg = torch.exp(walker.logstd).expand_as(mu)
            nlp = walker.neglogp(ds["actions"][sl], mu, sg, walker.logstd)
            vc = walker.critic(ds["obs"][sl]).squeeze(-1)
            rms = copy.deepcopy(walker.rms)
            if oc["cv_normalize_input"]:
                rms.update(ds["states"][sl])                # the central value sees the statistics that include its own minibatch
            vv = walker.cv(rms(ds["states"][sl]) if oc["cv_normalize_input"] else ds["states"][sl]).squeeze(-1)
        for j in range(minibatch):
            r = i * minibatch + j
            if oc["clip_value"]:
                vo = _value_design(None if ac_quiet[r] else int(kind[r]), float(dr[r]), float(vc[j]), float(vv[j]), e)
            else:             # the return next to the head that is to be quiet, not on it: an error of 0 leaves Adam only rounding noise to normalise
                sgn = 1.0 if r % 2 else -1.0
                vo = (float(vc[j]) + sgn * AC_QUIET_ERR - float(dr[r])) if ac_quiet[r] else \
                     (float(vv[j]) + sgn * CV_QUIET_ERR - float(dr[r])) if cv_quiet[r] else float(vv[j])
            final["values"][r] = vo
            final["returns"][r] = final["values"][r] + dr[r]
            final["neglogp"][r] = nlp[j] + shift[r]
            final["mus"][r] = mu[j] + (0.1 if shifted[r] else 0.0)
        for k in final:
            work[k][sl] = final[k][sl]
        walker.update(work, only=[(0, i)])
    out = dict(ds)
    out.update(final)
    return orc, out


def census_violations(summary, clip_value=True, minibatch=4):
    """names of the census conditions that do not hold (empty: the data is branch-rich and unambiguous).  clip_value off: the library takes
    no value-clip decision, and for minibatches up to 8 no step has the central value's norm below grad_norm (branch_dataset says why)."""
    bad = []
    for k in ROW_CLASSES:
        if "_clip_" in k and not clip_value:               # clip_value off: the library takes no such decision
            continue
        if summary["rows"][k] < MIN_ROWS:
            bad.append("%s: %d row decisions < %d" % (k, summary["rows"][k], MIN_ROWS))
    for k in STEP_CLASSES:
        if k == "cv_norm_below" and not clip_value and minibatch <= 8:
            continue
        if summary["steps"][k] < MIN_STEPS:
            bad.append("%s: %d steps < %d" % (k, summary["steps"][k], MIN_STEPS))
    for k, m in MARGINS.items():
        if k.endswith("_clip") and not clip_value:
            continue
        if summary["margins"][k] < m:
            bad.append("ambiguous %s decision: margin %.3g < %.3g" % (k, summary["margins"][k], m))
    return bad


# ---- GPU side
class env_around_create:
    """SDXP_* variables set around sdxp_create only (the switches are per handle)"""

    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def push_dataset(agent, ds, adv):
    """the steered columns of the oracle's dataset into the library's experience buffer"""
    T = agent.t
    T["MB_NEGLOGP"].reshape(-1).copy_(ds["neglogp"].cuda())
    T["MB_VALUES"].reshape(-1).copy_(ds["values"].cuda())
    T["MB_MUS"].reshape(-1, 23).copy_(ds["mus"].cuda())
    T["RETURNS"].copy_(ds["returns"].cuda())
    T["ADVANTAGES"].copy_(adv.cuda())
