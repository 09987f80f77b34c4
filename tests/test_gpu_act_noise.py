"""-m gpu: the exploration noise sdxp_act draws for itself (eps = None: randn() of csrc/sdxp_rollout.hip k_act_heads) against the numpy
restatement tests/helpers/device_rng.py act_noise, the rules of its counter and stream, the other outputs of such a call, and the
dataset rows k_act_heads writes at the edges of the widths sdxp_create accepts.  The distribution of the restated stream is checked on
the CPU (tests/test_device_rng_restatement.py); here the device is held to the restatement, draw by draw."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from helpers import device_rng as R                   # noqa: E402
from oracle.ppo_oracle import DEFAULT_CFG, PPOOracle  # noqa: E402

f32 = np.float32
N, H, A = 3, 8, 23
UNITS = (1024, 512, 256)


def logstd_values(a):
    """distinct, non-zero: sigma between 0.45 and 1.5"""
    return (f32(-0.787) + f32(0.05) * np.arange(a, dtype=f32)).astype(f32)


def make_agent(n=N, seed=22, horizon=H, obs_dim=None, state_dim=None, act_dim=A, minibatch=None):
    from seqdex_amd.ppo import SdxPPO, make_config
    cfg = make_config(n, obs_dim=obs_dim, state_dim=state_dim)
    cfg.horizon, cfg.act_dim = horizon, act_dim
    if minibatch:
        cfg.minibatch = cfg.cv_minibatch = minibatch
    agent = SdxPPO(n, config=cfg, seed=seed)
    off = 0
    k = cfg.obs_dim
    for u in UNITS:
        off += u * k + u
        k = u
    off += act_dim * k + act_dim                          # the mu head; logstd follows (SDXP_T_AC_PARAMS layout)
    agent.t["AC_PARAMS"][off:off + act_dim] = torch.from_numpy(logstd_values(act_dim)).cuda()
    return agent


def inputs(n, t, obs_dim=396, state_dim=564):
    g = torch.Generator().manual_seed(100 + t)
    obs = torch.randn(n, obs_dim, generator=g).clamp(-5, 5)
    st = (torch.randn(n, state_dim, generator=g) * 2).clamp(-5, 5)
    dones = (torch.rand(n, generator=g) < 0.3).long()
    return obs, st, dones


def host(t):
    return t.detach().cpu().numpy().copy()


def rollouts(agent, n, count=2, eps_at=()):
    """`count` rollouts of H sdxp_act calls with eps = None (calls whose number is in `eps_at` are given an eps); per call the returned
    actions and the rows of the dataset the call wrote"""
    out, call = [], 0
    for _ in range(count):
        acts = []
        for t in range(H):
            obs, st, dones = inputs(n, t)
            eps = torch.full((n, A), 0.25).cuda() if call in eps_at else None
            acts.append(host(agent.act(t, obs.cuda(), st.cuda(), dones.cuda(), eps)))
            call += 1
        torch.cuda.synchronize()
        T = {k: host(agent.t[k]) for k in ("MB_ACTIONS", "MB_MUS", "MB_SIGMAS", "MB_NEGLOGP")}
        for t in range(H):
            out.append(dict(a=acts[t], mb_a=T["MB_ACTIONS"][:, t], mu=T["MB_MUS"][:, t], sigma=T["MB_SIGMAS"][:, t], nlp=T["MB_NEGLOGP"][:, t]))
    return out


def noise_ratio(rec, seed, counter, n):
    """largest |a - a_ref| / (sigma E + ulp(a)) of one call, a_ref = fl(mu + fl(sigma eps_ref)), E = 8 2^-23 max(1, r)"""
    eps, r = R.act_noise_parts(seed, counter, n, A)[:2]
    a_ref = rec["mu"] + rec["sigma"] * eps
    assert a_ref.dtype == np.float32
    E = 8.0 * 2.0 ** -23 * np.maximum(1.0, r.astype(np.float64))
    bound = rec["sigma"].astype(np.float64) * E + np.spacing(np.abs(a_ref)).astype(np.float64)
    return float((np.abs(rec["a"].astype(np.float64) - a_ref.astype(np.float64)) / bound).max())


def device_eps(rec):
    return (rec["a"].astype(np.float64) - rec["mu"]) / rec["sigma"]


@pytest.fixture(scope="module")
def run22():
    agent = make_agent()
    try:
        yield rollouts(agent, N)
    finally:
        agent.close()


def test_actions_are_mu_plus_sigma_times_the_restated_noise(run22):
    """16 calls (two rollouts) of a fresh handle at N = 3: the returned actions against fl(mu + fl(sigma eps_ref)) with the handle's own
    MB_MUS / MB_SIGMAS and eps_ref = act_noise(seed, call number), within sigma E + ulp(a), E = 8 2^-23 max(1, r), r = sqrt(-2 ln u1):
    u1, u2 and the cosine's argument are reproduced bit for bit, logf is within 1 ulp, sqrtf correctly rounded, cosf within 2 ulp, the
    restatement's own roundings and the two products add the rest - about 5 2^-23 r; 8 leaves a 1.6 x margin.  A wrong counter, stream
    or bit field is off by order 1.
    Largest |a - a_ref| / bound seen on an MI355X: 0.17 (profiles/device_rng_gpu_bounds.txt)."""
    sig = run22[0]["sigma"]
    np.testing.assert_array_equal(sig, np.broadcast_to(sig[0], sig.shape))
    assert len(set(sig[0].tolist())) == A and (np.abs(sig[0] - 1.0) > 0.01).all()        # sigma is not 1, and differs by column
    worst = 0.0
    for counter, rec in enumerate(run22):
        ratio = noise_ratio(rec, 22, counter, N)
        worst = max(worst, ratio)
        assert ratio <= 1.0, "call %d: |a - a_ref| is %.3g of its bound" % (counter, ratio)
    print("act noise: largest |a - a_ref| / (sigma E + ulp) over %d calls = %.4f" % (len(run22), worst))
    eps = np.stack([device_eps(r) for r in run22])
    assert 0.5 < eps.std() < 1.5 and np.abs(eps).max() > 2.0                             # noise of order 1 was added


def test_counter_counts_calls_of_the_handle_and_goes_on_across_rollouts(run22):
    """the counter is the number of sdxp_act calls made on the handle so far: it does not restart at t = 0 of the second rollout (call 8
    is not call 0 again) and no two calls share a draw"""
    ref = [R.act_noise(22, c, N, A) for c in range(2 * H)]
    for c, rec in enumerate(run22):
        d = np.abs(device_eps(rec)[None] - np.stack(ref)).max(axis=(1, 2))
        assert int(d.argmin()) == c and d[c] < 1e-4
        assert np.delete(d, c).min() > 0.5, "call %d also fits another counter" % c


def test_calls_given_eps_count_and_a_fresh_handle_starts_at_zero(run22):
    """a second handle with the same seed: calls 0 and 2 are given an eps, calls 1 and 3.. draw their own - with counters 1 and 3..;
    where both handles drew for themselves (calls 1, 3..7 of the first rollout) the actions are bitwise equal"""
    agent = make_agent()
    try:
        got = rollouts(agent, N, count=1, eps_at=(0, 2))
    finally:
        agent.close()
    for c, rec in enumerate(got):
        if c in (0, 2):
            np.testing.assert_allclose(device_eps(rec), 0.25, rtol=0, atol=1e-5)
            assert not np.array_equal(rec["a"], run22[c]["a"])
        else:
            assert noise_ratio(rec, 22, c, N) <= 1.0, c
            np.testing.assert_array_equal(rec["a"].view(np.uint32), run22[c]["a"].view(np.uint32), err_msg="call %d" % c)


def test_a_fresh_handle_repeats_the_sequence_bit_for_bit(run22):
    agent = make_agent()
    try:
        got = rollouts(agent, N, count=1)
    finally:
        agent.close()
    for c, rec in enumerate(got):
        np.testing.assert_array_equal(rec["a"].view(np.uint32), run22[c]["a"].view(np.uint32), err_msg="call %d" % c)


def test_stream_is_env_times_64_plus_column(run22):
    """env e draws the same numbers at N = 3 and at N = 64"""
    n = 64
    agent = make_agent(n=n)
    try:
        recs = []
        for t in range(2):
            obs, st, dones = inputs(n, t)
            a = host(agent.act(t, obs.cuda(), st.cuda(), dones.cuda(), None))
            torch.cuda.synchronize()
            recs.append(dict(a=a, mu=host(agent.t["MB_MUS"])[:, t], sigma=host(agent.t["MB_SIGMAS"])[:, t]))
    finally:
        agent.close()
    for c, rec in enumerate(recs):
        assert noise_ratio(rec, 22, c, n) <= 1.0
        np.testing.assert_allclose(device_eps(rec)[:N], device_eps(run22[c]), rtol=0, atol=1e-4)


def test_two_ranks_draw_uncorrelated_sequences(run22):
    """seeds 22 and 23 (rank 0 and rank 1 of a shipped run): the correlation of the two handles' own draws over 16 calls is within 4 / sqrt(n)"""
    agent = make_agent(seed=23)
    try:
        other = rollouts(agent, N)
    finally:
        agent.close()
    for c, rec in enumerate(other):
        assert noise_ratio(rec, 23, c, N) <= 1.0, c
    x = np.stack([device_eps(r) for r in run22]).ravel()
    y = np.stack([device_eps(r) for r in other]).ravel()
    n = x.size
    assert n == 2 * H * N * A
    corr = float(np.corrcoef(x, y)[0, 1])
    print("correlation of seeds 22 and 23 over %d draws: %.4f (bound %.4f)" % (n, corr, 4.0 / math.sqrt(n)))
    assert abs(corr) <= 4.0 / math.sqrt(n)


def test_neglogp_and_dataset_actions_of_a_call_without_eps(run22):
    """MB_NEGLOGP = 0.5 sum z^2 + sum logstd + 0.5 A ln 2 pi in float64 from the device's own a, mu, sigma, within rtol (A + 4) 2^-23;
    MB_ACTIONS is the returned action, bit for bit"""
    ls = logstd_values(A).astype(np.float64)
    for c, rec in enumerate(run22):
        np.testing.assert_array_equal(rec["mb_a"].view(np.uint32), rec["a"].view(np.uint32), err_msg="call %d" % c)
        z = device_eps(rec)
        want = 0.5 * (z * z).sum(-1) + ls.sum() + 0.5 * A * math.log(2.0 * math.pi)
        np.testing.assert_allclose(rec["nlp"].astype(np.float64), want, rtol=(A + 4) * 2.0 ** -23, atol=0, err_msg="call %d" % c)


# ------------------------------------------------------------------------------------------------------------------ row writes at the edges
@pytest.mark.parametrize("obs_dim,state_dim,act_dim", [(4, 1024, 1), (1024, 4, 32), (260, 256, 23), (396, 564, 23)])
def test_dataset_rows_at_the_edges_of_the_accepted_widths(obs_dim, state_dim, act_dim):
    """k_act_heads copies the observation and state rows as clamped 16-byte pieces, 4 rounds of 64 lanes: one piece per row (width 4), all
    256 (1024), one piece in the second round (260), exactly one full round (256); act_dim 1, 23 and 32.  With an injected eps: MB_OBS,
    MB_STATES and MB_DONES are the inputs bit for bit, MB_SIGMAS = exp(logstd) to 1 ulp, the rest matches oracle/ppo_oracle.py built at
    the same widths (tolerances of tests/test_gpu_ppo_parity.py test_rollout_gae_and_dataset).  The dataset starts as NaN: a row left
    unwritten shows."""
    n, hz = N, 2
    agent = make_agent(n=n, horizon=hz, obs_dim=obs_dim, state_dim=state_dim, act_dim=act_dim, minibatch=2)
    try:
        oc = dict(DEFAULT_CFG)
        oc.update(obs_dim=obs_dim, state_dim=state_dim, act_dim=act_dim, horizon=hz, minibatch=2)
        orc = PPOOracle(oc, seed=0)
        orc.load_flat(agent.t["AC_PARAMS"].cpu(), agent.t["CV_PARAMS"].cpu())
        names = ("MB_OBS", "MB_STATES", "MB_DONES", "MB_SIGMAS", "MB_MUS", "MB_VALUES", "MB_NEGLOGP", "MB_ACTIONS")
        for k in names:
            agent.t[k].fill_(float("nan"))
        assert tuple(agent.t["MB_OBS"].shape) == (n, hz, obs_dim) and tuple(agent.t["MB_STATES"].shape) == (n, hz, state_dim)
        assert tuple(agent.t["MB_ACTIONS"].shape) == (n, hz, act_dim)
        fed, want, acts = [], [], []
        for t in range(hz):
            obs, st, dones = inputs(n, t, obs_dim, state_dim)
            dones[0] = 1 - t                                                    # both values of the flag, in both steps
            dones[1] = t
            eps = torch.randn(n, act_dim, generator=torch.Generator().manual_seed(7 + t))
            acts.append(host(agent.act(t, obs.cuda(), st.cuda(), dones.cuda(), eps.cuda())))
            fed.append((obs.numpy(), st.numpy(), dones.numpy()))
            want.append({k: v.numpy() for k, v in orc.act(obs, st, eps).items()})
        torch.cuda.synchronize()
        T = {k: host(agent.t[k]) for k in names}
        for k in names:
            assert not np.isnan(T[k]).any(), k
        sig = np.exp(logstd_values(act_dim).astype(np.float64)).astype(f32)
        for t in range(hz):
            obs, st, dones = fed[t]
            np.testing.assert_array_equal(T["MB_OBS"][:, t].view(np.uint32), obs.view(np.uint32), err_msg="MB_OBS t %d" % t)
            np.testing.assert_array_equal(T["MB_STATES"][:, t].view(np.uint32), st.view(np.uint32), err_msg="MB_STATES t %d" % t)
            np.testing.assert_array_equal(T["MB_DONES"][:, t], dones.astype(f32), err_msg="MB_DONES t %d" % t)
            err = np.abs(T["MB_SIGMAS"][:, t].astype(np.float64) - sig[None].astype(np.float64))
            assert (err <= np.spacing(sig)[None]).all(), "MB_SIGMAS t %d" % t
            w = want[t]
            np.testing.assert_array_equal(T["MB_ACTIONS"][:, t].view(np.uint32), acts[t].view(np.uint32))
            np.testing.assert_allclose(acts[t], w["actions"], rtol=2e-4, atol=2e-4)
            np.testing.assert_allclose(T["MB_MUS"][:, t], w["mus"], rtol=2e-4, atol=2e-4)
            np.testing.assert_allclose(T["MB_VALUES"][:, t], w["values"], rtol=2e-4, atol=2e-4)
            np.testing.assert_allclose(T["MB_NEGLOGP"][:, t], w["neglogp"], rtol=1e-4, atol=1e-4)
    finally:
        agent.close()
