"""seqdex_amd/csrc/sdxp_ppo_terms.h - the one statement of the PPO update's loss terms, their gradients and the step rules that k_head,
k_big_head, k_big_heads, k_ctrl and the apply kernels call - compiled for the CPU (tests/hipemu/ppo_terms_driver.cpp: plain loops over
rows and actions) against oracle/ppo_oracle.py on the branch-rich data of tests/helpers/ppo_branch_data.py.  No GPU.

Per minibatch of one mini-epoch the driver gets the oracle's own mu, value outputs and logstd; torch.autograd on the oracle's losses
gives the gradients.  Bound of every loss / gradient comparison: rtol 1e-5, atol 1e-6 (d loss / d logstd: the rtol is taken of its terms'
absolute sum, test_loss_terms_and_gradients_match_autograd says why).  Both sides evaluate the same fp32 formula on the
same inputs with no sum longer than 23 terms; they differ by the expf / logf implementations (a few ulp) and by the cancellation in the
KL summand (absolute, order 1e-7); the census keeps every branch decision away from its boundary."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from helpers import ppo_branch_data as BD  # noqa: E402
from oracle.ppo_oracle import census_summary  # noqa: E402
from tests import hipemu  # noqa: E402

N, MB, A = 16, 4, 23
CASES = {"defaults": {}, "clip_value_0": dict(clip_value=0), "entropy_and_bounds": dict(entropy_coef=0.02, bounds_loss_coef=0.05)}
RTOL, ATOL = 1e-5, 1e-6
f32 = C.c_float


@functools.lru_cache(maxsize=None)
def lib():
    l = C.CDLL(hipemu.build_ppo_terms())
    l.ppo_terms_minibatch.argtypes = [C.c_int, C.c_int, f32, f32, f32, f32, C.c_int] + [C.c_void_p] * 14
    l.ppo_terms_lr.argtypes, l.ppo_terms_lr.restype = [f32, f32, f32], f32
    l.ppo_terms_clip_scale.argtypes, l.ppo_terms_clip_scale.restype = [C.c_int, f32, f32], f32
    l.ppo_terms_adam_bias.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return l


def _np(t):
    return np.ascontiguousarray(t.detach().numpy(), np.float32)


def driver_minibatch(cfg, logstd, mu, act, omu, osg, adv, old_nlp, ret, old_v, v0, v1):
    arrs = [_np(x) for x in (logstd, mu, act, omu, osg, adv, old_nlp, ret, old_v, v0, v1)]
    rows, dmu, dls = np.zeros((MB, 8), np.float32), np.zeros((MB, A), np.float32), np.zeros(A, np.float32)
    lib().ppo_terms_minibatch(MB, A, cfg["e_clip"], cfg["critic_coef"], cfg["bounds_loss_coef"], cfg["entropy_coef"], int(cfg["clip_value"]),
                              *[x.ctypes.data_as(C.c_void_p) for x in arrs + [rows, dmu, dls]])
    return rows, dmu, dls


@functools.lru_cache(maxsize=None)
def walk(case):
    """the oracle's update of one mini-epoch, minibatch by minibatch; before each step the oracle's forward outputs of that minibatch, the
    autograd gradients of its losses with respect to them, and the driver's figures on the same inputs.  Computed once per case."""
    over = CASES[case]
    orc0, ds = BD.branch_dataset(N, MB, **over)
    orc = copy.deepcopy(orc0)
    c = orc.cfg
    work = {k: v.clone() for k, v in ds.items()}
    adv = orc.normalize_advantages(ds["returns"], ds["values"]) if c["normalize_advantage"] else ds["returns"] - ds["values"]
    steps, census, stats = [], dict(cv=[], ac=[]), dict(kl=[], lr_before=[], lr=[], gnorm=[], cv_gnorm=[])
    for i in range(ds["obs"].shape[0] // MB):
        sl = slice(i * MB, (i + 1) * MB)
        with torch.no_grad():
            rms = copy.deepcopy(orc.rms)                   # the central value sees the statistics that include its own minibatch
            if c["cv_normalize_input"]:
                rms.update(ds["states"][sl])
            vcv0 = orc.cv(rms(ds["states"][sl]) if c["cv_normalize_input"] else ds["states"][sl]).squeeze(-1)
            mu0, vc0 = orc.actor(ds["obs"][sl]), orc.critic(ds["obs"][sl]).squeeze(-1)
        mu, vc, vcv, ls = (x.detach().clone().requires_grad_(True) for x in (mu0, vc0, vcv0, orc.logstd))
        old_v, ret, omu, osg = work["values"][sl], work["returns"][sl], work["mus"][sl].clone(), work["sigmas"][sl].clone()
        sigma = torch.exp(ls).expand_as(mu)
        ratio = torch.exp(work["neglogp"][sl] - orc.neglogp(work["actions"][sl], mu, sigma, ls))
        a_loss = torch.max(-adv[sl] * ratio, -adv[sl] * torch.clamp(ratio, 1 - c["e_clip"], 1 + c["e_clip"]))
        c_loss, cv_loss = orc._critic_loss(old_v, vc, ret), orc._critic_loss(old_v, vcv, ret)
        b_loss = (torch.clamp_min(mu - 1.1, 0.0) ** 2 + torch.clamp_max(mu + 1.1, 0.0) ** 2).sum(-1)
        entropy = orc.entropy(ls)
        (orc.ac_loss(a_loss.mean(), c_loss.mean(), c["critic_coef"], entropy, c["entropy_coef"], b_loss.mean(), c["bounds_loss_coef"])
         + cv_loss.mean()).backward()
        with torch.no_grad():
            sg = sigma.detach()
            kl = (torch.log(osg / sg + 1e-5) + (sg ** 2 + (omu - mu) ** 2) / (2.0 * (osg ** 2 + 1e-5)) - 0.5).sum(-1)
            z2 = ((work["actions"][sl] - mu) / sg) ** 2
            dls_terms = ((adv[sl] * ratio).abs().unsqueeze(1) * (1.0 + z2)).sum(0) / MB      # what d loss / d logstd is the remainder of
        want = dict(a=a_loss, c=c_loss, cv=cv_loss, b=b_loss, kl=kl, entropy=entropy.expand(MB), dmu=mu.grad, dv0=vc.grad, dv1=vcv.grad, dls=ls.grad)
        rows, dmu, dls = driver_minibatch(c, ls, mu, work["actions"][sl], omu, osg, adv[sl], work["neglogp"][sl], ret, old_v, vc, vcv)
        got = dict(a=rows[:, 0], c=rows[:, 1], cv=rows[:, 2], b=rows[:, 3], kl=rows[:, 4], entropy=rows[:, 5], dv0=rows[:, 6], dv1=rows[:, 7],
                   dmu=dmu, dls=dls)
        stats["lr_before"].append(orc.lr)
        st = orc.update(work, only=[(0, i)])
        for k in ("kl", "lr", "gnorm", "cv_gnorm"):
            stats[k].append(st[k][0])
        stats["lr"][-1] = orc.lr                           # (st["lr"] is the rate the step used; orc.lr the one the rule left)
        # the walk's own forward pass is the one the oracle's step took
        np.testing.assert_allclose([float(a_loss.mean()), float(c_loss.mean()), float(cv_loss.mean()), float(kl.mean())],
                                   [st["a"][0], st["c"][0], st["cv"][0], st["kl"][0]], rtol=1e-6, atol=1e-7)
        for k in census:
            census[k] += st["census"][k]
        steps.append((got, {k: _np(v) for k, v in want.items()}, _np(dls_terms)))
    return dict(cfg=c, steps=steps, stats=stats, summary=census_summary(census), over=over)


def assert_branch_rich(w):
    bad = BD.census_violations(w["summary"], clip_value=bool(w["over"].get("clip_value", 1)), minibatch=MB)
    assert not bad, "the data of this case is not branch-rich and unambiguous on the oracle alone:\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("case", list(CASES))
def test_loss_terms_and_gradients_match_autograd(case):
    """surrogate, both value losses, bound loss, KL and entropy per row; d loss / d mu per (row, action), d loss / d v of both heads per row,
    d loss / d logstd (with the entropy term) per action: every minibatch of the mini-epoch.
    d loss / d logstd is what is left when the rows' terms gnlp (1 - z^2) / M cancel (clip_value_0, minibatch 12, action 9: -0.0078679 left
    of terms of 2.29, the driver 1.84e-6 away: 2.3e-4 of the remainder), and each term carries the relative error of the ratio
    exp(old neglogp - neglogp) of a neglogp near 30.  Its rtol 1e-5 is therefore taken of sum_rows |adv ratio| (1 + z^2) / M, formed from
    the oracle's values, not of the remainder; measured at most 0.51 of atol + that (every other quantity: at most 0.70 of its bound)."""
    w = walk(case)
    assert_branch_rich(w)
    scale = lambda k, want, terms: ATOL + RTOL * (terms if k == "dls" else np.abs(want[k]))
    worst = {}
    for got, want, terms in w["steps"]:
        for k in want:
            worst[k] = max(worst.get(k, 0.0), float(np.max(np.abs(got[k] - want[k]) / scale(k, want, terms))))
    print("figures", case, "max |got - want| / (atol + rtol |want|):", worst)
    for i, (got, want, terms) in enumerate(w["steps"]):
        for k in want:
            assert (np.abs(got[k] - want[k]) <= scale(k, want, terms)).all(), (k, "minibatch", i, got[k], want[k])
    assert any(np.abs(want["dmu"]).max() > 1e-3 for _, want, _ in w["steps"]) and any(np.abs(want["dv1"]).max() > 1e-2 for _, want, _ in w["steps"])


@pytest.mark.parametrize("case", list(CASES))
def test_step_rules_match_the_oracle(case):
    """the adaptive learning-rate rule chained over the run's recorded KL sequence, rate by rate to rtol 1e-6 (the branch tests' bound on the
    final rate); the clip scale on the recorded gradient norms of both optimisers against clip_grad_norm_ itself (the oracle's
    _clip_grads on a one-element gradient of that norm: the clipped element), rtol 1e-6: fewer than ten fp32 roundings of 6e-8 on either
    side.  That the norms lie on both sides of grad_norm, and the rates move both ways, is part of the census."""
    w = walk(case)
    assert_branch_rich(w)
    c, st = w["cfg"], w["stats"]
    lr = c["lr"]
    for kl, lr_before, lr_after in zip(st["kl"], st["lr_before"], st["lr"]):
        np.testing.assert_allclose(lr, lr_before, rtol=1e-6)
        lr = lib().ppo_terms_lr(lr, kl, c["kl_threshold"])
        np.testing.assert_allclose(lr, lr_after, rtol=1e-6)
    assert len(set(st["lr"])) > 3
    orc = BD.make_oracle(c)
    for truncate in (True, False):
        orc.cfg["truncate_grads"] = truncate
        for gn in st["gnorm"] + st["cv_gnorm"]:
            p = torch.nn.Parameter(torch.zeros(1))
            p.grad = torch.tensor([gn], dtype=torch.float32)
            orc._clip_grads([p])
            got = lib().ppo_terms_clip_scale(int(truncate), c["grad_norm"], gn)
            np.testing.assert_allclose(np.float32(got) * np.float32(gn), float(p.grad[0]), rtol=1e-6, atol=0)      # (a quiet step's norm can be 0)
            if not truncate or gn < 0.99 * c["grad_norm"]:
                assert got == 1.0
            elif gn > 1.01 * c["grad_norm"]:
                assert got < 1.0


def test_adam_bias_corrections_are_the_powf_form():
    """1 - beta^t for t = 1 .. 10240 (the step count of the shipped epoch): the header's pair equals, bit for bit, the plain restatement
    1.0f - powf(beta, (float)t) on the C library's powf, whose distance from 1 - beta**t in float64 is the bound the update has always had"""
    n = 10240
    bc1, bc2 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    lib().ppo_terms_adam_bias(1, n, bc1.ctypes.data_as(C.c_void_p), bc2.ctypes.data_as(C.c_void_p))
    libm = C.CDLL("libm.so.6")
    libm.powf.argtypes, libm.powf.restype = [f32, f32], f32
    t = np.arange(1, n + 1)
    for beta, got in ((0.9, bc1), (0.999, bc2)):
        plain = np.array([np.float32(1.0) - np.float32(libm.powf(beta, float(k))) for k in t], np.float32)
        exact = 1.0 - np.float64(beta) ** t
        bound = np.max(np.abs(plain.astype(np.float64) - exact) / exact)
        print("figures", beta, "max relative distance of the powf form from float64:", bound)
        assert (got.view(np.uint32) == plain.view(np.uint32)).all()
        assert np.max(np.abs(got.astype(np.float64) - exact) / exact) <= bound
