"""-m gpu: the persistent update kernel after its chain products moved from LDS read-backs to the gathered registers (forward L2,
backward L1) and the head-backward row halves of a column moved into one wave.  Three things could go wrong and
none of them shows as a crash: a barrier that was still needed (timing dependent results), an ownership index that one of prologue /
Adam / backward / epilogue did not follow (one layer's weights wrong), and a write-back that the next launch's prologue reads with
other indices (wrong from the second launch on).  The network shape is fixed by the kernel; the env count is what is small here
(n = 16: 160 optimiser steps per launch)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from helpers.persist_float64 import persistent_or_skip as _require_persistent  # noqa: E402
from test_gpu_fullsize_properties import _filled_agent  # noqa: E402
from test_gpu_ppo_parity import make_pair, rollout  # noqa: E402

N = 16
BITWISE = ("AC_PARAMS", "CV_PARAMS", "AC_ADAM_M", "AC_ADAM_V", "CV_ADAM_M", "CV_ADAM_V", "MB_MUS", "MB_SIGMAS")
# bounds of test_update_matches_autograd_adam (tests/test_gpu_ppo_parity.py) after one launch = 160 optimiser steps
BOUND_AC, BOUND_CV = 2e-4, 5e-4
# After the second launch (320 steps) no bound was known.  Measured on the commit before this change, same seeds, max |kernel - oracle|:
# adaptive_lr 0: actor-critic 1.0917e-05, central value 1.2156e-04; adaptive_lr 1 (the second launch runs at lr 3e-3): 1.3550e-04 / 1.2156e-04.
# The bound is twice the larger of the two: reordered sums move last bits; an index error moves a weight by whole Adam steps (lr 3e-4 .. 3e-3
# each).  This change keeps every sum's order: it measures the same figures.
PARENT_AC_320, PARENT_CV_320 = 1.3550e-04, 1.2156e-04
BOUND_AC_320, BOUND_CV_320 = 2.0 * PARENT_AC_320, 2.0 * PARENT_CV_320


def test_three_launches_bit_identical_on_two_handles():
    """same seed, same rollout, two handles, three launches each: every array the kernel writes, the learning rate and the KL sum
    equal bit for bit after each launch.  The exchange is tagged data and every LDS hand-over sits behind a barrier; a hand-over that
    lost its barrier gives results that depend on which wave ran first, and the two handles disagree."""
    a = _filled_agent(N, 9)
    b = _filled_agent(N, 9)
    try:
        _require_persistent(a)
        p0 = a.t["AC_PARAMS"].clone()
        for launch in range(3):
            a.update(); b.update()
            torch.cuda.synchronize()
            for k in BITWISE:
                np.testing.assert_array_equal(a.t[k].cpu().numpy(), b.t[k].cpu().numpy(), err_msg="launch %d %s" % (launch, k))
            ca, cb = a.ctrl(), b.ctrl()
            assert ca.ac_lr == cb.ac_lr and ca.sum_kl == cb.sum_kl, (launch, ca.ac_lr, cb.ac_lr, ca.sum_kl, cb.sum_kl)
            assert ca.ac_t == cb.ac_t == (launch + 1) * 5 * (N * 8 // 4)
        assert float((a.t["AC_PARAMS"] - p0).abs().max()) > 1e-4          # the launches did something
    finally:
        a.close(); b.close()


def _blocks(orc):
    """(name, array, offset, rows, cols) of the trunk's W1 and W2 of the three networks in the flat parameter arrays, walked in the
    order of PPOOracle.ac_flat / cv_flat"""
    out = []

    def walk(which, net, layers, o):
        for i, l in enumerate(layers):
            if i in (1, 2):
                out.append(("%s W%d" % (net, i), which, o, l.weight.shape[0], l.weight.shape[1]))
            o += l.weight.numel() + l.bias.numel()
        return o

    o = walk("ac", "actor", orc.actor.layers, 0)
    o += orc.actor.head.weight.numel() + orc.actor.head.bias.numel() + orc.logstd.numel()
    walk("ac", "critic", orc.critic.layers, o)
    walk("cv", "central value", orc.cv.layers, 0)
    return out


def second_launch_differences(adaptive):
    """one rollout, two launches on the same dataset beside two oracle updates: the flat parameters of both sides after each launch"""
    agent, orc = make_pair(N, adaptive_lr=adaptive)
    try:
        _require_persistent(agent)
        ds = rollout(agent, orc, N, torch.Generator().manual_seed(2))
        snaps = []
        for launch in range(2):
            agent.update()
            torch.cuda.synchronize()
            orc.update(ds)
            snaps.append(dict(ac=agent.t["AC_PARAMS"].cpu().numpy().copy(), cv=agent.t["CV_PARAMS"].cpu().numpy().copy(),
                              oac=orc.ac_flat().numpy().copy(), ocv=orc.cv_flat().numpy().copy(), lr=agent.ctrl().ac_lr, olr=orc.lr))
        return snaps, _blocks(orc)
    finally:
        agent.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["fixed_lr", "adaptive_lr"])
def launches(request):
    return second_launch_differences(request.param)


def test_trunk_w1_w2_of_every_network_against_the_oracle(launches):
    """after one launch, W1 and W2 of actor, critic and central value one by one: the column copy of W2 feeds backward L2 from other
    lanes than before, and a row or column copy read, updated or written with the wrong index shows in that block, by name"""
    snaps, blocks = launches
    s = snaps[0]
    assert len(blocks) == 6
    for name, which, o, rows, cols in blocks:
        got, want = s[which][o:o + rows * cols], s["o" + which][o:o + rows * cols]
        d = float(np.abs(got - want).max())
        print("%s [%d x %d]: max |kernel - oracle| %.3e" % (name, rows, cols, d))
        assert d < (BOUND_AC if which == "ac" else BOUND_CV), (name, d)
    np.testing.assert_allclose(s["lr"], s["olr"], rtol=1e-6)


def test_second_launch_reads_what_the_first_wrote_back(launches):
    """the epilogue of launch 1 and the prologue of launch 2 must use the same indices: all parameters after 320 optimiser steps.
    Measured before this change: see PARENT_AC_320 / PARENT_CV_320 above; allowed: twice that."""
    snaps, _ = launches
    s = snaps[1]
    d_ac, d_cv = float(np.abs(s["ac"] - s["oac"]).max()), float(np.abs(s["cv"] - s["ocv"]).max())
    print("after 320 steps: max |kernel - oracle| actor-critic %.3e (bound %.3e), central value %.3e (bound %.3e)"
          % (d_ac, BOUND_AC_320, d_cv, BOUND_CV_320))
    assert d_ac < BOUND_AC_320, d_ac
    assert d_cv < BOUND_CV_320, d_cv
    np.testing.assert_allclose(s["lr"], s["olr"], rtol=1e-6)
