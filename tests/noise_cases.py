"""Shared bodies of the observation / action noise tests (include/seqdex.h sdx_set_noise):
tests/test_observation_action_noise.py runs them on the emulated simulator (tests/hipemu), tests/test_gpu_observation_action_noise.py on
the GPU.  A `backend` is (make, dev): make(n, **desc) builds a simulator, dev(tensor) moves a host tensor to where its tensors live.
The expected values come from tests/helpers/noise_restatement.py, a numpy restatement of the definition."""
import numpy as np
import torch

from helpers import noise_restatement as nr
from seqdex_amd import _abi
from seqdex_amd import domain_randomization as dr

SEED = 22
KINDS = {"grasp": dict(), "orient": dict(task_kind=1), "insert": dict(task_kind=2, max_episode_length=125.0),
         "search": dict(task_kind=3, max_episode_length=75.0, act_moving_average=0.6, target_euler=[0.0, 3.14, 1.57])}
# observation columns the task never writes: zeros in SDX_T_OBS, so SDX_T_OBS_CLAMPED holds an additive operand itself
NEVER_WRITTEN = {"grasp": [131, 263, 395], "orient": list(range(62, 186)), "search": list(range(62, 186)), "insert": list(range(16, 23)) + [60]}
NEVER = 10 ** 9          # a frequency no run reaches: no refresh unless the test asks for one
STEPS = 40000            # schedule_steps of the shipped blocks

GAUSSIAN, UNIFORM, ADDITIVE, SCALING = nr.GAUSSIAN, nr.UNIFORM, nr.ADDITIVE, nr.SCALING
# (schedule, schedule_steps, frame): none, the middle of a linear ramp, a constant schedule past its step
SCHEDULES = {"none": (0, 0, 123), "linear-mid": (1, STEPS, STEPS // 2), "constant": (2, 300, 301)}


def attr(distribution, operation, rng, corr=(0.0, 0.0), schedule=0, steps=0):
    a = _abi.NoiseAttr()
    a.distribution, a.operation, a.schedule, a.schedule_steps = distribution, operation, schedule, steps
    a.range[0], a.range[1] = rng
    a.range_correlated[0], a.range_correlated[1] = corr
    return a


def blocks(distribution, operation, schedule="none"):
    """an (observations, actions, frame) case: spreads of the size of the shipped blocks, means that are not zero"""
    sc, steps, frame = SCHEDULES[schedule]
    if distribution == GAUSSIAN:
        o = attr(distribution, operation, (0.001, 0.002), (-0.0005, 0.001), sc, steps)
        a = attr(distribution, operation, (0.01, 0.05), (0.0, 0.015), sc, steps)
    else:
        o = attr(distribution, operation, (-0.002, 0.003), (0.0005, 0.0015), sc, steps)
        a = attr(distribution, operation, (-0.05, 0.04), (-0.01, 0.02), sc, steps)
    if operation == SCALING:            # factors around 1
        for b in (o, a):
            b.range[0] += 1.0
            b.range_correlated[0] += 1.0
            if distribution == UNIFORM:
                b.range[1] += 1.0
                b.range_correlated[1] += 1.0
    return o, a, frame


class Tracked:
    """a simulator plus the two counters of the noise that no tensor shows: the step counter (post-physics steps since create) and
    gravity's draw count (non-env randomizations since create)"""

    def __init__(self, backend, kind, n, **kw):
        self.make, self.dev = backend
        args = dict(KINDS[kind])
        args.update(kw)
        self.kind, self.n = kind, n
        self.s = self.make(n, seed=SEED, **args)
        self.steps, self.draws = 0, 0
        self.width = int(self.s.OBS.shape[1])

    def close(self):
        self.s.close()

    def randomize(self, frame, desc=None, frequency=NEVER):
        """randomization on at `frame` (as the sampler's tests set frames): SDX_T_DR_FRAME[1] = frame, one more non-env draw"""
        self.s.DR_FRAME[0] = frame
        self.s.set_randomization(desc if desc is not None else dr.identity_desc(frequency))
        self.draws += 1
        assert int(self.s.DR_FRAME[1]) == frame

    def frame1(self):
        return int(self.s.DR_FRAME[1])

    def step(self, acts):
        """one sdx_step; counts a refresh when SDX_T_DR_FRAME[1] moved"""
        before = self.frame1()
        self.s.step(acts)
        self.steps += 1
        if self.frame1() != before:
            self.draws += 1

    def pre_physics(self, acts):
        before = self.frame1()
        self.s.pre_physics(acts)
        if self.frame1() != before:
            self.draws += 1

    def post_physics(self):
        self.s.post_physics()
        self.steps += 1

    def want_actions(self, a, acts_host, draws, steps, frame):
        o, b = nr.operand(a, SEED, "actions", self.n, 23, draws, steps, frame)
        return nr.apply(a, acts_host, o, b, float(self.s._desc.clip_actions), "actions", frame) + (o, b)

    def want_obs(self, a, draws, steps, frame):
        o, b = nr.operand(a, SEED, "observations", self.n, self.width, draws, steps, frame)
        return nr.apply(a, host(self.s.OBS), o, b, float(self.s._desc.clip_obs), "observations", frame) + (o, b)


def host(t):
    return t.detach().cpu().numpy().copy()


def assert_within(got, want, tol, what):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bad = ~(err <= tol)
    assert not bad.any(), "%s: %d of %d outside the bound, worst %g against %g at %s" % (
        what, int(bad.sum()), bad.size, float(err[bad].max()), float(tol[bad][err[bad].argmax()]), np.argwhere(bad)[0].tolist())


# ------------------------------------------------------------------------------------------------------------------ 1. known operand
def case_known_operand(t, distribution, operation, schedule):
    """one sdx_step with both blocks on: SDX_T_ACTIONS and SDX_T_OBS_CLAMPED against the restatement.  The action is 0 (additive: ACTIONS is
    the operand itself) or 1 (scaling: 1 x operand); on a task's never-written observation columns OBS_CLAMPED is the additive operand."""
    o_attr, a_attr, frame = blocks(distribution, operation, schedule)
    t.randomize(frame)
    t.s.set_noise(observations=o_attr, actions=a_attr)
    acts_host = np.full((t.n, 23), 0.0 if operation == ADDITIVE else 1.0, np.float32)
    acts = t.dev(torch.from_numpy(acts_host.copy()))
    draws, steps = t.draws, t.steps
    t.step(acts)
    assert t.draws == draws, "no refresh in this step (frequency NEVER)"
    assert t.frame1() == frame
    what = "%s dist %d op %d %s" % (t.kind, distribution, operation, schedule)
    # actions: the counters in force before the step
    want, tol, op, bound = t.want_actions(a_attr, acts_host, draws, steps, frame)
    got = host(t.s.ACTIONS)
    # tolerance (helpers/noise_restatement.py): each gaussian draw may be off by 2 ulp of itself (the sampler's bound; a uniform white draw
    # is exact), the sum corr + white rounds once more (1 ulp of the operand, counted only when a draw moved), then one rounding per
    # following operation: x + o or x * o (1 ulp of the result; none where x = 0 and the block is additive, the sum IS the operand then)
    assert_within(got, want, tol, what + " ACTIONS")
    np.testing.assert_array_equal(host(acts), acts_host, err_msg="the caller's action buffer is only read")
    assert np.abs(op).max() > 0 and (op != op[0, 0]).any()
    if operation == ADDITIVE:
        assert (tol == bound).all()                                   # zero action: exactly the operand, up to the draws' own bound
    # observations: the counters after the step (the step counter includes this step)
    want, tol, op, bound = t.want_obs(o_attr, draws, steps + 1, frame)
    got = host(t.s.OBS_CLAMPED)
    assert_within(got, want, tol, what + " OBS_CLAMPED")
    nw = NEVER_WRITTEN[t.kind]
    clean = host(t.s.OBS)
    assert (clean[:, nw] == 0).all()
    if operation == ADDITIVE:
        assert (tol[:, nw] == bound[:, nw]).all() and np.abs(got[:, nw]).min() > 0
    assert (clean[:, [c for c in range(t.width) if c not in nw]] != 0).any()        # written columns took part
    return got


# ------------------------------------------------------------------------------------------------------------------ 2. zero / isolation
WATCH = ("ROOT", "DOF", "OBS", "OBS_CLAMPED", "STATES", "ACTIONS", "REW")


def fixed_actions(n, steps, seed=5):
    g = torch.Generator().manual_seed(seed)
    acts = [(torch.rand(n, 23, generator=g) * 3 - 1.5) for _ in range(steps)]      # some outside the +-1 clamp
    acts[0][0, 0] = -0.0
    acts[0][0, 1] = 0.0
    return acts


def run(t, acts, names=WATCH):
    out = []
    for a in acts:
        t.step(t.dev(a.clone()))
        out.append({k: host(t.s.tensor(k)) for k in names})
    return out


def assert_same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape
    np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b,
                                  err_msg=what)


def case_zero_operand(backend, kind, n, params, base=None, steps=3):
    """frame 0 of the shipped linear schedule: every scaled number is zero, three steps are bit-identical to noise off"""
    acts = fixed_actions(n, steps)
    if base is None:
        off = Tracked(backend, kind, n)
        try:
            off.randomize(0)
            base = run(off, acts)
        finally:
            off.close()
    on = Tracked(backend, kind, n)
    try:
        on.randomize(0)
        rep = on.s.set_noise(params)
        assert set(rep) == {"observations", "actions"}
        got = run(on, acts)
    finally:
        on.close()
    for i in range(steps):
        for k in ("ROOT", "DOF", "OBS", "OBS_CLAMPED", "ACTIONS", "REW"):
            assert_same_bits(got[i][k], base[i][k], "step %d %s" % (i, k))
    assert np.signbit(got[0]["ACTIONS"][0, 0]) and not np.signbit(got[0]["ACTIONS"][0, 1])        # the negative zero survived


def case_isolation(backend, kind, n, steps, base=None, extra=()):
    """observation noise only, fixed actions: everything but SDX_T_OBS_CLAMPED is bit-identical to noise off"""
    acts = fixed_actions(n, steps)
    names = WATCH + tuple(extra)
    if base is None:
        off = Tracked(backend, kind, n)
        try:
            off.randomize(50000)
            base = run(off, acts, names)
        finally:
            off.close()
    on = Tracked(backend, kind, n)
    try:
        on.randomize(50000)
        on.s.set_noise(observations=attr(GAUSSIAN, ADDITIVE, (0.0, 0.002), (0.0, 0.001), 1, STEPS))
        got = run(on, acts, names)
    finally:
        on.close()
    for i in range(steps):
        for k in names:
            if k != "OBS_CLAMPED":
                assert_same_bits(got[i][k], base[i][k], "step %d %s" % (i, k))
        assert (got[i]["OBS_CLAMPED"] != base[i]["OBS_CLAMPED"]).mean() > 0.9
    return base


# ------------------------------------------------------------------------------------------------------------------ 3. correlation, refresh
def case_refresh(backend, n, gravity):
    """white part zero: the operand is the correlated part, equal step over step; it changes exactly at a reset with
    frame - last >= frequency - with gravity randomized or not - and not at an earlier reset.  sdx_pre_physics / sdx_post_physics only."""
    t = Tracked(backend, "grasp", n)
    try:
        d = dr.identity_desc(3)
        if gravity:
            d.gravity.distribution, d.gravity.operation = GAUSSIAN, ADDITIVE
            d.gravity.range[0], d.gravity.range[1] = 0.0, 0.4
        t.randomize(40000, d)
        a_attr = attr(GAUSSIAN, ADDITIVE, (0.0, 0.0), (0.0, 0.015))
        o_attr = attr(UNIFORM, ADDITIVE, (0.0, 0.0), (0.001, 0.002))
        t.s.set_noise(observations=o_attr, actions=a_attr)
        zeros = t.dev(torch.zeros(n, 23))
        last, prev_a, prev_o = 40000, None, None
        col = NEVER_WRITTEN["grasp"][0]
        # (frame, reset flags): an early reset (1 < 3 frames after the last refresh), no reset, a due reset, an early one, a due one
        for frame, reset in ((40001, [1] + [0] * (n - 1)), (40002, [0] * n), (40004, [0, 1] + [0] * (n - 2)), (40005, [1] * n), (40007, [0] * (n - 1) + [1])):
            t.s.DR_FRAME[0] = frame
            t.s.RESET[:] = t.dev(torch.tensor(reset))
            draws = t.draws
            t.pre_physics(zeros)
            due = any(reset) and frame - last >= 3
            assert t.draws == draws + (1 if due else 0), (frame, reset)
            if due:
                last = frame
            assert t.frame1() == last
            # the actions were noised before this call's re-sampling: the draw count in force until now
            want, tol, _, _ = t.want_actions(a_attr, np.zeros((n, 23), np.float32), draws, t.steps, last)
            got_a = host(t.s.ACTIONS)
            assert_within(got_a, want, tol, "ACTIONS at frame %d" % frame)      # tol = 2 ulp of the draw: white is exactly 0, x = 0
            t.post_physics()
            want, tol, _, _ = t.want_obs(o_attr, t.draws, t.steps, last)         # ... the observations after it
            got_o = host(t.s.OBS_CLAMPED)[:, col]
            assert_within(got_o, want[:, col], tol[:, col], "OBS_CLAMPED at frame %d" % frame)
            if prev_a is not None:
                assert (got_a == prev_a).all() == (draws == prev_draws), frame
                assert (got_o == prev_o).all() == (not due), frame
            prev_a, prev_o, prev_draws = got_a, got_o, draws
    finally:
        t.close()


def case_actions_not_reclamped(backend, n):
    t = Tracked(backend, "grasp", n)
    try:
        assert float(t.s._desc.clip_actions) == 1.0
        t.randomize(50000)
        a_attr = attr(GAUSSIAN, ADDITIVE, (0.0, 0.05), (0.0, 0.015))
        t.s.set_noise(actions=a_attr)
        acts_host = np.full((n, 23), 1.0, np.float32)
        acts_host[:, 0] = 7.5                                                     # clamped to 1 first, then noised
        acts = t.dev(torch.from_numpy(acts_host.copy()))
        t.pre_physics(acts)
        want, tol, op, _ = t.want_actions(a_attr, acts_host, t.draws, t.steps, 50000)
        got = host(t.s.ACTIONS)
        assert_within(got, want, tol, "ACTIONS")
        assert (op > 1e-4).any() and (got[op > 1e-4] > 1.0).all()
        np.testing.assert_array_equal(host(acts), acts_host, err_msg="the caller's buffer")
    finally:
        t.close()


def case_independent_of_n(backend, n_small, n_large):
    out = []
    for n in (n_small, n_large):
        t = Tracked(backend, "grasp", n)
        try:
            t.randomize(50000)
            t.s.set_noise(observations=attr(GAUSSIAN, ADDITIVE, (0.0, 0.002), (0.0, 0.001)), actions=attr(UNIFORM, SCALING, (0.9, 1.1), (1.0, 1.02)))
            t.s.RESET.zero_()
            t.pre_physics(t.dev(torch.ones(n, 23)))
            t.post_physics()
            out.append((host(t.s.ACTIONS)[:n_small], host(t.s.OBS_CLAMPED)[:n_small]))
        finally:
            t.close()
    assert_same_bits(out[0][0], out[1][0], "ACTIONS")
    assert_same_bits(out[0][1], out[1][1], "OBS_CLAMPED")


def case_snapshot(backend, n, params):
    """save_all, three steps (the second one with a refresh), restore_all, the same three steps: the noise repeats bit for bit"""
    t = Tracked(backend, "grasp", n)
    try:
        p = dict(params)
        p["frequency"] = 1
        t.s.DR_FRAME[0] = 50000
        t.s.set_randomization(p)
        t.s.set_noise(p)
        acts = fixed_actions(n, 4, seed=9)
        t.step(t.dev(acts[3]))
        st = t.s.snapshot()
        st.save()

        def three():
            out = []
            for i in range(3):
                if i == 1:
                    t.s.RESET[:] = 1
                    t.s.RANDOMIZE[:] = 5
                f1 = t.frame1()
                t.step(t.dev(acts[i]))
                out.append((host(t.s.OBS_CLAMPED), host(t.s.ACTIONS), t.frame1() != f1))
            return out
        first = three()
        st.restore()
        second = three()
        assert [r[2] for r in first] == [False, True, False] == [r[2] for r in second]
        for i in range(3):
            assert_same_bits(first[i][0], second[i][0], "OBS_CLAMPED step %d" % i)
            assert_same_bits(first[i][1], second[i][1], "ACTIONS step %d" % i)
        assert (first[0][0] != first[2][0]).mean() > 0.9
    finally:
        t.close()
