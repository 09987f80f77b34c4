"""Shared bodies of the reset-draw tests (csrc/sdx_task.hip k_pre_physics and its task tails): what a reset draws
for itself when the caller passes no pile choice - the pile, InsertSim's plate yaw and harvest-ring slot, Search's lattice jitter and
target drop - against tests/helpers/device_rng.py, a numpy restatement of the draws.  tests/test_reset_draws.py runs them on the emulated
simulator (tests/hipemu), tests/test_gpu_reset_draws.py on the GPU.  A `backend` is (make, dev): make(n, **desc) builds a simulator,
dev(tensor) moves a host tensor to where its tensors live.

The step counter behind the draws has no tensor: it is advanced once per post-physics launch (k_tvalue's finalize branch), so `Counted`
counts its own step() / post_physics() calls.  Every case resets at step 0 and at two later counts."""
import numpy as np
import torch

from helpers import device_rng as R

SEED = 5
N = 32
K = 7                       # saved piles per brick type in these cases
KINDS = {"grasp": dict(), "orient": dict(task_kind=1), "insert": dict(task_kind=2, max_episode_length=125.0),
         "search": dict(task_kind=3, max_episode_length=75.0, act_moving_average=0.6, target_euler=[0.0, 3.14, 1.57])}
BRICK0, NBRICK, NFREE, PLATE = 9, 132, 72, 141      # SDX_ACTOR_BRICK0, SDX_NBRICK, SDX_NFREE, SDX_ACTOR_PLATE
f32 = np.float32


def host(t):
    return t.detach().cpu().numpy().copy()


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_within_ulps(got, want, ulps, what):
    """|got - want| <= ulps x the spacing of float32 at |want|"""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    tol = ulps * np.spacing(np.abs(want)).astype(np.float64)
    bad = ~(err <= tol)
    assert not bad.any(), "%s: %d of %d outside %g ulp, worst %g against %g at %s" % (
        what, int(bad.sum()), bad.size, ulps, float(err[bad].max()), float(tol[bad][err[bad].argmax()]), np.argwhere(bad)[0].tolist())


class Counted:
    """a simulator of N envs with K distinct saved piles per brick type, and the step counter kept by counting"""

    def __init__(self, backend, kind):
        self.make, self.dev = backend
        self.kind = kind
        self.s = self.make(N, seed=SEED, **KINDS[kind])
        self.steps = 0
        self.seg = np.array([self.s.scene.seg_index(e) for e in range(N)])
        lattice = host(self.s.ROOT.view(N, 142, 13))[0, BRICK0:BRICK0 + NBRICK]            # the default saved pile (K = 1)
        rng = np.random.default_rng(11)
        self.piles = np.tile(lattice[None, None], (8, K, 1, 1)).astype(f32)
        self.piles[:, :, :, 0:3] += rng.uniform(-0.01, 0.01, (8, K, NBRICK, 3)).astype(f32)
        self.piles[:, :, :, 7:13] = rng.uniform(-1.0, 1.0, (8, K, NBRICK, 6)).astype(f32)   # a restore zeroes the velocities
        self.s.load_initial_states(self.piles)
        self.choice = np.full(N, -1, np.int32)
        self.s.PILE_CHOICE.copy_(self.dev(torch.from_numpy(self.choice.copy())))
        self.zero_actions = self.dev(torch.zeros(N, 23))

    def close(self):
        self.s.close()

    def advance_to(self, count):
        """the first advance is a whole sdx_step, the rest post-physics launches alone; no env resets on the way"""
        while self.steps < count:
            self.s.RESET.zero_()
            if self.steps == 0:
                self.s.step(self.zero_actions)
            else:
                self.s.post_physics()
            self.steps += 1

    def reset(self, mask):
        """reset_idx(mask) with NO pile choice; returns (root before, root after) and holds PILE_CHOICE to the restatement"""
        before = host(self.s.ROOT.view(N, 142, 13))
        self.s.reset_idx(self.dev(torch.from_numpy(mask.astype(np.uint8))))
        after = host(self.s.ROOT.view(N, 142, 13))
        envs = np.flatnonzero(mask)
        self.choice[envs] = R.pile_choice(SEED, envs, self.steps, K)
        got = host(self.s.PILE_CHOICE)
        bad = np.flatnonzero(got != self.choice)
        assert bad.size == 0, "%s PILE_CHOICE at step %d: %d of %d entries differ, env %d holds %d against %d" % (
            self.kind, self.steps, bad.size, N, bad[0], got[bad[0]], self.choice[bad[0]])
        np.testing.assert_array_equal(bits(after[~mask]), bits(before[~mask]), err_msg="unmasked envs are untouched")
        return before, after

    def pile_of(self, e):
        return self.piles[e % 8, self.choice[e]]


def masks():
    """the env masks of a case's three reset events, each another set of envs; every env is reset at least once"""
    env = np.arange(N)
    return [env % 2 == 0, env % 3 != 1, env % 4 != 2]


# ------------------------------------------------------------------------------------------------------------------ 1. pile choice
def case_pile_choice(backend, kind, counts=(0, 1, 3)):
    """all four tasks: PILE_CHOICE of the masked envs is sdx_hash(seed, env, step) % K, the other envs keep their entry, and the bricks
    the tails leave alone are the chosen pile's, bit for bit, with zero velocities"""
    t = Counted(backend, kind)
    try:
        seen = set()
        for count, mask in zip(counts, masks()):
            t.advance_to(count)
            _, after = t.reset(mask)
            for e in np.flatnonzero(mask):
                pile, b = t.pile_of(e), after[e, BRICK0:BRICK0 + NBRICK]
                keep = np.ones(NBRICK, bool)
                if kind in ("insert", "search"):
                    keep[t.seg[e] - BRICK0] = False              # the target brick belongs to the task's reset tail
                if kind == "search":
                    keep[:NFREE] = False                         # ... and so do the free bricks' x and y (case_search)
                np.testing.assert_array_equal(bits(b[keep, 0:7]), bits(pile[keep, 0:7]), err_msg="env %d" % e)
                assert not b[keep, 7:13].any()
                seen.add(int(t.choice[e]))
        assert (t.choice >= 0).all() and len(seen) == K             # every env was drawn for, every pile was drawn
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------------------------ 2. InsertSim
def insert_counts():
    """step 0, step 1 and the first later step whose yaw differs from step 1's (there is one among 2..16)"""
    other = [s for s in range(2, 17) if R.insert_yaw_half(SEED, s) != R.insert_yaw_half(SEED, 1)]
    assert other, "the yaw must differ between some pair of steps in 1..16"
    return (0, 1, other[0])


def case_insert(backend):
    """the restored brick and hand are those of slot sdx_hash(seed ^ 0x5EED, env, step) % min(count, 5000) of the env's ring - ring
    fill counts 1, 5 and 5003 (above SDX_HARVEST_SLOTS - 1: the clamp) side by side -, the plate's yaw is the one draw of the event"""
    t = Counted(backend, "insert")
    try:
        s = t.s
        g = torch.Generator().manual_seed(1)
        slots = R.HARVEST_SLOTS
        obj = torch.randn(8, slots, 13, generator=g)
        hand = torch.randn(8, slots, 23, 2, generator=g) * 0.1
        s.HARVEST_OBJ.copy_(t.dev(obj))
        s.HARVEST_HAND.copy_(t.dev(hand))
        fill = np.array([1, 5, slots + 2, 5, 1, slots + 2, 5, slots - 1], np.int32)
        s.HARVEST_COUNT.copy_(t.dev(torch.from_numpy(fill.copy())))
        obj, hand = obj.numpy(), hand.numpy()
        yaws, picked = [], {1: set(), 5: set(), slots - 1: set(), slots + 2: set()}
        for count, mask in zip(insert_counts(), masks()):
            t.advance_to(count)
            _, after = t.reset(mask)
            envs = np.flatnonzero(mask)
            slot = R.insert_slot(SEED, envs, count, fill[envs % 8])
            dof = host(s.DOF.view(N, 23, 2))
            for e, j in zip(envs, slot):
                np.testing.assert_array_equal(bits(after[e, t.seg[e], 0:7]), bits(obj[e % 8, j, 0:7]), err_msg="env %d step %d" % (e, count))
                assert not after[e, t.seg[e], 7:13].any()
                np.testing.assert_array_equal(bits(dof[e, :, 0]), bits(hand[e % 8, j, :, 0]), err_msg="env %d step %d" % (e, count))
                assert not dof[e, :, 1].any()
                picked[int(fill[e % 8])].add(int(j))
            half = np.float64(R.insert_yaw_half(SEED, count))
            plate = after[envs, PLATE]
            assert_within_ulps(plate[:, 5], np.full(envs.size, f32(np.sin(half))), 1, "plate sin at step %d" % count)
            assert_within_ulps(plate[:, 6], np.full(envs.size, f32(np.cos(half))), 1, "plate cos at step %d" % count)
            assert (bits(plate) == bits(plate[0])).all()                  # one yaw for all envs of the event
            assert not plate[:, 3:5].any() and not plate[:, 7:13].any()
            yaws.append(float(plate[0, 5]))
        assert yaws[1] != yaws[2]                                         # the yaw is drawn per event
        assert picked[1] == {0} and len(picked[5]) > 2 and max(picked[slots + 2]) > 5 and max(picked[slots + 2]) < slots - 1
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------------------------ 3. Search
def assert_either_form(got, plain, contracted, what):
    """every stored value is within 1 ulp of the restated multiply-add in one of the two forms a compiler may give it: product and sum
    rounded one by one, or contracted into one rounding.  (Where the sum cancels - the target brick at r near -1 lands at x = 0.05 from
    0.25 - 0.2 - the two forms themselves are several ulp of the result apart: the product's rounding error, half an ulp of 0.2, is two
    ulp of 0.05.  The emulator build does not contract, hipcc does.)"""
    got, plain, contracted = (np.asarray(a, f32).astype(np.float64) for a in (got, plain, contracted))
    err = np.minimum(np.abs(got - plain) / np.spacing(np.abs(plain).astype(f32)), np.abs(got - contracted) / np.spacing(np.abs(contracted).astype(f32)))
    bad = ~(err <= 1.0)
    assert not bad.any(), "%s: %d of %d more than 1 ulp from both forms, worst %g ulp at %s" % (what, int(bad.sum()), bad.size, float(err[bad].max()), np.argwhere(bad)[0].tolist())
    return (got == plain).mean(), (got == contracted).mean()


def case_search(backend, counts=(0, 1, 3)):
    """x and y of every free brick = the chosen pile's value + the coordinate's own jitter, the target brick hangs at
    (0.25 + 0.2 r, 0.19 + 0.15 r, 0.9) with the one shared r; each within 1 ulp of the restated float32 value (the compiler may contract
    the multiply-add: assert_either_form); z, the quaternions and the fixed bricks are the pile's, bit for bit"""
    t = Counted(backend, "search")
    try:
        shares = []
        for count, mask in zip(counts, masks()):
            t.advance_to(count)
            _, after = t.reset(mask)
            envs = np.flatnonzero(mask)
            lattice = np.stack([t.pile_of(e)[:NFREE, 0:2].reshape(-1) for e in envs])
            xy = [R.search_jittered(SEED, envs, count, lattice, c).reshape(envs.size, NFREE, 2) for c in (False, True)]
            drop = [R.search_drop_pos(SEED, envs, count, c) for c in (False, True)]
            for k, e in enumerate(envs):
                pile, b = t.pile_of(e), after[e, BRICK0:BRICK0 + NBRICK]
                tb = t.seg[e] - BRICK0
                assert tb < NFREE
                free = np.ones(NFREE, bool)
                free[tb] = False
                shares.append(assert_either_form(b[:NFREE][free, 0:2], xy[0][k][free], xy[1][k][free], "env %d step %d free bricks" % (e, count)))
                np.testing.assert_array_equal(bits(b[:NFREE, 3:7]), bits(pile[:NFREE, 3:7]))
                np.testing.assert_array_equal(bits(b[:NFREE][free, 2]), bits(pile[:NFREE][free, 2]))
                assert not b[:, 7:13].any()
                assert_either_form(b[tb, 0:2], drop[0][k, 0:2], drop[1][k, 0:2], "env %d step %d target brick" % (e, count))
                assert b[tb, 2] == f32(0.9)
            jit = R.search_jitter(SEED, envs, count)
            assert np.abs(jit).max() > 0.019 and np.abs(jit).min() < 0.001                       # the jitter is there, over its whole range
        print("search jitter: share of values equal to the plain form %.3f, to the contracted form %.3f" % tuple(np.mean(shares, axis=0)))
    finally:
        t.close()
