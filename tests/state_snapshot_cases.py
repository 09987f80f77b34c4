"""Shared bodies of the sim-snapshot tests (include/seqdex.h sdx_state_*): tests/test_state_snapshot.py runs them on
the emulated simulator (tests/hipemu), tests/test_gpu_state_snapshot.py on the GPU.  A `backend` is (make, dev): make(n, **desc) builds a
simulator, dev(tensor) moves a host tensor to where the simulator's tensors live.  Every comparison is exact (NaN-aware)."""
import copy
import os

import numpy as np
import pytest
import torch
import yaml

from seqdex_amd import _abi
from seqdex_amd.sim import SdxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXC = 1536

# tensors of _abi.T by their part in a snapshot.  ENV: [N, ...] rows of an env row (ROOT / DOF: N * 142 / N * 23 rows); GLOBAL: only save_all /
# restore_all move them; EXCLUDED: logs and diagnostics, never touched.  The warm-start rows are state up to WARM_COUNT.
ENV = ["ROOT", "DOF", "RB", "CONTACT", "JAC_EEF", "TARGETS", "PREV_TARGETS", "OBS", "STATES", "OBS_CLAMPED", "STATES_CLAMPED", "REW", "RESET",
       "PROGRESS", "RANDOMIZE", "ACTIONS", "INIT_POS", "INIT_ROT", "SUCCESSES", "META_REW", "FINGER_DIST", "TVALUE", "ARM_CONTACTS",
       "STUDENT_OBS", "SUCCESS_BUF", "PILE_CHOICE", "NCONTACTS", "INSERT_AUX", "SEG_PIXELS", "EMERGENCE", "JACOBIAN", "WARM_COUNT", "CAM_ROT",
       "DR_DOF", "DR_LINK", "DR_BRICK"]
ENV_SEARCH = ["SEG_IMAGE", "TVALUE_OBS"]
WARM = ["WARM_KEYS", "WARM_LAMBDA"]
GLOBAL = ["CONS_SUCCESSES", "DR_GRAVITY", "DR_FRAME"]
EXCLUDED = ["DEBUG", "HARVEST_HAND", "HARVEST_OBJ", "HARVEST_COUNT", "TV_SUCCESS", "TV_FAILURE", "TV_COUNT", "PILE_HARVEST", "PILE_HARVEST_COUNT",
            "CONTACT_STATS", "TV_KEYS", "HARVEST_KEYS", "PILE_HARVEST_KEYS"]
assert sorted(ENV + ENV_SEARCH + WARM + GLOBAL + EXCLUDED) == sorted(_abi.T)      # every tensor id is classified

KINDS = {"grasp": dict(), "orient": dict(task_kind=1), "insert": dict(task_kind=2, max_episode_length=125.0),
         "search": dict(task_kind=3, max_episode_length=75.0, act_moving_average=0.6, target_euler=[0.0, 3.14, 1.57])}


def env_names(s):
    names = list(ENV)
    if s._desc.task_kind == _abi.TASK_SEARCH:
        names += ENV_SEARCH
    return names


def has_warm(s):
    return s._desc.warm_start > 0.0


def per_env(s, name, t=None):
    t = s.tensor(name) if t is None else t
    return t.reshape(s.num_envs, -1)


def record(s):
    """host copies of every tensor that is state"""
    r = {k: s.tensor(k).detach().cpu().clone() for k in env_names(s) + GLOBAL}
    if has_warm(s):
        for k in WARM:
            r[k] = s.tensor(k).detach().cpu().clone()
    return r


def _eq(a, b, msg):
    np.testing.assert_array_equal(a.numpy(), b.numpy(), err_msg=msg)      # (NaN == NaN for assert_array_equal)


def assert_envs_equal(s, ra, ea, rb, eb, what=""):
    """env ea[i] of record ra equals env eb[i] of record rb in every per-env tensor (the warm-start rows up to the count)"""
    n = s.num_envs
    for k in env_names(s):
        _eq(ra[k].reshape(n, -1)[ea], rb[k].reshape(n, -1)[eb], "%s %s" % (what, k))
    if "WARM_KEYS" in ra:
        for a, b in zip(ea, eb):
            c = int(ra["WARM_COUNT"][a])
            _eq(ra["WARM_KEYS"][a, :c], rb["WARM_KEYS"][b, :c], "%s WARM_KEYS env %d" % (what, a))
            _eq(ra["WARM_LAMBDA"][a, :, :c], rb["WARM_LAMBDA"][b, :, :c], "%s WARM_LAMBDA env %d" % (what, a))


def assert_records_equal(s, ra, rb, what="", with_global=True):
    e = list(range(s.num_envs))
    assert_envs_equal(s, ra, e, rb, e, what)
    if with_global:
        for k in GLOBAL:
            _eq(ra[k], rb[k], "%s %s" % (what, k))


def assert_untouched(s, before, envs=None, what=""):
    """the listed envs (default: all) hold exactly what `before` recorded, the whole warm-start rows included"""
    now = record(s)
    e = list(range(s.num_envs)) if envs is None else list(envs)
    n = s.num_envs
    for k in env_names(s) + (WARM if has_warm(s) else []):
        _eq(now[k].reshape(n, -1)[e], before[k].reshape(n, -1)[e], "%s %s" % (what, k))


def poison(s, names):
    for k in names:
        t = s.tensor(k)
        if t.dtype.is_floating_point:
            t.fill_(-12345.678)
        else:
            t.fill_(0x5A5A if t.dtype == torch.int16 else 0x5A5A5A5A)


def tiled_state(golden_dir, n):
    """the settled P1 piles tiled over n envs, every env with its own finger targets and arm velocities"""
    st = np.load(os.path.join(golden_dir, "P1_settled_state.npz"))
    m = st["root"].shape[0]
    reps = (n + m - 1) // m
    root = np.tile(st["root"], (reps, 1, 1))[:n].copy()
    dof = np.tile(st["dof"], (reps, 1, 1))[:n].copy()
    tg = np.tile(st["targets"], (reps, 1))[:n].copy()
    rng = np.random.default_rng(7)
    tg[:, 7:] += rng.uniform(-0.05, 0.05, (n, 16)).astype(np.float32)
    dof[:, :7, 1] += rng.uniform(-0.2, 0.2, (n, 7)).astype(np.float32)
    return root, dof, tg


def actions(n, steps, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, 23, generator=g) * 2 - 1) for _ in range(steps)]


def make_scene_sim(backend, golden_dir, n, kind="grasp", steps=2, **kw):
    """a simulator in a contact-rich state: saved piles loaded, the P1 state copied in, no env about to reset, `steps` steps taken"""
    make, dev = backend
    args = dict(KINDS[kind])
    args.update(kw)
    s = make(n, seed=22, **args)
    s.load_initial_states(np.load(os.path.join(golden_dir, "F8_reset_idx.npz"))["piles"])
    root, dof, tg = tiled_state(golden_dir, n)
    s.ROOT.copy_(dev(torch.from_numpy(root.reshape(-1, 13))))
    s.DOF.copy_(dev(torch.from_numpy(dof.reshape(-1, 2))))
    s.TARGETS.copy_(dev(torch.from_numpy(tg)))
    s.PREV_TARGETS.copy_(dev(torch.from_numpy(tg)))
    s.WARM_COUNT.zero_()
    s.RESET.zero_()                      # (sdx_create sets every flag: the first step would put every env back onto a saved pile)
    s.refresh_kinematics()
    for a in actions(n, steps, seed=3):
        s.step(dev(a))
    return s


def run(s, dev, acts):
    out = []
    for a in acts:
        s.step(dev(a))
        out.append(record(s))
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. completeness
def case_poison(backend, golden_dir, n):
    s = make_scene_sim(backend, golden_dir, n)
    try:
        st = s.snapshot()
        st.save()
        saved = record(s)
        assert int(saved["WARM_COUNT"].min()) > 100 and int(saved["NCONTACTS"].max()) < MAXC      # contact-rich, a cache to carry
        state = env_names(s) + GLOBAL + WARM
        other = [k for k in EXCLUDED]
        poison(s, state + other)
        garbage = {k: s.tensor(k).detach().cpu().clone() for k in other + WARM}
        st.restore()
        assert_records_equal(s, saved, record(s), "restore_all")
        for k in other:                                                      # not part of any snapshot
            _eq(s.tensor(k).detach().cpu(), garbage[k], "excluded " + k)
        now = record(s)
        for e in range(n):                                                   # behind the warm count nothing is written
            c = int(saved["WARM_COUNT"][e])
            _eq(now["WARM_KEYS"][e, c:], garbage["WARM_KEYS"][e, c:], "WARM_KEYS tail")
            _eq(now["WARM_LAMBDA"][e, :, c:], garbage["WARM_LAMBDA"][e, :, c:], "WARM_LAMBDA tail")
        assert s.state_stats() == [0, 0, 0]
        st.close()
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 2. replay
def case_replay(backend, golden_dir, n, kind="grasp", resets=False, randomize=False):
    make, dev = backend
    s = make_scene_sim(backend, golden_dir, n, kind)
    try:
        if kind == "search":
            s.render_segmentation()                                          # the image and the pixel statistics hold something
        if randomize:
            p = copy.deepcopy(yaml.safe_load(open(os.path.join(ROOT, "seqdex_amd", "cfg", "allegro_hand_block_assembly_grasp_sim.yaml")))
                              ["task"]["randomization_params"])
            p["frequency"] = 1
            s.DR_FRAME[0] = 40000                                            # past every schedule: full-strength samples
            s.set_randomization(p)
            s.step(dev(actions(n, 1, seed=9)[0]))
        half = list(range(0, n, 2))
        if resets:                                                           # about half the envs run out of time inside the window
            s.PROGRESS[half] = int(s._desc.max_episode_length) - 2
            if randomize:
                s.RANDOMIZE[half] = 5
        st = s.snapshot()
        st.save()
        saved = record(s)
        acts = actions(n, 3)
        first = run(s, dev, acts)
        if resets:
            assert bool((first[-1]["PROGRESS"][half] < 3).all()) and bool((first[-1]["PROGRESS"][1::2] > 3).all())      # a reset happened
            if randomize:                                                    # ... and re-sampled the env's rows
                assert bool((first[-1]["DR_DOF"][half] != saved["DR_DOF"][half]).any())
                assert bool((first[-1]["RANDOMIZE"][half] < 5).all())
        assert not torch.equal(first[-1]["DOF"], saved["DOF"])
        poison(s, env_names(s))
        st.restore()
        assert_records_equal(s, saved, record(s), "restore_all")
        second = run(s, dev, acts)
        for i, (a, b) in enumerate(zip(first, second)):
            assert_records_equal(s, a, b, "replay step %d" % i)
        st.close()
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 3. rows and clones
def case_rows(backend, golden_dir, n, use_clone):
    make, dev = backend
    s = make_scene_sim(backend, golden_dir, n)
    try:
        before = record(s)
        if use_clone:
            src, dst = [0, 0, 1], [8, 16, 9]
            s.clone_envs(src, dst)
        else:
            src, dst = [0, 1], [24, 9]
            st = s.snapshot(rows=6)
            st.save([0, 1, 2], [5, 0, 3])
            st.restore([5, 0], dst)
        now = record(s)
        assert_envs_equal(s, now, dst, before, src, "copied")
        assert_untouched(s, before, [e for e in range(n) if e not in dst], "other envs")
        acts = actions(n, 3)
        for a in acts:
            for x, y in zip(src, dst):
                a[y] = a[x]
        for i, r in enumerate(run(s, dev, acts)):
            assert_envs_equal(s, r, dst, r, src, "step %d" % i)
            assert not torch.equal(per_env(s, "DOF", r["DOF"])[0], per_env(s, "DOF", before["DOF"])[0])
        assert s.state_stats() == [0, 0, 0]
        if not use_clone:
            st.close()
    finally:
        s.close()


def dst_of(e, n):
    """an env of e's class other than e (a permutation of the envs for n >= 16)"""
    return e + 8 if e + 8 < n else e % 8


def case_list_lengths(backend, golden_dir, s, count):
    """save `count` envs into permuted rows, poison, restore each row into another env of its class: copy only, no step"""
    make, dev = backend
    n = s.num_envs
    envs = list(range(count))
    rows = [(7 * i + 3) % n for i in range(count)]
    dst = [dst_of(e, n) for e in envs]
    before = record(s)
    st = s.snapshot()
    try:
        ids = lambda v: dev(torch.tensor(v, dtype=torch.int32))      # noqa: E731  (device tensors: the unchecked path)
        st.save(ids(envs), ids(rows))
        poison(s, [k for k in env_names(s) if k != "WARM_COUNT"])
        s.WARM_COUNT.zero_()
        garbage = record(s)
        st.restore(ids(rows), ids(dst))
        now = record(s)
        assert_envs_equal(s, now, dst, before, envs, "restored")
        assert_untouched(s, garbage, [e for e in range(n) if e not in dst], "other envs")
        assert s.state_stats() == [0, 0, 0]
    finally:
        s.WARM_COUNT.zero_()
        for k in env_names(s):                                        # leave the shared simulator as it was
            s.tensor(k).copy_(dev(before[k]))
        if has_warm(s):
            for k in WARM:
                s.tensor(k).copy_(dev(before[k]))
        st.close()


# ------------------------------------------------------------------------------------------------------------------ 4. skips
def case_skips(backend, golden_dir, s):
    make, dev = backend
    n = s.num_envs
    ids = lambda v: dev(torch.tensor(v, dtype=torch.int32))          # noqa: E731
    before = record(s)
    st = s.snapshot(rows=4)
    try:
        assert s.state_stats() == [0, 0, 0]
        s.clone_envs(ids([2]), ids([3]))                              # another target brick
        assert s.state_stats() == [0, 1, 0]
        s.clone_envs(ids([-1, 0, n, 1]), ids([7, n, 15, -1]))
        assert s.state_stats() == [4, 1, 0]
        st.restore(ids([1]), ids([1]))                                # row 1 was never saved
        assert s.state_stats() == [4, 1, 1]
        st.save(ids([2, -1, n, 4]), ids([0, 1, 2, 4]))                # only env 2 -> row 0 is in range
        assert s.state_stats() == [7, 1, 1]
        st.restore(ids([0, 0, 1, 4, -1]), ids([3, n, 9, 2, 2]))       # class mismatch, env out of range, never saved, two rows out of range
        assert s.state_stats() == [10, 2, 2]
        assert_untouched(s, before, None, "after skipped entries")
        for k in GLOBAL:
            _eq(s.tensor(k).detach().cpu(), before[k], k)
        # the same kinds as host lists: refused before anything is launched
        st2 = s.snapshot(rows=4)
        st2.save([2], [0])
        for bad in (lambda: s.clone_envs([2], [3]), lambda: s.clone_envs([-1], [7]), lambda: s.clone_envs([0], [n]),
                    lambda: s.clone_envs([0, 0], [8, 8]), lambda: s.clone_envs([0, 8], [8, 16]), lambda: s.clone_envs([0, 1], [8]),
                    lambda: st2.restore([1], [1]), lambda: st2.restore([0], [3]), lambda: st2.restore([4], [2]), lambda: st2.restore([0, 0], [2, 2]),
                    lambda: st2.save([n], [0]), lambda: st2.save([0, 1], [2, 2]), lambda: st2.save([0], [4]), lambda: s.same_class_envs(n)):
            with pytest.raises(ValueError):
                bad()
        st2.close()
        assert s.state_stats() == [10, 2, 2]
        assert_untouched(s, before, None, "after refused lists")
        assert s.same_class_envs(2) == [e for e in range(n) if e % 8 == 2]
    finally:
        st.close()


# ------------------------------------------------------------------------------------------------------------------ 5. warm-cache edges
def _pattern(s, dev, seed):
    n = s.num_envs
    g = torch.Generator().manual_seed(seed)
    s.WARM_KEYS.copy_(dev(torch.randint(0, 2 ** 31 - 1, (n, MAXC), generator=g, dtype=torch.int32)))
    s.WARM_LAMBDA.copy_(dev(torch.rand(n, 3, MAXC, generator=g)))


def case_warm_edges(backend, s, counts):
    """copy only: the first `count` keys and impulses arrive (clone 0 -> 8, save 1 / restore -> 9), the rest of the destination stays"""
    make, dev = backend
    st = s.snapshot(rows=1)
    try:
        for i, c in enumerate(counts):
            _pattern(s, dev, 100 + i)
            s.WARM_COUNT.fill_(7)
            s.WARM_COUNT[0] = c
            s.WARM_COUNT[1] = c
            before = record(s)
            s.clone_envs([0], [8])
            st.save([1], [0])
            st.restore([0], [9])
            now = record(s)
            k = min(max(c, 0), MAXC)
            for a, b in ((0, 8), (1, 9)):
                assert int(now["WARM_COUNT"][b]) == k, (c, b)
                _eq(now["WARM_KEYS"][b, :k], before["WARM_KEYS"][a, :k], "keys %d" % c)
                _eq(now["WARM_LAMBDA"][b, :, :k], before["WARM_LAMBDA"][a, :, :k], "impulses %d" % c)
                _eq(now["WARM_KEYS"][b, k:], before["WARM_KEYS"][b, k:], "keys behind %d" % c)
                _eq(now["WARM_LAMBDA"][b, :, k:], before["WARM_LAMBDA"][b, :, k:], "impulses behind %d" % c)
            others = [e for e in range(s.num_envs) if e not in (8, 9)]
            for name in WARM + ["WARM_COUNT"]:
                _eq(per_env(s, name, now[name])[others], per_env(s, name, before[name])[others], "%s of other envs, count %d" % (name, c))
    finally:
        st.close()


# ------------------------------------------------------------------------------------------------------------------ 6. across handles
def case_across_handles(backend, golden_dir, n_big, n_small):
    make, dev = backend
    a = make_scene_sim(backend, golden_dir, n_big)
    b = make_scene_sim(backend, golden_dir, n_small)
    c = None
    try:
        envs = list(range(n_small))
        st = a.snapshot(rows=n_small)
        with pytest.raises(SdxError, match="error -4"):               # SDX_ERR_STATE: nothing saved yet, so the last save was no save_all
            st.restore()
        st.save(envs)
        with pytest.raises(SdxError, match="error -4"):
            st.restore()
        poison(b, [k for k in env_names(b) if k != "WARM_COUNT"])
        st.restore(envs, envs, sim=b)
        ra, rb = record(a), record(b)
        for k in env_names(a):
            _eq(per_env(b, k, rb[k]), per_env(a, k, ra[k])[:n_small], "restored into the small simulator: " + k)
        acts = actions(n_big, 3)
        for i, x in enumerate(acts):
            a.step(dev(x))
            b.step(dev(x[:n_small].clone()))
            ra, rb = record(a), record(b)
            for k in env_names(a):
                _eq(per_env(b, k, rb[k]), per_env(a, k, ra[k])[:n_small], "step %d %s" % (i, k))
        # a full snapshot only goes back into a simulator with as many envs; another layout is refused outright
        full = a.snapshot()
        full.save()
        with pytest.raises(SdxError, match="error -1"):               # SDX_ERR_INVALID: 26 envs' global state into 10 envs
            st2 = full
            st2.restore(sim=b)
        c = make(n_small, seed=22, warm_start=0.0)
        cold = c.snapshot()
        cold.save()
        with pytest.raises(SdxError, match="error -1"):
            cold.restore([0], [0], sim=b)
        with pytest.raises(SdxError, match="error -1"):
            cold.save([0], [0], sim=b)
        cold.close(); full.close(); st.close()
    finally:
        a.close(); b.close()
        if c is not None:
            c.close()


# ------------------------------------------------------------------------------------------------------------------ 7. InsertSim's classes
def case_insert_classes(backend, golden_dir, n):
    """InsertSim: the base plate is one of three by env % 3, so env 0's state fits env 24 (n >= 25) but not env 8"""
    make, dev = backend
    s = make_scene_sim(backend, golden_dir, n, "insert", steps=1)
    try:
        assert s.same_class_envs(0) == [e for e in range(n) if e % 24 == 0]
        before = record(s)
        ids = lambda v: dev(torch.tensor(v, dtype=torch.int32))      # noqa: E731
        s.clone_envs(ids([0]), ids([8]))
        assert s.state_stats() == [0, 1, 0]
        assert_untouched(s, before, None, "InsertSim 0 -> 8")
        with pytest.raises(ValueError):
            s.clone_envs([0], [8])
        s.clone_envs([0], [24])
        assert_envs_equal(s, record(s), [24], before, [0], "InsertSim 0 -> 24")
        # InsertSim flags a reset on every step from this state (the brick is nowhere near the site) and reset draws are keyed by the env,
        # so the pair is followed through the physics and the observations, which is where the base plate enters
        for i in range(2):
            s.simulate()
            s.compute_observations()
            r = record(s)
            assert_envs_equal(s, r, [24], r, [0], "InsertSim physics step %d" % i)
        assert not torch.equal(per_env(s, "DOF", r["DOF"])[0], per_env(s, "DOF", before["DOF"])[0])
    finally:
        s.close()
