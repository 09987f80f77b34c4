"""CPU (-m "not gpu"): domain randomization (include/seqdex.h sdx_set_randomization).

- the YAML parser: the shipped blocks, errors that name the key, the report of no-ops and unsupported entries;
- the ABI mirror of sdx_dr_desc;
- the device sampler (sdx_randomize.hip k_dr_sample / k_dr_gravity) on the SIMT emulator against the numpy restatement of the rules below;
- the randomization variant of k_physics on the emulator: bit-identical to the default kernel with the scene's rows, and per env equal to the
  C oracle run with that env's values as scene constants."""
import copy
import ctypes as C
import os
import subprocess
import tempfile
import warnings

import numpy as np
import pytest
import yaml

from seqdex_amd import domain_randomization as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "seqdex_amd", "cfg")
TASKS = ("grasp_sim", "insert_sim", "orient", "search")
f32 = np.float32


def shipped(name):
    with open(os.path.join(CFG, "allegro_hand_block_assembly_%s.yaml" % name)) as f:
        return yaml.safe_load(f)


# ------------------------------------------------------------------ numpy restatement of the sampling rules
M64 = (1 << 64) - 1
TAG = 0xD0A1
SLOTS = 287
SLOT_LINK, SLOT_BRICK, SLOT_GRAV = 92, 140, 284


def sdx_hash(seed, a, b):
    z = (seed + 0x9E3779B97F4A7C15 * (a + 1) + 0xBF58476D1CE4E5B9 * (b + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def uni(h, which):
    b = (h >> 16) & 0xFFFFFF if which else h >> 40
    return (f32(b) + f32(0.5)) * f32(1.0 / 16777216.0)


def sched(a, frame):
    if a.schedule == 1:
        return f32(min(frame, a.schedule_steps)) / f32(a.schedule_steps)
    if a.schedule == 2:
        return f32(0.0) if frame < a.schedule_steps else f32(1.0)
    return f32(1.0)


def _f(fn, x):   # a correctly rounded float32 libm function (float64 evaluation, one rounding)
    return f32(fn(np.float64(x)))


def value(a, s, h, v0):
    """dr_value of sdx_randomize.hip in float32 arithmetic"""
    scaling = a.operation == 2
    lo, hi, one = f32(a.range[0]), f32(a.range[1]), f32(1.0)
    if a.distribution == 1:
        mu = lo * s + (one - s) if scaling else lo * s
        z = _f(np.sqrt, f32(-2.0) * _f(np.log, uni(h, 0))) * _f(np.cos, f32(6.28318530718) * uni(h, 1))
        x = mu + (hi * s) * f32(z)
    else:
        a0 = lo * s + (one - s) if scaling else lo * s
        a1 = hi * s + (one - s) if scaling else hi * s
        u = uni(h, 0)
        if a.distribution == 2:
            x = a0 + (a1 - a0) * u
        else:
            x = a0 if a0 == a1 else _f(np.exp, _f(np.log, a0) + (_f(np.log, a1) - _f(np.log, a0)) * u)
    if a.num_buckets > 0:
        blo = lo - f32(2.0) * _f(np.sqrt, hi) if a.distribution == 1 else lo
        bhi = lo + f32(2.0) * _f(np.sqrt, hi) if a.distribution == 1 else hi
        nb = a.num_buckets
        grid = [blo + (bhi - blo) * f32(k) / f32(nb) for k in range(nb)]
        k = max(0, sum(1 for g in grid if g <= x) - 1)
        x = grid[k]
    return f32(v0 * x) if scaling else f32(v0 + x)


def sample_env(d, desc, seed, e, draw, frame):
    """the rows k_dr_sample writes for env e: dof [4,23], link [2,24], brick [2,72]; None where an attribute is not randomized"""
    out = {}
    for k in range(SLOT_GRAV):
        if k < SLOT_LINK:
            r, j = divmod(k, 23)
            a = (d.dof_stiffness, d.dof_damping, d.dof_lower, d.dof_upper)[r]
            v0 = f32((desc.kp, desc.kd, desc.lower, desc.upper)[r][j])
            factor = False
        elif k < SLOT_BRICK:
            i = k - SLOT_LINK
            factor = i < 24
            a = d.link_mass if factor else d.link_friction
            v0 = f32(desc.link_mass[i % 24] if factor else desc.friction)
        else:
            i = k - SLOT_BRICK
            factor = i < 72
            a = d.brick_mass if factor else d.brick_friction
            v0 = f32(desc.brick_mass[desc.brick_type[i % 72]] if factor else desc.friction)
        if a.distribution == 0:
            out[k] = None
            continue
        scaled = a.operation == 2
        base = f32(1.0) if factor and scaled else v0
        s = sched(a, frame)
        v = base if s == 0 else value(a, s, sdx_hash(seed ^ TAG, e * SLOTS + k, draw), base)
        out[k] = (v / v0 if v0 != 0 else f32(1.0)) if factor and not scaled else v
    return out


def sample_gravity(d, desc, seed, draw, frame):
    s = sched(d.gravity, frame)
    return [f32(desc.gravity[c]) if s == 0 else value(d.gravity, s, sdx_hash(seed ^ TAG, SLOT_GRAV + c, draw), f32(desc.gravity[c]))
            for c in range(3)]


def device_rows(sim, e):
    rows = np.concatenate([sim.DR_DOF[e].numpy().ravel(), sim.DR_LINK[e].numpy().ravel(), sim.DR_BRICK[e].numpy().ravel()])
    assert rows.size == SLOT_GRAV
    return rows


def assert_env_matches(sim, d, e, draw, frame, ulps):
    want = sample_env(d, sim._desc, 22, e, draw, frame)
    got = device_rows(sim, e)
    for k, w in want.items():
        if w is None:
            continue
        attr = (k // 23) if k < SLOT_LINK else None
        exact = ulps == 0 or (attr is None and k >= SLOT_LINK)   # uniform slots (masses, frictions) are exact
        if exact:
            assert got[k] == w, (e, k, got[k], w)
        else:
            assert abs(int(np.float32(got[k]).view(np.int32)) - int(np.float32(w).view(np.int32))) <= ulps, (e, k, got[k], w)


# ------------------------------------------------------------------ 1. parsing
@pytest.mark.parametrize("task", TASKS)
def test_shipped_blocks_parse_and_stay_off(task):
    cfg = shipped(task)
    assert cfg["task"]["randomize"] is False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        d, rep = dr.parse(cfg["task"]["randomization_params"])
    assert d.frequency == 1000
    g = d.gravity
    assert (g.distribution, g.operation, g.schedule, g.schedule_steps, list(g.range)) == (1, 1, 1, 40000, [0.0, f32(0.4)])
    for f, dist, op, rng in (("dof_stiffness", 3, 2, [0.75, 1.5]), ("dof_damping", 3, 2, [0.3, 3.0]), ("dof_lower", 1, 1, [0.0, 0.01]),
                             ("dof_upper", 1, 1, [0.0, 0.01]), ("link_mass", 2, 2, [0.5, 1.5]), ("link_friction", 2, 2, [0.7, 1.3])):
        a = getattr(d, f)
        assert (a.distribution, a.operation, a.schedule, a.schedule_steps) == (dist, op, 1, 30000), f
        np.testing.assert_array_equal(list(a.range), np.float32(rng))
    assert d.link_friction.num_buckets == 250 and d.link_mass.num_buckets == 0
    assert set(rep["noop"]) >= {"observations", "actions", "actor_params.hand.tendon_properties"}
    lego = task != "search"       # the reference Search block has its brick entries commented out
    assert ("actor_params.hand.color" in rep["noop"]) == lego
    assert ("actor_params.lego.scale" in rep["unsupported"]) == lego
    assert (d.brick_friction.num_buckets, d.brick_mass.distribution) == ((250, 2) if lego else (0, 0))
    assert len(rep["randomized"]) == (9 if lego else 7)


def test_parse_errors_name_the_key():
    base = shipped("grasp_sim")["task"]["randomization_params"]
    cases = [
        (lambda p: p["actor_params"].__setitem__("robot", {}), "actor_params.robot"),
        (lambda p: p["actor_params"]["hand"].__setitem__("joint_properties", {}), "actor_params.hand.joint_properties"),
        (lambda p: p["actor_params"]["hand"]["dof_properties"].__setitem__("armature", p["actor_params"]["hand"]["dof_properties"]["lower"]),
         "actor_params.hand.dof_properties.armature"),
        (lambda p: p["actor_params"]["hand"]["rigid_body_properties"].__setitem__("inertia", {}), "rigid_body_properties.inertia"),
        (lambda p: p["actor_params"]["hand"]["rigid_body_properties"]["mass"].__setitem__("distribution", "beta"), "mass.distribution"),
        (lambda p: p["sim_params"]["gravity"].__setitem__("operation", "multiply"), "gravity.operation"),
        (lambda p: p["sim_params"]["gravity"].__setitem__("schedule", "cosine"), "gravity.schedule"),
        (lambda p: p["sim_params"].__setitem__("dt", p["sim_params"]["gravity"]), "sim_params.dt"),
        (lambda p: p.__setitem__("camera", {}), "randomization_params.camera"),
    ]
    for mutate, key in cases:
        p = copy.deepcopy(base)
        mutate(p)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(ValueError, match=key.replace(".", r"\.")):
                dr.parse(p)
    with pytest.raises(ValueError, match="randomization_params"):
        dr.parse({})


def test_lego_scale_warns_once_per_process():
    p = shipped("insert_sim")["task"]["randomization_params"]
    dr._warned.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        dr.parse(p)
        dr.parse(p)
    msgs = [str(x.message) for x in w if "lego.scale" in str(x.message)]
    assert len(msgs) == 1


# ------------------------------------------------------------------ 2. ABI
def test_dr_desc_layout_matches_header():
    src = ('#include <stdio.h>\n#include "seqdex.h"\nint main(){printf("%zu %zu\\n", sizeof(sdx_dr_desc), sizeof(sdx_dr_attr));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        a, b = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    assert int(a) == C.sizeof(dr.DrDesc) and int(b) == C.sizeof(dr.DrAttr)
    from seqdex_amd import _abi
    assert [_abi.T[k] for k in ("DR_DOF", "DR_LINK", "DR_BRICK", "DR_GRAVITY", "DR_FRAME")] == [51, 52, 53, 54, 55]


# ------------------------------------------------------------------ 3. the sampler on the emulator
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def emu():
    from tests.hipemu.sim import EmuSim
    return EmuSim


def _desc_all():
    """every distribution, bucketed friction, schedules"""
    p = copy.deepcopy(shipped("grasp_sim")["task"]["randomization_params"])
    p["actor_params"].pop("lego")
    p["actor_params"]["lego"] = {"rigid_body_properties": {"mass": {"range": [0.5, 1.5], "operation": "scaling", "distribution": "uniform",
                                                                    "schedule": "constant", "schedule_steps": 300}},
                                 "rigid_shape_properties": {"friction": {"range": [1.0, 0.1], "operation": "scaling", "distribution": "gaussian",
                                                                         "num_buckets": 40, "schedule": "linear", "schedule_steps": 30000}}}
    p["frequency"] = 3
    d, _ = dr.parse(p)
    return d


@pytest.mark.parametrize("frame", [0, 15000, 20000, 50000])
def test_emulated_sampler_matches_numpy(emu, frame):
    d = _desc_all()
    s = emu(3, seed=22)
    try:
        s.DR_FRAME[0] = frame
        s.set_randomization(d)
        for e in range(3):
            assert_env_matches(s, d, e, 0, frame, ulps=2)
        want_g = sample_gravity(d, s._desc, 22, 0, frame)
        got_g = s.DR_GRAVITY.numpy()
        for c in range(3):
            assert abs(int(np.float32(got_g[c]).view(np.int32)) - int(np.float32(want_g[c]).view(np.int32))) <= 2
        if frame == 0:     # the linear schedule starts at "no randomization": every value is the scene's (constant-schedule masses too)
            np.testing.assert_array_equal(s.DR_DOF[:, 0].numpy(), np.tile(np.float32(s._desc.kp), (3, 1)))
            np.testing.assert_array_equal(s.DR_BRICK.numpy()[:, 1], np.float32(s._desc.friction))
            np.testing.assert_array_equal(s.DR_LINK.numpy()[:, 0], 1.0)
            np.testing.assert_array_equal(got_g, np.float32(s._desc.gravity))
        else:
            assert (s.DR_DOF[:, 0].numpy() != np.float32(s._desc.kp)).mean() > 0.9
        if frame >= 30000:  # past schedule_steps: friction on its 250-bucket grid
            lo, hi = f32(0.7), f32(1.3)
            grid = np.array([lo + (hi - lo) * f32(k) / f32(250) for k in range(250)], np.float32) * np.float32(s._desc.friction)
            assert np.isin(s.DR_LINK.numpy()[:, 1], grid).all()
        assert (s.DR_FRAME.numpy() == [frame, frame]).all()
    finally:
        s.close()


def test_emulated_frequency_rule(emu):
    """an env is re-sampled when it resets with randomize_buf >= frequency (randomize_buf -> 0); gravity when some env resets and
    frame - last_rand_frame >= frequency (BT:238-248)"""
    d = _desc_all()                  # frequency 3
    n = 4
    s = emu(n, seed=22)
    try:
        s.DR_FRAME[0] = 40000
        s.set_randomization(d)
        draws = [0] * n
        gdraw, last = 0, 40000
        acts = torch.zeros(n, 23)
        for frame, reset, rbuf in ((40001, [1, 1, 0, 0], [3, 2, 5, 0]), (40002, [0, 0, 0, 0], [9, 9, 9, 9]),
                                   (40004, [0, 1, 1, 1], [0, 7, 3, 1]), (40005, [1, 0, 0, 0], [4, 0, 0, 0])):
            s.DR_FRAME[0] = frame
            s.RESET[:] = torch.tensor(reset)
            s.RANDOMIZE[:] = torch.tensor(rbuf)
            before = [device_rows(s, e).copy() for e in range(n)]
            g_before = s.DR_GRAVITY.numpy().copy()
            s.pre_physics(acts)
            for e in range(n):
                hit = reset[e] and rbuf[e] >= 3
                if hit:
                    draws[e] += 1
                    assert_env_matches(s, d, e, draws[e], frame, ulps=2)
                    assert s.RANDOMIZE[e] == 0
                else:
                    np.testing.assert_array_equal(device_rows(s, e), before[e])
                    assert s.RANDOMIZE[e] == rbuf[e]
            if any(reset) and frame - last >= 3:
                gdraw += 1
                last = frame
                want = sample_gravity(d, s._desc, 22, gdraw, frame)
                np.testing.assert_allclose(s.DR_GRAVITY.numpy(), want, rtol=1e-6, atol=1e-7)
            else:
                np.testing.assert_array_equal(s.DR_GRAVITY.numpy(), g_before)
            assert s.DR_FRAME[1] == last
    finally:
        s.close()


def test_emulated_samples_do_not_depend_on_n(emu):
    d = _desc_all()
    a, b = emu(2, seed=22), emu(5, seed=22)
    try:
        for s in (a, b):
            s.DR_FRAME[0] = 35000
            s.set_randomization(d)
        for name in ("DR_DOF", "DR_LINK", "DR_BRICK", "DR_GRAVITY"):
            np.testing.assert_array_equal(getattr(a, name).numpy()[:2], getattr(b, name).numpy()[:2])
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 4. physics on the emulator
def _state(scene, n):
    from test_physics_oracle import base_state
    root, dof, tg = base_state(scene, n)
    t0 = scene.brick_types[0]
    floor_top = scene.statics[6]["center"][2] + scene.statics[6]["half"][2]
    root[:, 9, 0:3] = [0.25, 0.19, floor_top + t0["half"][2] - t0["center"][2] - 0.0005]   # brick 0 sliding on the floor slab
    root[:, 9, 7:10] = [0.6, 0.0, 0.0]
    tg[:, 8] = scene.upper[8] + 0.5                                                         # dof 8 driven past its upper limit
    return root, dof, tg


def _load(s, root, dof, tg):
    s.ROOT.numpy()[:] = root.reshape(s.ROOT.shape)
    s.DOF.numpy()[:] = dof.reshape(s.DOF.shape)
    s.TARGETS.numpy()[:] = tg
    s.WARM_COUNT.zero_()
    s.refresh_kinematics()


def test_emulated_variant_with_scene_rows_is_bit_identical(emu):
    from seqdex_amd.scene import load_scene
    scene = load_scene()
    root, dof, tg = _state(scene, 1)
    a, b = emu(1, seed=22), emu(1, seed=22)
    try:
        _load(a, root, dof, tg)
        _load(b, root, dof, tg)
        b.set_randomization(dr.identity_desc())
        for _ in range(2):
            a.simulate()
            b.simulate()
        for name in ("ROOT", "DOF", "RB", "CONTACT"):
            np.testing.assert_array_equal(getattr(a, name).numpy(), getattr(b, name).numpy(), err_msg=name)
        assert int(b.DR_FRAME[0]) == 2 and int(a.DR_FRAME[0]) == 0
    finally:
        a.close()
        b.close()


def test_emulated_per_env_rows_match_oracle(emu):
    """each env of one launch = the C oracle run with that env's values as scene constants (a brick on a static body: the oracle's
    friction is the mean of the brick's and the static body's)"""
    from oracle import physics_oracle as po
    from seqdex_amd.scene import load_scene
    scene = load_scene()
    n = 2
    root, dof, tg = _state(scene, n)
    s = emu(n, seed=22, warm_start=0.0)
    try:
        _load(s, root, dof, tg)
        s.set_randomization(dr.identity_desc())
        base = s._desc
        fb = [0.4, 1.3]                      # brick friction factors (x scene friction)
        kpf, kdf, up = [1.0, 0.6], [1.0, 2.0], [0.0, -0.05]
        lmf, bmf = [1.0, 1.4], [1.0, 0.7]
        grav = [0.3, -0.2, -8.0]            # global: every env's oracle gets it
        descs = []
        for e in range(n):
            s.DR_DOF[e, 0] = torch.tensor(np.float32(base.kp) * f32(kpf[e]))
            s.DR_DOF[e, 1] = torch.tensor(np.float32(base.kd) * f32(kdf[e]))
            s.DR_DOF[e, 3] = torch.tensor(np.float32(base.upper) + f32(up[e]))
            s.DR_LINK[e, 0] = lmf[e]
            s.DR_BRICK[e, 0] = bmf[e]
            s.DR_BRICK[e, 1] = float(f32(base.friction) * f32(fb[e]))
            d = type(base).from_buffer_copy(base)
            d.friction = f32(0.5) * (f32(base.friction) * f32(fb[e]) + f32(base.friction))
            for j in range(23):
                d.kp[j] = np.float32(base.kp[j]) * f32(kpf[e])
                d.kd[j] = np.float32(base.kd[j]) * f32(kdf[e])
                d.upper[j] = np.float32(base.upper[j]) + f32(up[e])
            for k in range(24):
                d.link_mass[k] = np.float32(base.link_mass[k]) * f32(lmf[e])
                for i in range(6):
                    d.link_inertia[k][i] = np.float32(base.link_inertia[k][i]) * f32(lmf[e])
            for t in range(8):
                d.brick_mass[t] = np.float32(base.brick_mass[t]) * f32(bmf[e])
                for i in range(3):
                    d.brick_inertia[t][i] = np.float32(base.brick_inertia[t][i]) * f32(bmf[e])
            d.gravity[:] = grav
            d.warm_start = 0.0
            descs.append(d)
        s.DR_GRAVITY[:] = torch.tensor(grav)
        o = [(root[e:e + 1].copy(), dof[e:e + 1].copy()) for e in range(n)]
        for it in range(8):
            s.simulate()
            g_root = s.ROOT.numpy().reshape(n, 142, 13)
            g_dof = s.DOF.numpy().reshape(n, 23, 2)
            for e in range(n):
                po.simulate(descs[e], o[e][0], o[e][1], tg[e:e + 1])
                np.testing.assert_allclose(g_root[e, 9, 7:10], o[e][0][0, 9, 7:10], atol=2e-5)
                np.testing.assert_allclose(g_root[e, 10:13, 0:3], o[e][0][0, 10:13, 0:3], atol=2e-5)
                np.testing.assert_allclose(g_dof[e, :, 0], o[e][1][0, :, 0], atol=1e-5)
                np.testing.assert_allclose(g_dof[e, :, 1], o[e][1][0, :, 1], atol=5e-5)
            if it == 0:   # the two envs really differ: brick 0 decelerates by its own friction
                assert abs(g_root[0, 9, 7] - g_root[1, 9, 7]) > 1e-2
        for _ in range(30):
            s.simulate()
        g_dof = s.DOF.numpy().reshape(n, 23, 2)
        for e in range(n):
            assert g_dof[e, 8, 0] == np.float32(base.upper[8]) + f32(up[e])
    finally:
        s.close()


def test_bad_ranges_are_rejected(emu):
    """a negative sigma would put NaN into the rows (its square root makes a bucket grid); lo > hi is an error too - in the parser and in
    the C entry point"""
    g = {"range": [0.0, -0.1], "operation": "additive", "distribution": "gaussian", "num_buckets": 10}
    u = {"range": [1.3, 0.7], "operation": "scaling", "distribution": "uniform"}
    for spec, key in ((g, "sim_params.gravity.range"), (u, "sim_params.gravity.range")):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            dr.parse({"sim_params": {"gravity": spec}})
    from seqdex_amd.sim import SdxError
    s = emu(1, seed=22)
    try:
        for rng in ((0.0, -0.1), ):
            d = dr.identity_desc()
            d.gravity.distribution, d.gravity.operation, d.gravity.num_buckets = 1, 1, 10
            d.gravity.range[0], d.gravity.range[1] = rng
            with pytest.raises(SdxError, match="sdx_set_randomization"):
                s.set_randomization(d)
        d = dr.identity_desc()
        d.link_mass.distribution, d.link_mass.operation = 2, 2
        d.link_mass.range[0], d.link_mass.range[1] = 1.5, 0.5
        with pytest.raises(SdxError, match="sdx_set_randomization"):
            s.set_randomization(d)
    finally:
        s.close()


def test_emulated_reset_idx_resamples_masked_envs(emu):
    """reset_idx -> apply_randomizations (GS:1395-1396): sdx_reset_idx re-samples the masked envs whose randomize_buf >= frequency"""
    d = _desc_all()                  # frequency 3
    n = 3
    s = emu(n, seed=22)
    try:
        s.DR_FRAME[0] = 40000
        s.set_randomization(d)
        s.RESET.zero_()
        s.RANDOMIZE[:] = torch.tensor([5, 5, 1])
        before = [device_rows(s, e).copy() for e in range(n)]
        s.reset_idx(torch.tensor([1, 0, 1], dtype=torch.uint8))
        assert_env_matches(s, d, 0, 1, 40000, ulps=2)
        np.testing.assert_array_equal(device_rows(s, 1), before[1])      # not in the mask
        np.testing.assert_array_equal(device_rows(s, 2), before[2])      # randomize_buf < frequency
        assert s.RANDOMIZE.tolist() == [0, 5, 1]
    finally:
        s.close()
