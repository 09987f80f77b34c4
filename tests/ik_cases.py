"""Shared bodies of the pose-solver tests (include/seqdex.h sdx_solve_ik): tests/test_ik.py runs them on the emulated
simulator (tests/hipemu), tests/test_gpu_ik.py on the GPU.  A `backend` is (make, dev) as in tests/dof_dynamics_cases.py, whose placing
helpers are used here.  The reference is the law in numpy float64 (tests/helpers/ik_float64.py) built from the scene descriptor alone; a
bar on a solution is 4 x what the same law in numpy float32 loses against float64 on the same inputs; a reached pose is judged by the
engine's own refresh_kinematics().  N = 3 everywhere (one env per workgroup: no pack size to straddle)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import torch

import dof_dynamics_cases as D
from helpers import ik_float64 as H
from seqdex_amd import _abi
from seqdex_amd import ik

f32 = np.float32
N, ND, NL, NA = D.N, D.ND, D.NL, 7
SEED = D.SEED
host = D.host
MARGIN = 4.0              # the kernel's bar over the float32 restatement's deviation (the margin of DESIGN.md sections 22 and 23)
OFFSET = (0.0, 0.0, 0.02)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINGERS = ("ff", "mf", "rf", "th")


def _params(**kw):
    base = dict(tip_offset=OFFSET)
    base.update(kw)
    return ik.IkParams(**base)


def _half(s):
    lo, up = D._limits(s)
    return 0.5 * (up - lo)


def _draw_reach(s, rng, n=N):
    """q* = mid-range + 0.3 x half-range x U(-1, 1);  q0 = clip(q* + 0.3 U(-1, 1))"""
    lo, up = D._limits(s)
    qs = (D._mid(s) + 0.3 * _half(s) * rng.uniform(-1, 1, (n, ND))).astype(f32)
    q0 = np.clip(qs + 0.3 * rng.uniform(-1, 1, (n, ND)), lo, up).astype(f32)
    return qs, q0


def _rb(s):
    rb = host(s.RB).reshape(s.num_envs, -1, 13)
    return rb[:, :NL, 0:3].astype(np.float64), rb[:, :NL, 3:7].astype(np.float64)


def _poses_at(s, dev, q, offset=OFFSET):
    """the engine's own refresh_kinematics() at q [n, 23]: hand-base position [n, 3] and orientation [n, 4], the four tip points [n, 4, 3]
    (float32, the points from the float32 rows of SDX_T_RB in float64)"""
    D._place(s, dev, q)
    p, r = _rb(s)
    ee = int(s._desc.hand_base_body)
    tips = np.array([[H.tip_point(s._desc, p[e], r[e], f, np.asarray(offset, np.float64)) for f in range(4)] for e in range(len(q))])
    return p[:, ee].astype(f32), r[:, ee].astype(f32), tips.astype(f32)


def _measure_engine(s, dev, q, bp, bq, tp, offset=OFFSET):
    """the errors of the configuration q against the targets as SDX_T_RB shows them after set-and-refresh: [n, 6] float64"""
    D._place(s, dev, q)
    p, r = _rb(s)
    ee = int(s._desc.hand_base_body)
    out = np.zeros((len(q), 6))
    for e in range(len(q)):
        out[e, 0] = np.linalg.norm(bp[e].astype(np.float64) - p[e, ee])
        out[e, 1] = np.linalg.norm(H.rotation_error(bq[e].astype(np.float64), r[e, ee]))
        for f in range(4):
            out[e, 2 + f] = np.linalg.norm(tp[e, f].astype(np.float64) - H.tip_point(s._desc, p[e], r[e], f, np.asarray(offset, np.float64)))
    return out


def _fk_slack(s, dev, q, offset=OFFSET):
    """4 x the largest difference between SDX_T_RB at q and the helper's float64 forward kinematics: link origins and tip points in m, link
    orientations as the length of the rotation error between the two"""
    D._place(s, dev, q)
    p, r = _rb(s)
    worst = 0.0
    for e in range(len(q)):
        p64, r64, _ = H.fk(s._desc, q[e], np.float64)
        worst = max(worst, float(np.abs(p[e] - p64).max()))
        worst = max(worst, max(float(np.linalg.norm(H.rotation_error(r[e, k], r64[k]))) for k in range(NL)))
        for f in range(4):
            off = np.asarray(offset, np.float64)
            worst = max(worst, float(np.abs(H.tip_point(s._desc, p[e], r[e], f, off) - H.tip_point(s._desc, p64, r64, f, off)).max()))
    return MARGIN * worst


def _t(dev, a):
    return None if a is None else dev(torch.from_numpy(np.ascontiguousarray(a, f32)))


def _call(s, dev, bp, bq, tp, params, q0):
    """-> (q [n, 23], err [n, 6], converged [n, 5], iters [n, 5]) on the host"""
    sol = s.solve_ik(_t(dev, bp), _t(dev, bq), _t(dev, tp), params, q0=_t(dev, q0))
    return host(sol.q), host(sol.err), host(sol.converged), host(sol.iters)


def _law(s, q0, bp, bq, tp, params, dtype, lower=None, upper=None):
    return [H.solve(s._desc, q0[e], None if bp is None else bp[e], None if bq is None else bq[e], None if tp is None else tp[e], params,
                    lower, upper, dtype) for e in range(len(q0))]


def _inside(s, q):
    lo, up = D._limits(s)
    return bool(np.isfinite(q).all() and (q >= lo.astype(f32)).all() and (q <= up.astype(f32)).all())


def _expect_value_error(fn, word):
    try:
        fn()
    except ValueError as err:
        assert word in str(err), err
    else:
        raise AssertionError("accepted a bad %s" % word)


def _against_float64(s, dev, q0, bp, bq, tp, params, what, margin=MARGIN):
    """q_out against the float64 law on the same q0 and targets; the bar: margin x the float32 law's deviation.  Returns (yardstick, engine's
    deviation, the float64 solutions, the engine's outputs)"""
    r64 = _law(s, q0, bp, bq, tp, params, np.float64)
    r32 = _law(s, q0, bp, bq, tp, params, np.float32)
    out = _call(s, dev, bp, bq, tp, params, q0)
    q = out[0]
    assert _inside(s, q), what
    yard = max(float(np.abs(r32[e].q.astype(np.float64) - r64[e].q).max()) for e in range(len(q0)))
    dev_ = max(float(np.abs(q[e].astype(np.float64) - r64[e].q).max()) for e in range(len(q0)))
    print("%s: q_out: float32 law vs float64 %.3g rad, engine vs float64 %.3g rad (bar %.3g, ratio %.2f)" % (
        what, yard, dev_, margin * yard, dev_ / yard if yard > 0 else float("inf")))
    assert 0 < yard < 1e-3, (what, yard)                                             # float32 rounding, not a modelling difference
    assert dev_ <= margin * yard, (what, dev_, yard)
    return yard, dev_, r64, out


# ------------------------------------------------------------------------------------------------------------------ 1. ABI
def _declared_functions():
    txt = open(os.path.join(ROOT, "include", "seqdex.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(sdx(?:p|tv)?_[a-z_0-9]+)\s*\(", txt)))


def case_abi(backend):
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        assert hasattr(s.lib, "sdx_solve_ik") and "sdx_solve_ik" in _abi.SDX_EXPORTS
        assert sorted(_abi.SDX_EXPORTS) == _declared_functions()
        assert _abi.SDX_ABI_VERSION == 8 and len(_abi.T) == 56
        src = '#include <stdio.h>\n#include "seqdex.h"\nint main(){printf("%zu %d\\n", sizeof(sdx_ik_attr), SDX_ABI_VERSION);return 0;}\n'
        with tempfile.TemporaryDirectory() as d:
            open(os.path.join(d, "t.c"), "w").write(src)
            subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
            size, abi = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
        assert size == C.sizeof(_abi.IkAttr) == 4 * (7 + 12) and abi == 8
        q0, bp, bq, tp = dev(torch.zeros(N, ND)), dev(torch.zeros(N, 3)), dev(torch.zeros(N, 4)), dev(torch.zeros(N, 4, 3))
        bq[:, 3] = 1.0
        q, err, info = dev(torch.zeros(N, ND)), dev(torch.zeros(N, 6)), dev(torch.zeros(N, 6, dtype=torch.int32))
        P = lambda t: C.c_void_p(t.data_ptr())                                      # noqa: E731
        good = _params().to_attr()
        call = s.lib.sdx_solve_ik
        assert call(None, C.byref(good), P(q0), P(bp), P(bq), P(tp), P(q), P(err), P(info), None) == -1     # NULL handle

        def refused(attr, args, word):
            assert call(s.h, attr, *args, None) == -1, word
            assert b"sdx_solve_ik: " + word in s.lib.sdx_last_error(s.h), (word, s.lib.sdx_last_error(s.h))

        full = (P(q0), P(bp), P(bq), P(tp), P(q), P(err), P(info))
        refused(None, full, b"attr is NULL")
        refused(C.byref(good), (P(q0), P(bp), P(bq), P(tp), None, P(err), P(info)), b"q_out_dev is NULL")
        refused(C.byref(good), (P(q0), None, P(bq), P(tp), P(q), P(err), P(info)), b"task_mask selects the hand base")
        refused(C.byref(good), (P(q0), P(bp), None, P(tp), P(q), P(err), P(info)), b"task_mask selects the hand base")
        refused(C.byref(good), (P(q0), P(bp), P(bq), None, P(q), P(err), P(info)), b"task_mask selects a fingertip")
        for mask in (0, 1 << 5, 0x3f, 1 << 31):
            a = _params().to_attr()
            a.task_mask = mask
            refused(C.byref(a), full, b"task_mask")
        for iters in (0, -1, 257):
            a = _params().to_attr()
            a.max_iters = iters
            refused(C.byref(a), full, b"max_iters")
        for field in ("damping_arm", "damping_finger", "max_step", "pos_tol", "rot_tol"):
            for bad in (-1.0, float("nan"), float("inf")):
                a = _params().to_attr()
                setattr(a, field, bad)
                refused(C.byref(a), full, b"damping_arm, damping_finger, max_step, pos_tol and rot_tol")
        for bad in (float("nan"), float("inf")):
            a = _params().to_attr()
            a.tip_offset[2][1] = bad
            refused(C.byref(a), full, b"tip_offset")
        a = _params().to_attr()
        a.max_step = 0.0
        refused(C.byref(a), full, b"max_step must be > 0")
        assert call(s.h, C.byref(good), *full, None) == 0
        assert call(s.h, C.byref(good), None, P(bp), P(bq), P(tp), P(q), None, None, None) == 0          # q0 from SDX_T_DOF, no err, no info
        arm, fingers = _params(tasks=("base",)).to_attr(), _params(tasks=FINGERS).to_attr()
        assert call(s.h, C.byref(arm), P(q0), P(bp), P(bq), None, P(q), P(err), P(info), None) == 0      # NULL targets, unused
        assert call(s.h, C.byref(fingers), P(q0), None, None, P(tp), P(q), P(err), P(info), None) == 0
        # the Python side: the tensor checks of osc_torques
        p = _params()
        for name, shape in (("base_pos", (N, 3)), ("base_quat", (N, 4)), ("tip_pos", (N, 4, 3)), ("q0", (N, ND)), ("out", (N, ND))):
            ok = dict(base_pos=bp, base_quat=bq, tip_pos=tp, q0=q0, out=q)
            wide = shape[:-1] + (2 * shape[-1],)
            bads = [dev(torch.zeros(shape[:-1] + (shape[-1] + 1,))), dev(torch.zeros(shape, dtype=torch.float64)), dev(torch.zeros(wide))[..., ::2], [0.0]]
            if bp.device.type != "cpu":
                bads.append(torch.zeros(shape))
            for bad in bads:
                _expect_value_error(lambda: s.solve_ik(params=p, **dict(ok, **{name: bad})), name)
        _expect_value_error(lambda: s.solve_ik(None, bq, tp, p), "base_pos")
        _expect_value_error(lambda: s.solve_ik(bp, None, tp, p), "base_quat")
        _expect_value_error(lambda: s.solve_ik(bp, bq, None, p), "tip_pos")
        _expect_value_error(lambda: ik.IkParams(tasks=("base", "pinky")), "tasks")
        _expect_value_error(lambda: ik.IkParams(tip_offset=[0.0, 1.0]), "tip_offset")
        try:
            s.solve_ik(bp, bq, tp, ik.IkParams(max_iters=0))
        except Exception as err_:                                                   # the library's own message
            assert "max_iters" in str(err_)
        else:
            raise AssertionError("max_iters = 0 accepted")
        d = ik.IkParams()
        assert d.tasks == ik.TASKS and d.task_mask == 31 and (d.max_iters, d.damping_arm, d.damping_finger, d.max_step, d.pos_tol, d.rot_tol) == (
            32, 0.05, 0.01, 0.2, 1e-4, 1e-3) and d.tip_offset == ((0.0, 0.0, 0.0),) * 4
        assert ik.IkParams(tasks="mf").task_mask == 4 and ik.IkParams(tasks=("th", "base")).task_mask == 17
        at = _params(tasks=("ff",), tip_offset=[[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]]).to_attr()
        assert at.task_mask == 2 and [list(r) for r in at.tip_offset] == [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]]
        s1 = s.solve_ik(bp, bq, tp, p)
        s2 = s.solve_ik(bp, bq, tp, good, q0=q0)                                    # a ready IkAttr
        assert tuple(s1.q.shape) == (N, ND) and tuple(s1.err.shape) == (N, 6) and s1.q.data_ptr() == s2.q.data_ptr()      # allocated once
        assert tuple(s1.converged.shape) == (N, 5) and s1.converged.dtype == torch.bool and tuple(s1.iters.shape) == (N, 5)
        assert s.solve_ik(bp, bq, tp, p, out=q).q.data_ptr() == q.data_ptr()
        assert s.solve_ik(bp, bq, tp, p, q0=q0, out=q0).q.data_ptr() == q0.data_ptr()                                   # in place
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 2. one step
def case_one_step(backend):
    """max_iters = 1, tolerances 0.  env 0: q0 0.5 rad from q* in every joint, the step limit scales the arm's step; env 1: joint 1 starts 5 mrad
    below its upper limit and the target lies beyond it, the clamp bites; env 2: a small step inside the limits, neither happens"""
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        rng = np.random.default_rng(201)
        lo, up = D._limits(s)
        qs, q0 = _draw_reach(s, rng)
        q0[0] = np.clip(qs[0] + 0.5 * rng.choice([-1.0, 1.0], ND), lo, up).astype(f32)
        q0[1:] = (D._mid(s) + 0.2 * _half(s) * rng.uniform(-1, 1, (2, ND))).astype(f32)
        qs[1:] = q0[1:] + rng.uniform(-0.04, 0.04, (2, ND)).astype(f32)
        q0[1, 1] = f32(up[1] - 0.005)
        qs[1, 1] = f32(up[1] + 0.06)                                                # (a configuration to take targets from: no limit applies to it)
        bp, bq, tp = _poses_at(s, dev, qs)
        params = _params(max_iters=1, pos_tol=0.0, rot_tol=0.0)
        yard, dev_, r64, out = _against_float64(s, dev, q0, bp, bq, tp, params, "one step of the law")
        assert r64[0].scaled[0] and not r64[0].clamped[0], r64[0]
        assert r64[1].clamped[0] and not r64[1].scaled[0] and r64[1].q[1] == up.astype(f32)[1], r64[1]
        assert not r64[2].scaled[0] and not r64[2].clamped[0], r64[2]
        q, err, conv, iters = out
        assert q[1, 1] == up.astype(f32)[1]
        assert (iters == 1).all() and not conv.any()
        step0 = np.abs(q[0, :NA].astype(np.float64) - q0[0, :NA])
        assert abs(step0.max() - 0.2) < 1e-6, step0                                 # the largest |dq_j| of the scaled step is max_step
        return yard, dev_
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 3. fixed-length loop
def case_fixed_loop(backend, margin=MARGIN):
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        rng = np.random.default_rng(202)
        qs, q0 = _draw_reach(s, rng)
        bp, bq, tp = _poses_at(s, dev, qs)
        params = _params(max_iters=8, pos_tol=0.0, rot_tol=0.0)
        yard, dev_, r64, out = _against_float64(s, dev, q0, bp, bq, tp, params, "eight steps of the law", margin)
        assert (out[3] == 8).all() and not out[2].any()
        return yard, dev_
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 4. reach
def case_reach(backend):
    """default parameters: every (env, task) pair converges, in the helper within max_iters / 2; the pose SDX_T_RB shows at q_out lies within
    the tolerances of the targets"""
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        rng = np.random.default_rng(SEED)
        qs, q0 = _draw_reach(s, rng)
        bp, bq, tp = _poses_at(s, dev, qs)
        params = _params()
        r64 = _law(s, q0, bp, bq, tp, params, np.float64)
        for e in range(N):                                                          # the helper first
            assert r64[e].converged.all() and (r64[e].iters <= params.max_iters // 2).all(), (e, r64[e])
        q, err, conv, iters = _call(s, dev, bp, bq, tp, params, q0)
        assert _inside(s, q)
        slack = max(_fk_slack(s, dev, q), _fk_slack(s, dev, qs))
        seen = _measure_engine(s, dev, q, bp, bq, tp)
        it64 = np.stack([r.iters for r in r64])
        print("reach: slack %.3g (4 x SDX_T_RB against the float64 forward kinematics); SDX_T_RB at q_out: position errors up to %.3g m "
              "(tolerance %.3g), rotation error up to %.3g (tolerance %.3g); err_out differs from them by up to %.3g; iterations engine %s "
              "helper %s" % (slack, seen[:, [0, 2, 3, 4, 5]].max(), params.pos_tol, seen[:, 1].max(), params.rot_tol, np.abs(err - seen).max(),
                             iters.tolist(), it64.tolist()))
        assert 0 < slack < 1e-5, slack
        assert conv.all(), conv
        assert (seen[:, [0, 2, 3, 4, 5]] <= f32(params.pos_tol) + slack).all(), seen
        assert (seen[:, 1] <= f32(params.rot_tol) + slack).all(), seen
        assert (np.abs(iters - it64) <= 1).all(), (iters, it64)
        assert (np.abs(err - seen) <= slack).all(), (err, seen)
        assert (iters > 0).all()
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 5. masks
def case_masks(backend):
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        rng = np.random.default_rng(205)
        qs, q0 = _draw_reach(s, rng)
        bits = lambda a: np.ascontiguousarray(a).view(np.uint32)                    # noqa: E731
        # arm only: no tip targets
        bp, bq, _ = _poses_at(s, dev, qs)
        q, err, conv, iters = _call(s, dev, bp, bq, None, _params(tasks=("base",)), q0)
        np.testing.assert_array_equal(bits(q[:, NA:]), bits(q0[:, NA:]))
        assert conv[:, 0].all() and not conv[:, 1:].any() and (iters[:, 0] > 0).all() and (iters[:, 1:] == 0).all()
        assert (bits(err[:, 2:]) == 0).all() and (np.abs(q[:, :NA] - q0[:, :NA]).max(1) > 0.01).all()
        # fingers only: the base stays at q0's pose, no base targets
        mixed = np.concatenate([q0[:, :NA], qs[:, NA:]], 1)
        _, _, tp = _poses_at(s, dev, mixed)
        q, err, conv, iters = _call(s, dev, None, None, tp, _params(tasks=FINGERS), q0)
        np.testing.assert_array_equal(bits(q[:, :NA]), bits(q0[:, :NA]))
        assert conv[:, 1:].all() and not conv[:, 0].any() and (iters[:, 0] == 0).all() and (iters[:, 1:] > 0).all()
        assert (bits(err[:, :2]) == 0).all()
        seen = _measure_engine(s, dev, q, bp, bq, tp)
        assert (seen[:, 2:] <= 1e-4 + 1e-5).all(), seen
        # one finger
        q, err, conv, iters = _call(s, dev, None, None, tp, _params(tasks=("mf",)), q0)
        mf = slice(NA + 4, NA + 8)
        rest = np.r_[0:NA + 4, NA + 8:ND]
        np.testing.assert_array_equal(bits(q[:, rest]), bits(q0[:, rest]))
        assert conv[:, 2].all() and not conv[:, [0, 1, 3, 4]].any() and (iters[:, [0, 1, 3, 4]] == 0).all()
        assert (np.abs(q[:, mf] - q0[:, mf]).max(1) > 0.01).all() and (bits(err[:, [0, 1, 2, 4, 5]]) == 0).all()
        # a target is needed exactly when its task is selected
        for kw, word in ((dict(base_pos=None, base_quat=_t(dev, bq), tip_pos=_t(dev, tp)), "base_pos"),
                         (dict(base_pos=_t(dev, bp), base_quat=_t(dev, bq), tip_pos=None), "tip_pos")):
            _expect_value_error(lambda: s.solve_ik(params=_params(), q0=_t(dev, q0), **kw), word)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 6. already there
def case_already_there(backend):
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        rng = np.random.default_rng(206)
        qs, _ = _draw_reach(s, rng)
        bp, bq, tp = _poses_at(s, dev, qs)
        q, err, conv, iters = _call(s, dev, bp, bq, tp, _params(), qs)
        np.testing.assert_array_equal(q.view(np.uint32), qs.view(np.uint32))
        assert conv.all() and (iters == 0).all()
        assert (err[:, [0, 2, 3, 4, 5]] <= 1e-4).all() and (err[:, 1] <= 1e-3).all()
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 7. unreachable
def case_unreachable(backend):
    """the base target 3 m away, the tips 0.5 m off: finite, inside the limits, nothing converges, every task uses all its iterations"""
    make, dev = backend
    s = make(N, seed=SEED)
    try:
        rng = np.random.default_rng(207)
        qs, q0 = _draw_reach(s, rng)
        bp, bq, tp = _poses_at(s, dev, qs)
        bp = (bp + f32([3.0, 0.0, 0.0])).astype(f32)
        tp = (tp + f32([0.0, 0.5, 0.0])).astype(f32)
        params = _params(max_iters=12)
        q, err, conv, iters = _call(s, dev, bp, bq, tp, params, q0)
        assert _inside(s, q) and np.isfinite(err).all()
        assert not conv.any() and (iters == 12).all(), (conv, iters)
        slack = _fk_slack(s, dev, q)
        seen = _measure_engine(s, dev, q, bp, bq, tp)
        print("unreachable: errors %s; err_out differs from SDX_T_RB's by up to %.3g (slack %.3g)" % (seen.max(0), np.abs(err - seen).max(), slack))
        assert (seen[:, 0] > 2.0).all() and (seen[:, 2:] > 0.3).all()
        assert (np.abs(err - seen) <= slack).all(), (err, seen)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 8. limits, randomization
def case_randomized_limits(backend):
    """SDX_T_DR_DOF rows 2 and 3 narrowed to mid-range +- 0.1 half-ranges, the targets at q* outside them: with randomization on the solution
    stays inside the narrowed limits and rests on some of them; a simulator with randomization off takes the same call past them"""
    make, dev = backend
    rng = np.random.default_rng(208)
    outs = []
    for randomize in (True, False):
        s = make(N, seed=SEED)
        try:
            lo, up = D._limits(s)
            nlo, nup = (D._mid(s) - 0.1 * _half(s)).astype(f32), (D._mid(s) + 0.1 * _half(s)).astype(f32)
            if randomize:
                qs = (D._mid(s) + 0.3 * _half(s) * np.sign(rng.uniform(-1, 1, (N, ND)))).astype(f32)
                q0 = np.tile(D._mid(s).astype(f32), (N, 1))
                D._dr_on(s, dev)
                dd = host(s.DR_DOF)
                np.testing.assert_array_equal(dd[:, 2], np.tile(lo.astype(f32), (N, 1)))
                dd[:, 2, :], dd[:, 3, :] = nlo, nup
                s.DR_DOF.copy_(dev(torch.from_numpy(dd)))
            bp, bq, tp = _poses_at(s, dev, qs)
            q, err, conv, iters = _call(s, dev, bp, bq, tp, _params(), q0)
            outs.append(q)
            if randomize:
                assert np.isfinite(q).all() and (q >= nlo).all() and (q <= nup).all(), q
                at = (q == nlo) | (q == nup)
                print("narrowed limits: %d of %d DOFs rest on one" % (int(at.sum()), at.size))
                assert at[:, :NA].any(1).all() and at[:, NA:].any(1).all()
                r64 = _law(s, q0, bp, bq, tp, _params(), np.float64, nlo, nup)
                assert all((r.q >= nlo).all() and (r.q <= nup).all() and r.clamped.any() for r in r64)
            else:
                assert _inside(s, q)
                assert ((q < nlo) | (q > nup)).any(1).all(), q
                assert conv.all(), conv
        finally:
            s.close()


# ------------------------------------------------------------------------------------------------------------------ 9. independence
def case_independence(backend):
    """q0 = None starts from SDX_T_DOF; the call changes no tensor of the simulator; a step after it is a step without it"""
    make, dev = backend
    rng = np.random.default_rng(209)
    s = make(N, seed=SEED)
    try:
        qs, q0 = _draw_reach(s, rng)
        bp, bq, tp = _poses_at(s, dev, qs)
    finally:
        s.close()
    qd = rng.uniform(-0.3, 0.3, (N, ND)).astype(f32)

    def run(calls):
        s = make(N, seed=SEED)
        try:
            D._place(s, dev, q0, qd)
            out = []
            for i in range(2):
                if calls:
                    before = {name: host(t).tobytes() for name, t in s._tensors.items()}
                    start = D._dofs(s)[:, :, 0].copy()
                    q, err, conv, iters = _call(s, dev, bp, bq, tp, _params(), None)
                    for name, t in s._tensors.items():
                        assert host(t).tobytes() == before[name], name
                    assert len(before) == 56
                    q2 = _call(s, dev, bp, bq, tp, _params(), start)[0]
                    np.testing.assert_array_equal(q.view(np.uint32), q2.view(np.uint32))
                    assert conv.all() and (np.abs(q - start).max(1) > 0.01).all()
                s.simulate()
                out.append([host(t).view(np.uint32) for t in (s.DOF, s.ROOT, s.RB, s.JAC_EEF, s.CONTACT)])
            return out
        finally:
            s.close()

    a, b = run(True), run(False)
    for i in range(2):
        for name, x, y in zip(("DOF", "ROOT", "RB", "JAC_EEF", "CONTACT"), a[i], b[i]):
            np.testing.assert_array_equal(x, y, err_msg="%s, step %d" % (name, i))
    assert (a[1][0] != a[0][0]).any()


# ------------------------------------------------------------------------------------------------------------------ 10. N against 2 N
def case_n_against_2n(backend):
    make, dev = backend
    outs = []
    for n in (N, 2 * N):
        s = make(n, seed=SEED)
        try:
            r = np.random.default_rng(210)
            qs, q0 = _draw_reach(s, r, n=2 * N)
            bp, bq, tp = _poses_at(s, dev, qs[:n])
            outs.append(_call(s, dev, bp, bq, tp, _params(), q0[:n]))
        finally:
            s.close()
    for name, a, b in zip(("q", "err", "converged", "iters"), *outs):
        np.testing.assert_array_equal(a.view(np.uint8), b[:N].view(np.uint8), err_msg=name)
    assert outs[0][2].all()
