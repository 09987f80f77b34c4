"""-m gpu: the persistent update runs Adam of layers 1 and 2 with the operands of the next element in flight (adam_l1_ahead / adam_l2_ahead,
csrc/sdxp_persist_adam.h) instead of loops that read every operand behind the arithmetic of the element in front.  The arithmetic of an element is
the serial loops', rounding for rounding:

    d_s = rn(dy_s gs)                                       gg = fma(d_3, x_3, fma(d_2, x_2, fma(d_1, x_1, fma(d_0, x_0, 0))))
    m = fma(0.1, gg, rn(0.9 m))                             v = fma(gg, rn(0.001 gg), rn(0.999 v))
    w = fma(-rn(lrb m), v_rcp(fma(isq, v_sqrt(v), 1e-8)), w)

The serial loops are kept as the reference inside the test entry sdxpk_adam_ahead_check (csrc/sdxp_persist_checks.hip, built with the epoch
kernel's flags): one workgroup of 512 threads standing for CU 37, an LDS image [3][4][1024] for S.x1, per lane 8 elements x 3 networks of
(w, m, v), column factors per lane, row factors per row; it hands back (gg, m, v, w) of the serial loops and of adam_l1_ahead.

(a) adam_l1_ahead against the serial loops, bit for bit, gg, m, v and w of all 12 288 elements.
(b) gg, m, v of the serial loops against the forms above in exact rational arithmetic on the host (dyadic rationals as integer pairs), rounded to float32 once per operation, bit for
    bit.  First the host shows that the inputs tell the forms apart: gg against multiply-then-add, m against fma(0.9, m, rn(0.1 gg)), v against
    fma(0.999, v, rn(rn(0.001 gg) gg)), each in at least 15 % of the elements.  Rows with gg = 0, with v = 0 and gg = 0 (denominator 1e-8) and
    with negative m are among the inputs.
(c) w of the serial loops against float64: |w - w64| <= B 2^-24 (|w_old| + |step64|), step64 = lrb m / (isq sqrt(v) + 1e-8) in float64.  The
    serial loops of the commit before this change measure W_PARENT (below) on these inputs (v_sqrt / v_rcp are 1 ulp each; measure_w() below, printed by the
    test); B is four times that.
(d) two epoch-kernel handles from one state at 4 actors x horizon 8, minibatch 4, 2 mini-epochs - 16 optimiser steps, the smallest shape that
    runs every shadow with `pending` false and true: parameters, moments and the rewritten mu / sigma rows bit-identical.
(e) the same case against the hipGraph path (SDXP_UPDATE_IMPL=graph): max |persistent - graph| of every parameter array within four times
    what the commit before this change shows.  The hipGraph path's reductions use atomics and move from run to run, so PARENT holds the largest
    of 8 measurements with measure_paths_parameters() on that commit."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from helpers.persist_float64 import persistent_or_skip  # noqa: E402
from test_gpu_persist_input_grams import _agent  # noqa: E402

MB, U0, U1, NTH, G = 4, 1024, 512, 512, 37
F32 = np.float32
# SC_*: clip scale of actor-critic / central value, lr / (1 - b1^t) and 1 / sqrt(1 - b2^t) of the two optimisers (t = 3 and t = 5, lr 3e-4 and 5e-4)
SCAL = np.array([0.731, 0.412, 3e-4 / (1 - 0.9 ** 3), 1 / np.sqrt(1 - 0.999 ** 3), 5e-4 / (1 - 0.9 ** 5), 1 / np.sqrt(1 - 0.999 ** 5)], F32)
ZERO_COL, ZERO_LANE = 7, 5          # column of S.x1 that is zero in every sample (row element 0 of lane 7 of waves 0 and 4); lane whose column factors are zero
W_PARENT = 1.585                    # (c): max |w - w64| / (2^-24 (|w_old| + |step64|)) of the serial loops - the code of the commit before this change - as this test prints it
W_BOUND = 4.0 * W_PARENT
# (e): max |persistent - graph| with the library of the commit before this change (SDX_LIB_PATH=<its libseqdex_hip.so>), largest of 8 runs of
#   python -c "import sys; sys.path[:0] = ['tests', '.']; import test_gpu_persist_adam_ahead as t; [print(t.measure_paths_parameters()) for _ in range(8)]"
#   {'AC_PARAMS': 7.70e-06, 'CV_PARAMS': 1.61e-05} {6.89e-06, 2.09e-05} {8.44e-06, 2.18e-05} {8.44e-06, 3.71e-05} {5.38e-06, 2.02e-05} {6.89e-06, 2.91e-05} {8.44e-06, 2.81e-05} {7.64e-06, 2.22e-05}
PARENT = {"AC_PARAMS": 8.444301784038544e-06, "CV_PARAMS": 3.708153963088989e-05}


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def inputs():
    """x1 [3][MB][U0], dy1 [3][MB][U1], dyr [3][MB][2], state [3: w, m, v][24][NTH]"""
    r = np.random.default_rng(0)
    x1 = r.standard_normal((3, MB, U0)).astype(F32)
    dy1 = (0.01 * r.standard_normal((3, MB, U1))).astype(F32)
    dyr = (0.01 * r.standard_normal((3, MB, 2))).astype(F32)
    w = (0.1 * r.standard_normal((24, NTH))).astype(F32)
    m = (0.01 * r.standard_normal((24, NTH))).astype(F32)
    v = r.uniform(0.0, 1e-4, (24, NTH)).astype(F32)
    x1[:, :, ZERO_COL] = 0.0                      # gg = 0 in a row element (v > 0)
    dy1[:, :, ZERO_LANE] = 0.0                    # gg = 0 in the column elements of one lane ...
    for net in range(3):
        v[net * 8 + 4:net * 8 + 8, ZERO_LANE] = 0.0   # ... whose second moments are zero: denominator 1e-8
    return x1, dy1, dyr, np.stack([w, m, v])


def operands(x1, dy1, dyr):
    """(dy [24][NTH][MB], x [24][NTH][MB], net [24]) of every element, as the kernel addresses them"""
    tid = np.arange(NTH)
    wave, lane = tid >> 6, tid & 63
    dy, x = np.empty((24, NTH, MB), F32), np.empty((24, NTH, MB), F32)
    for net in range(3):
        for j in range(8):
            k = (wave & 3) * 256 + lane + 64 * j if j < 4 else np.full(NTH, 4 * G + j - 4)
            x[net * 8 + j] = x1[net][:, k].T
            dy[net * 8 + j] = dyr[net][:, wave >> 2].T if j < 4 else dy1[net][:, tid].T
    return dy, x, np.repeat(np.arange(3), 8)


# Exact arithmetic on the host: every float32 and every product or sum of them is a dyadic rational n 2^e, held as the pair of Python integers (n, e)
def fr(x):
    m, e = math.frexp(float(x))
    return int(m * 2 ** 53), e - 53


def mul(a, b):
    return a[0] * b[0], a[1] + b[1]


def add(a, b):
    if a[1] < b[1]:
        a, b = b, a
    return (a[0] << (a[1] - b[1])) + b[0], b[1]


def rn(a):
    """n 2^e rounded to float32, to nearest, ties to even (subnormals included), as a Python float"""
    n, e = a
    if n == 0:
        return 0.0
    s, n = (-1 if n < 0 else 1), abs(n)
    u = max(e + n.bit_length() - 1, -126) - 23          # exponent of the last place
    sh = u - e
    if sh <= 0:
        return math.ldexp(s * n, e)
    f, rem, half = n >> sh, n & ((1 << sh) - 1), 1 << (sh - 1)
    if rem > half or (rem == half and (f & 1)):
        f += 1
    return math.ldexp(s * f, u)


def fma(a, b, c):
    """rn(a b + c) of three floats"""
    return rn(add(mul(fr(a), fr(b)), fr(c)))


def rmul(a, b):
    return rn(mul(fr(a), fr(b)))


def exact_forms(dy, x, net, state):
    """(gg, m, v) of the kernel's forms and the fractions of elements in which (multiply-then-add, the other contraction of m, of v) differ"""
    c09, c0999, c0001, c01 = float(F32(0.9)), float(F32(0.999)), float(F32(0.001)), float(F32(0.1))
    gg, mo, vo = np.empty((24, NTH), F32), np.empty((24, NTH), F32), np.empty((24, NTH), F32)
    other = np.zeros(3)
    dy, x, state = dy.astype(np.float64), x.astype(np.float64), state.astype(np.float64)     # (exact: Python floats of the float32 values)
    for e in range(24):
        gs = float(SCAL[1] if net[e] == 2 else SCAL[0])
        for t in range(NTH):
            g, ga = 0.0, 0.0
            for s in range(MB):
                d = rmul(dy[e, t, s], gs)
                g = fma(d, x[e, t, s], g)
                ga = rn(add(fr(rmul(d, x[e, t, s])), fr(ga)))
            m0, v0 = state[1, e, t], state[2, e, t]
            m = fma(c01, g, rmul(c09, m0))
            v = fma(g, rmul(c0001, g), rmul(c0999, v0))
            other += (ga != g, fma(c09, m0, rmul(c01, g)) != m, fma(c0999, v0, rmul(rmul(c0001, g), g)) != v)
            gg[e, t], mo[e, t], vo[e, t] = g, m, v
    return gg, mo, vo, other / (24 * NTH)


_cache = {}


def _run():
    """(inputs, out [2][4][24][NTH] of the test entry, host forms); computed once"""
    if not _cache:
        from seqdex_amd import _abi
        from seqdex_amd.sim import _stream_ptr
        lib, dev = _abi.load_library(), torch.device("cuda:0")
        lib.sdxpk_adam_ahead_check.restype = C.c_int
        lib.sdxpk_adam_ahead_check.argtypes = [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3
        x1, dy1, dyr, state = inputs()
        d = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (x1, dy1, dyr, SCAL, state)]
        out = torch.full((2, 4, 24, NTH), float("nan"), device=dev)
        assert lib.sdxpk_adam_ahead_check(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), G, d[4].data_ptr(), out.data_ptr(), _stream_ptr(dev)) == 0
        torch.cuda.synchronize()
        dy, x, net = operands(x1, dy1, dyr)
        _cache["r"] = ((dy, x, net, state), out.cpu().numpy(), exact_forms(dy, x, net, state))
    return _cache["r"]


def test_helper_equals_the_serial_loops_bit_for_bit():
    _, out, _ = _run()
    assert np.isfinite(out).all()
    for i, name in enumerate(("gg", "m", "v", "w")):
        bad = np.argwhere(bits(out[1, i]) != bits(out[0, i]))
        print("%s: %d of %d elements of adam_l1_ahead differ in bits from the serial loops" % (name, len(bad), out[0, i].size))
        assert len(bad) == 0, "%s: first (element, thread) %r: helper %r serial %r" % (name, tuple(bad[0]), out[1, i][tuple(bad[0])], out[0, i][tuple(bad[0])])


def test_serial_loops_have_the_stated_forms():
    (dy, x, net, state), out, (gg, m, v, other) = _run()
    print("inputs: gg differs from multiply-then-add in %.1f %% of the elements, m from the other contraction in %.1f %%, v in %.1f %%" % tuple(100 * other))
    assert (other >= 0.15).all(), other
    assert (gg == 0).sum() >= 12 and ((gg == 0) & (state[2] == 0)).sum() >= 12 and (state[1] < 0).mean() > 0.4      # the rows asked for are there
    assert ((v == 0) == ((gg == 0) & (state[2] == 0))).all()
    for name, got, want in (("gg", out[0, 0], gg), ("m", out[0, 1], m), ("v", out[0, 2], v)):
        # (+0 and -0: fma(d, x, +0) of a vanishing product is +0 in the kernel and in the rational form alike; compare values there, bits elsewhere)
        bad = np.argwhere((bits(got) != bits(want)) & ~((got == 0) & (want == 0)))
        print("%s: %d of %d elements of the serial loops differ from the exact forms" % (name, len(bad), got.size))
        assert len(bad) == 0, "%s: first (element, thread) %r: kernel %r host %r" % (name, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def measure_w(out, dy, x, net, state):
    """max over the elements of |w - w64| / (2^-24 (|w_old| + |step64|)) for the serial loops"""
    gs = np.where(net == 2, SCAL[1], SCAL[0]).astype(np.float64)[:, None]
    lrb = np.where(net == 2, SCAL[4], SCAL[2]).astype(np.float64)[:, None]
    isq = np.where(net == 2, SCAL[5], SCAL[3]).astype(np.float64)[:, None]
    g = ((dy.astype(np.float64) * gs[:, :, None]) * x.astype(np.float64)).sum(-1)
    m = 0.9 * state[1].astype(np.float64) + 0.1 * g
    v = 0.999 * state[2].astype(np.float64) + 0.001 * g * g
    step = lrb * m / (isq * np.sqrt(v) + 1e-8)
    w64 = state[0].astype(np.float64) - step
    return float((np.abs(out[0, 3].astype(np.float64) - w64) / (2.0 ** -24 * (np.abs(state[0].astype(np.float64)) + np.abs(step)))).max())


def test_serial_loops_weight_against_float64():
    (dy, x, net, state), out, _ = _run()
    worst = measure_w(out, dy, x, net, state)
    print("w of the serial loops: max |w - w64| = %.3f * 2^-24 (|w_old| + |step64|) (before the change %.3g, bound %.3g)" % (worst, W_PARENT, W_BOUND))
    assert worst <= W_BOUND


KEYS = ("AC_PARAMS", "CV_PARAMS", "AC_ADAM_M", "AC_ADAM_V", "CV_ADAM_M", "CV_ADAM_V", "MB_MUS", "MB_SIGMAS")


def measure_paths_parameters():
    """{parameter array: max |persistent - graph|} after one update of 2 mini-epochs of the 4 x 8 rollout (16 optimiser steps)"""
    a, b = _agent(2), _agent(2, impl="graph")
    try:
        persistent_or_skip(a)
        assert b.update_impl() == "graph"
        a.update(); b.update()
        torch.cuda.synchronize()
        assert a.update_impl() == "persistent" and a.ctrl().ac_t == b.ctrl().ac_t == 16
        return {k: float((a.t[k].double() - b.t[k].double()).abs().max()) for k in PARENT}
    finally:
        a.close(); b.close()


def test_two_epoch_handles_end_bit_identical():
    a, b = _agent(2), _agent(2)
    try:
        persistent_or_skip(a)
        assert b.update_impl() == "persistent"
        p0 = a.t["AC_PARAMS"].clone()
        a.update(); b.update()
        torch.cuda.synchronize()
        assert a.update_impl() == "persistent" and a.ctrl().ac_t == b.ctrl().ac_t == 16
        for k in KEYS:
            np.testing.assert_array_equal(a.t[k].cpu().numpy().view(np.int32), b.t[k].cpu().numpy().view(np.int32), err_msg=k)
        assert float((a.t["AC_PARAMS"] - p0).abs().max()) > 1e-4              # the epoch did something
    finally:
        a.close(); b.close()


def test_parameters_against_the_graph_path():
    got = measure_paths_parameters()
    for k, d in got.items():
        print("%s: max |persistent - graph| %.4e (before the change %.4e, bound %.4e)" % (k, d, PARENT[k], 4.0 * PARENT[k]))
    for k, d in got.items():
        assert d <= 4.0 * PARENT[k], (k, d)
