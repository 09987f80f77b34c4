"""-m gpu: the persistent update takes the Adam elements of layer 1 two at a time as packed f32 (adam_l1_ahead with adam2x / grad4x2,
csrc/sdxp_persist_adam.h: v_pk_mul_f32 / v_pk_fma_f32, one instruction for the same operation of two elements).  Every element keeps its operands,
its operations and its roundings:

    d_s = rn(dy_s gs)                                       gg = fma(d_3, x_3, fma(d_2, x_2, fma(d_1, x_1, fma(d_0, x_0, 0))))
    m = fma(0.1, gg, rn(0.9 m))                             v = fma(gg, rn(0.001 gg), rn(0.999 v))
    w = fma(-rn(lrb m), v_rcp(fma(isq, v_sqrt(v), 1e-8)), w)

The one-element form it replaced (adam1x, grad4 and the loop over the lane's 24 elements) is kept verbatim as the reference inside the test entry
sdxpk_packed_adam_check (csrc/sdxp_persist_checks.hip, built with the epoch kernel's flags): one workgroup of 512 threads standing for CU 37, an
LDS image [3][4][1024] for S.x1, per lane 8 elements x 3 networks of (w, m, v), column factors per lane, row factors per row; it hands back
(gg, m, v, w) of the one-element form and of the paired one.  Two cases: clip scales below 1, and clip scale 1.

Only the layer-1 update is paired in the kernel; layers 0 and 2 still run the one-element helpers and have no entry here.

(a) the inputs, asserted on the host: gradient elements of both signs over at least seven binades; exact zeros and -0.0 among x, dy, m, v, w;
    subnormal gg, m and v; second moments small enough (0, subnormal, 1e-36) that 1e-8 decides the denominator; different scalars for the actor /
    critic and the central value; NaN and inf among x, dy, m and v.
(b) the paired form against the one-element form, gg, m, v and w of all 2 x 12 288 elements: equal bit for bit where the reference is finite
    or inf, NaN where the reference is NaN (payloads are not compared).
(c) gg, m, v of the one-element form against the forms above in exact rational arithmetic on the host, rounded to float32 once per operation
    (the machinery of tests/test_gpu_persist_adam_ahead.py), bit for bit on every element with finite operands, subnormals included (only where an
    operation of the element underflows to zero is the zero's sign left out).  First the
    host shows that the inputs tell the forms apart: gg against multiply-then-add, m and v against the other contraction, each in at least 15 %
    of the elements."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_persist_adam_ahead import G, MB, NTH, U0, U1, F32, add, bits, fma, fr, mul, operands, rmul, rn  # noqa: E402

# SC_*: clip scale of actor-critic / central value, lr / (1 - b1^t) and 1 / sqrt(1 - b2^t) of the two optimisers (t = 3 and t = 5, lr 3e-4 and 5e-4)
_OPT = [3e-4 / (1 - 0.9 ** 3), 1 / np.sqrt(1 - 0.999 ** 3), 5e-4 / (1 - 0.9 ** 5), 1 / np.sqrt(1 - 0.999 ** 5)]
CASES = {"clipped": np.array([0.731, 0.412] + _OPT, F32), "clip scale 1": np.array([1.0, 1.0] + _OPT, F32)}
ZERO_COL, NEGZERO_COL, INF_COL = 7, 9, 13        # columns of S.x1 (row element 0 of lanes 7 / 9 / 13 of waves 0 and 4): +0, -0.0, inf in every sample
ZERO_LANE, NEGZERO_LANE, SUB_LANE, NAN_LANE = 5, 6, 11, 21   # threads whose column factors are +0 / -0.0 / subnormal / NaN
STATE_ROWS = {"m +0": 29, "m -0.0": 30, "v -0.0": 31, "w -0.0": 32, "m subnormal": 33, "v subnormal": 34, "m nan": 40, "v inf": 41, "m inf": 42}   # threads
V_SMALL = 1e-36                                  # a normal second moment with isq sqrt(v) far below 1e-8 2^-25


def inputs():
    """x1 [3][MB][U0], dy1 [3][MB][U1], dyr [3][MB][2], state [3: w, m, v][24][NTH]"""
    r = np.random.default_rng(5)
    x1 = (r.standard_normal((3, MB, U0)) * 2.0 ** (np.arange(U0) % 11 - 5)).astype(F32)              # rows: eleven binades of columns
    dy1 = (0.01 * r.standard_normal((3, MB, U1)) * 2.0 ** (np.arange(U1) % 16 - 8)).astype(F32)       # columns: sixteen binades of lanes
    dyr = (0.01 * r.standard_normal((3, MB, 2))).astype(F32)
    w = (0.1 * r.standard_normal((24, NTH))).astype(F32)
    m = (0.01 * r.standard_normal((24, NTH))).astype(F32)
    v = r.uniform(0.0, 1e-4, (24, NTH)).astype(F32)
    x1[:, :, 4 * G:4 * G + 4] = r.standard_normal((3, MB, 4)).astype(F32)                             # the columns every lane's column elements read
    x1[:, :, ZERO_COL], x1[:, :, NEGZERO_COL], x1[:, :, INF_COL] = 0.0, -0.0, np.inf
    dy1[:, :, ZERO_LANE], dy1[:, :, NEGZERO_LANE], dy1[:, :, NAN_LANE] = 0.0, -0.0, np.nan
    dy1[:, :, SUB_LANE] = (r.standard_normal((3, MB)) * 3e-41).astype(F32)
    for net in range(3):                                                                              # the column elements whose gg vanishes or is subnormal:
        c = slice(net * 8 + 4, net * 8 + 8)                                                           # v = 0, small, subnormal - the denominator is 1e-8
        v[c, ZERO_LANE], v[c, NEGZERO_LANE], v[c, SUB_LANE] = 0.0, V_SMALL, r.uniform(1e-44, 1e-40, 4).astype(F32)
    m[:, STATE_ROWS["m +0"]], m[:, STATE_ROWS["m -0.0"]], v[:, STATE_ROWS["v -0.0"]], w[:, STATE_ROWS["w -0.0"]] = 0.0, -0.0, -0.0, -0.0
    m[:, STATE_ROWS["m subnormal"]] = (r.standard_normal(24) * 1e-40).astype(F32)
    v[:, STATE_ROWS["v subnormal"]] = r.uniform(1e-44, 1e-40, 24).astype(F32)
    m[:, STATE_ROWS["m nan"]], v[:, STATE_ROWS["v inf"]], m[:, STATE_ROWS["m inf"]] = np.nan, np.inf, -np.inf
    return x1, dy1, dyr, np.stack([w, m, v])


def exact_forms(dy, x, net, state, scal):
    """(gg, m, v) of the stated forms, a mask of the elements whose operands are all finite, a mask of the elements in which some operation's
    exact result is not zero but rounds to zero (an underflow: the kernel's zero carries the sign of the exact result, the rational form's
    does not), and the fractions of the finite elements in which (multiply-then-add, the other contraction of m, of v) differ"""
    c09, c0999, c0001, c01 = float(F32(0.9)), float(F32(0.999)), float(F32(0.001)), float(F32(0.1))
    gg, mo, vo = np.zeros((24, NTH), F32), np.zeros((24, NTH), F32), np.zeros((24, NTH), F32)
    ok = np.isfinite(dy).all(-1) & np.isfinite(x).all(-1) & np.isfinite(state[1]) & np.isfinite(state[2])
    other, under = np.zeros(3), np.zeros((24, NTH), bool)
    lost = lambda exact: exact[0] != 0 and rn(exact) == 0          # a nonzero exact result that rounds to zero
    dy, x, state = dy.astype(np.float64), x.astype(np.float64), state.astype(np.float64)     # (exact: Python floats of the float32 values)
    for e in range(24):
        gs = float(scal[1] if net[e] == 2 else scal[0])
        for t in np.nonzero(ok[e])[0]:
            g, ga, u = 0.0, 0.0, False
            for s in range(MB):
                d = rmul(dy[e, t, s], gs)
                u |= lost(mul(fr(dy[e, t, s]), fr(gs))) or lost(add(mul(fr(d), fr(x[e, t, s])), fr(g)))
                g = fma(d, x[e, t, s], g)
                ga = rn(add(fr(rmul(d, x[e, t, s])), fr(ga)))
            m0, v0 = state[1, e, t], state[2, e, t]
            m = fma(c01, g, rmul(c09, m0))
            v = fma(g, rmul(c0001, g), rmul(c0999, v0))
            u |= lost(mul(fr(c09), fr(m0))) or lost(mul(fr(c0999), fr(v0))) or lost(mul(fr(c0001), fr(g)))
            u |= lost(add(mul(fr(c01), fr(g)), fr(rmul(c09, m0)))) or lost(add(mul(fr(g), fr(rmul(c0001, g))), fr(rmul(c0999, v0))))
            under[e, t] = u
            other += (ga != g, fma(c09, m0, rmul(c01, g)) != m, fma(c0999, v0, rmul(rmul(c0001, g), g)) != v)
            gg[e, t], mo[e, t], vo[e, t] = g, m, v
    return gg, mo, vo, ok, under, other / ok.sum()


_cache = {}


def _run():
    """(operands, {case: (out [2][4][24][NTH] of the test entry, host forms)}); computed once"""
    if not _cache:
        from seqdex_amd import _abi
        from seqdex_amd.sim import _stream_ptr
        lib, dev = _abi.load_library(), torch.device("cuda:0")
        lib.sdxpk_packed_adam_check.restype = C.c_int
        lib.sdxpk_packed_adam_check.argtypes = [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3
        x1, dy1, dyr, state = inputs()
        dy, x, net = operands(x1, dy1, dyr)
        d = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (x1, dy1, dyr, state)]
        res = {}
        for name, scal in CASES.items():
            sc = torch.from_numpy(scal).to(dev)
            out = torch.full((2, 4, 24, NTH), 12345.0, device=dev)
            assert lib.sdxpk_packed_adam_check(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), sc.data_ptr(), G, d[3].data_ptr(), out.data_ptr(), _stream_ptr(dev)) == 0
            torch.cuda.synchronize()
            res[name] = (out.cpu().numpy(), exact_forms(dy, x, net, state, scal))
        _cache["r"] = ((dy, x, net, state), res)
    return _cache["r"]


def _subnormal(a):
    return (a != 0) & (np.abs(a) < np.finfo(F32).tiny)


def _negzero(a):
    return (a == 0) & np.signbit(a)


def test_inputs_cover_the_stated_cases():
    (dy, x, net, state), res = _run()
    assert CASES["clipped"][0] < 1 and CASES["clipped"][1] < 1 and (CASES["clip scale 1"][:2] == 1).all()
    assert CASES["clipped"][2] != CASES["clipped"][4] and CASES["clipped"][3] != CASES["clipped"][5] and set(net) == {0, 1, 2}   # actor / critic and central value
    for a, what in ((x, "x"), (dy, "dy"), (state[1], "m"), (state[2], "v")):
        assert _negzero(a).any() and ((a == 0) & ~np.signbit(a)).any(), what
    assert _negzero(state[0]).any()
    assert _subnormal(state[1]).sum() >= 24 and _subnormal(state[2]).sum() >= 24 and _subnormal(dy).any()
    assert np.isnan(dy).any() and np.isinf(x).any() and np.isnan(state[1]).any() and np.isinf(state[1]).any() and np.isinf(state[2]).any()
    for name, (out, (gg, m, v, ok, _, other)) in res.items():
        g = gg[ok]
        for sign in (1, -1):
            e = np.floor(np.log2(np.abs(g[(sign * g > 0) & ~_subnormal(g)]).astype(np.float64)))
            print("%s: gg of sign %+d in %d binades (2^%d .. 2^%d)" % (name, sign, len(np.unique(e)), e.min(), e.max()))
            assert len(np.unique(e)) >= 7
        assert _subnormal(g).sum() >= 12 and (g == 0).sum() >= 24
        # 1e-8 decides the denominator: isq sqrt(v) below 2^-25 1e-8, so that fma(isq, sqrt(v), 1e-8) is 1e-8 itself
        tiny = ok & (np.sqrt(v.astype(np.float64)) * 1.01 * float(max(CASES[name][3], CASES[name][5])) < 2.0 ** -25 * 1e-8)
        print("%s: %d elements whose denominator is 1e-8, of them %d with v = 0, %d with subnormal v" % (name, tiny.sum(), (tiny & (v == 0)).sum(), (tiny & _subnormal(v)).sum()))
        assert (tiny & (v == 0)).sum() >= 12 and (tiny & _subnormal(v)).sum() >= 12 and (tiny & (v > 1e-37)).sum() >= 12
        print("%s: gg differs from multiply-then-add in %.1f %% of the elements, m from the other contraction in %.1f %%, v in %.1f %%" % ((name,) + tuple(100 * other)))
        assert (other >= 0.15).all(), other


def test_pairs_equal_the_one_element_form_bit_for_bit():
    _, res = _run()
    for name, (out, _) in res.items():
        assert not (out == 12345.0).any()                   # every slot was written by both forms
        assert np.isnan(out[0]).any() and np.isinf(out[0]).any() and np.isfinite(out[0]).mean() > 0.95
        for i, what in enumerate(("gg", "m", "v", "w")):
            ref, got = out[0, i], out[1, i]
            nan = np.isnan(ref)
            bad = np.argwhere(np.where(nan, ~np.isnan(got), bits(got) != bits(ref)))
            print("%s, %s: %d of %d elements of the paired form differ from the one-element form (%d NaN in both)" % (name, what, len(bad), ref.size, (nan & np.isnan(got)).sum()))
            assert len(bad) == 0, "%s %s: first (element, thread) %r: paired %r one-element %r" % (name, what, tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])


def test_one_element_form_has_the_stated_forms():
    _, res = _run()
    for name, (out, (gg, m, v, ok, under, _)) in res.items():
        assert 0 < under.sum() < 100                          # the underflowing elements are there, and they are few
        for what, got, want in (("gg", out[0, 0], gg), ("m", out[0, 1], m), ("v", out[0, 2], v)):
            # (+0 and -0: an exact zero has the same sign in the kernel and in the rational form; where an operation of the element underflows
            # the kernel's zero carries the sign of the exact result and the rational form has none: compare values there, bits elsewhere)
            bad = np.argwhere(ok & (bits(got) != bits(want)) & ~(under & (got == 0) & (want == 0)))
            print("%s, %s: %d of %d elements of the one-element form differ from the exact forms (%d elements with an underflow)" % (name, what, len(bad), ok.sum(), under.sum()))
            assert len(bad) == 0, "%s %s: first (element, thread) %r: kernel %r host %r" % (name, what, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
