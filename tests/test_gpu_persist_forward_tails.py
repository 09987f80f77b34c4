"""-m gpu: the publish tails of forward L0 / L1 / L2 of the persistent update kernel (csrc/sdxp_persist_tails.h: fwd_tail).  The waves of a CU leave
their partial dot products in S.fpart; wave 0 adds them, adds the bias, applies elu and publishes the three networks of a (sample, row) as one
packed word.  One lane per (network, sample, row) forms ONE output now - 48 / 24 / 12 lanes - and the networks meet in the storing lane through
v_permlane16_swap / v_permlane32_swap / row_shl, where one lane per (sample, row) formed the three networks one after the other.  Every lane
keeps the expression its output had, so the bits must not move:

    L0: (q[0] + q[1]) + bias      L1: (((q[0] + q[1]) + q[2]) + q[3]) + bias      L2: ((bias + q[0]) + q[1]) + ... + q[7]

The test entry sdxpk_forward_tail_check (csrc/sdxp_persist_checks.hip, built with the epoch kernel's flags) runs fwd_tail beside the former tail,
kept there verbatim, one workgroup per case.

(a) the packed values of the storing lanes: new == former, bit for bit - a network that reached the wrong lane or the wrong slot of the word shows
    here, the inputs of the three networks being unrelated;
(b) the pre-activations == sequential float32 adds on the host, bit for bit;
(c) asserted on the host first: another grouping of the same adds (a pairwise tree in front of the bias) differs in more than a third of the cases
    of L1 and L2 - a case is one workgroup, 24 / 12 lanes of five / nine operands each; per lane, with so few operands, a regrouping shows in about
    one lane in twenty (L1) and one in three (L2), both printed - so a regrouped sum could not pass (b);
(d) asserted on the host first: the pre-activations cover > 0, (-17, 0), +0.0, -0.0 and < -17 (where elu has reached -1), each at least
    five times per layer.

Inputs as in test_gpu_persist_ordered_sum.py: 13 random significant bits at exponents spread over 2^-12 .. 2^12, mixed signs.  Case 0 is all
-0.0 (every pre-activation -0.0), case 1 holds terms that cancel in pairs with a +0.0 bias (+0.0), cases 2..9 keep their exponents below 2^3 so
that sums between -17 and 0 are common.

The last test runs the epoch kernel at 16 actors x horizon 8 (160 optimiser steps): two handles from one state must end bit-identical in
parameters, moments and control block, and within 1e-4 of the hipGraph path (the bound of tests/test_gpu_ppo_parity.py at this size) - the tails,
the head forward and the statistics thread of every step are in it."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from helpers.persist_float64 import MB, N, persistent_or_skip  # noqa: E402
from test_gpu_fullsize_properties import _filled_agent  # noqa: E402

NWV, CASES = 8, 48
TERMS = {0: 2, 1: 4, 2: 8}
LANES = {0: 48, 1: 24, 2: 12}
STORING = {0: 16, 1: 8, 2: 4}
BIAS0 = {0: 0, 1: 12, 2: 18}            # BIAS_L0, BIAS_L1, BIAS_L2 (csrc/sdxp_persist_lds.h)


def _values(r, shape, emin=-24, emax=0):
    m = r.integers(1 << 12, 1 << 13, size=shape).astype(np.float64)
    return (m * 2.0 ** r.integers(emin, emax + 1, size=shape) * r.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def _inputs(layer):
    r = np.random.default_rng(11 + layer)
    fpart, bias = _values(r, (CASES, 3 * MB * NWV)), _values(r, (CASES, 64))
    fpart[2:10], bias[2:10] = _values(r, (8, 3 * MB * NWV), -24, -10), _values(r, (8, 64), -24, -10)
    fpart[0], bias[0] = -0.0, -0.0
    a = np.abs(fpart[1, 0::2])
    fpart[1, 0::2], fpart[1, 1::2], bias[1] = a, -a, 0.0
    return fpart, bias


def _bias_slot(layer, lane):
    net = lane // (LANES[layer] // 3)
    return BIAS0[layer] + (net * 4 + lane % 4 if layer == 0 else net * 2 + lane % 2 if layer == 1 else net)


def _operands(layer, fpart, bias):
    """q [CASES][lanes][terms], b [CASES][lanes]: lane (net, s, r) reads S.fpart[(net MB + s) NWV + terms r ..] = S.fpart[terms lane ..]"""
    t, lanes = TERMS[layer], LANES[layer]
    q = fpart[:, :t * lanes].reshape(CASES, lanes, t)
    b = bias[:, [_bias_slot(layer, l) for l in range(lanes)]]
    return q, b


def _sequential(layer, q, b):
    if layer == 2:
        t = b.copy()
        for w in range(q.shape[2]):
            t = (t + q[:, :, w]).astype(np.float32)
        return t
    t = q[:, :, 0].copy()
    for w in range(1, q.shape[2]):
        t = (t + q[:, :, w]).astype(np.float32)
    return (t + b).astype(np.float32)


def _tree(q, b):
    x = q.copy()
    while x.shape[2] > 1:
        x = (x[:, :, 0::2] + x[:, :, 1::2]).astype(np.float32)
    return (x[:, :, 0] + b).astype(np.float32)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("layer", [0, 1, 2])
def test_one_network_per_lane_publishes_the_former_words(layer):
    from seqdex_amd import _abi
    from seqdex_amd.sim import _stream_ptr
    lib, dev = _abi.load_library(), torch.device("cuda:0")
    lib.sdxpk_forward_tail_check.restype = C.c_int
    lib.sdxpk_forward_tail_check.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    fpart, bias = _inputs(layer)
    q, b = _operands(layer, fpart, bias)
    want = _sequential(layer, q, b)
    lanes, st = LANES[layer], STORING[layer]
    # (d) the branches of elu and both zeros
    wb = _bits(want)
    kinds = {"> 0": int((want > 0).sum()), "(-17, 0)": int(((want < 0) & (want > -17)).sum()), "+0.0": int((wb == 0).sum()),
             "-0.0": int((wb == np.int32(-2 ** 31)).sum()), "< -17": int((want < -17).sum())}
    print("layer %d: pre-activations of %d lanes: %s" % (layer, want.size, kinds))
    assert all(v >= 5 for v in kinds.values()), kinds
    # (c) the order of the adds shows in the bits
    if layer > 0:
        moved = _bits(_tree(q, b)) != wb
        print("layer %d: a pairwise tree in front of the bias differs from the kernel's order in %d of %d lanes, in %d of %d cases" % (
            layer, int(moved.sum()), want.size, int(moved.any(axis=1).sum()), CASES))
        assert 3 * int(moved.any(axis=1).sum()) > CASES
    d_f, d_b = torch.from_numpy(fpart).to(dev), torch.from_numpy(bias).to(dev)
    ref, got, pre = (torch.full((CASES, 48), float("nan"), device=dev) for _ in range(3))
    assert lib.sdxpk_forward_tail_check(layer, d_f.data_ptr(), d_b.data_ptr(), CASES, ref.data_ptr(), got.data_ptr(), pre.data_ptr(), _stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    ref, got, pre = (x.cpu().numpy() for x in (ref, got, pre))
    # (b)
    print("layer %d: pre-activations against the host: %d of %d differ in bits" % (layer, int((_bits(pre[:, :lanes]) != wb).sum()), want.size))
    np.testing.assert_array_equal(_bits(pre[:, :lanes]), wb)
    assert np.isnan(pre[:, lanes:]).all()
    # (a)
    assert not np.isnan(ref[:, :3 * st]).any() and np.isnan(ref[:, 3 * st:]).all() and np.isnan(got[:, 3 * st:]).all()
    print("layer %d: packed values, one network per lane against one lane per word: %d of %d differ in bits" % (
        layer, int((_bits(got[:, :3 * st]) != _bits(ref[:, :3 * st])).sum()), CASES * 3 * st))
    np.testing.assert_array_equal(_bits(got[:, :3 * st]), _bits(ref[:, :3 * st]))
    # the word of storing lane l holds the outputs of lanes l, l + st, l + 2 st: elu of exactly those pre-activations (x above 0, -1 below -18: 1 - e^-18 rounds to 1)
    word = ref[:, :3 * st].reshape(CASES, st, 3)
    for net in range(3):
        p = want[:, net * st:(net + 1) * st]
        np.testing.assert_array_equal(word[:, :, net][p > 0], p[p > 0])
        assert (word[:, :, net][p < -18] == -1.0).all()
        assert ((word[:, :, net] <= 0) == (p <= 0)).all()


def test_epoch_kernel_twice_bit_identical_and_within_the_graph_paths_bound():
    a = _filled_agent(N, 9)
    b = _filled_agent(N, 9)
    c = _filled_agent(N, 9, impl="graph")
    try:
        persistent_or_skip(a)
        assert b.update_impl() == "persistent" and c.update_impl() == "graph"
        p0 = a.t["AC_PARAMS"].clone()
        for ag in (a, b, c):
            ag.update()
        torch.cuda.synchronize()
        ca, cb, cc = a.ctrl(), b.ctrl(), c.ctrl()
        assert a.update_impl() == "persistent" and ca.ac_t == cb.ac_t == cc.ac_t == 5 * (N * 8 // MB) == 160
        for k in ("AC_PARAMS", "CV_PARAMS", "AC_ADAM_M", "AC_ADAM_V", "CV_ADAM_M", "CV_ADAM_V", "MB_MUS", "MB_SIGMAS"):
            np.testing.assert_array_equal(a.t[k].cpu().numpy().view(np.int32), b.t[k].cpu().numpy().view(np.int32), err_msg=k)
        assert bytes(ca) == bytes(cb)                                           # the control block: running sums, last_kl, lr, counters, tags
        assert float((a.t["AC_PARAMS"] - p0).abs().max()) > 1e-4              # the epoch did something
        d_ac = float((a.t["AC_PARAMS"] - c.t["AC_PARAMS"]).abs().max())
        d_cv = float((a.t["CV_PARAMS"] - c.t["CV_PARAMS"]).abs().max())
        print("persistent against hipGraph after 160 steps: max |diff| actor-critic %.3e, central value %.3e (bound 1e-4)" % (d_ac, d_cv))
        assert d_ac < 1e-4 and d_cv < 1e-4, (d_ac, d_cv)
    finally:
        a.close(); b.close(); c.close()
