"""-m gpu: the backward phases of the persistent update kernel publish from their reducing lanes.  Backward L2 and backward L1
(csrc/sdxp_persist.hip) end in a reduction over the workgroup's 32 DPP rows; the lanes of wave 0 that add the row sums - (net, sample, column)
= lane - apply elu' to their own sum, store it for the CU's own Adam (dyown) and hand the three networks of one (sample, column) to ONE lane
by cross-lane moves (row_shl:8, v_permlane16_swap, v_permlane32_swap), which publishes the packed word in front of the reduction's closing
barrier.  A network handed to the wrong slot of the word does not crash anything: it shows as one wrong block of gradient factors; a barrier
that is missing shows as two runs that differ.

(a) k_update_persistent<true> - forward + backward of ONE minibatch, the multi-rank factor path at world size 1, same backward code as the
epoch kernel, and the instantiation whose dY0 words take the permlane path - against a float64 backward of the same parameters on the same
four rows: the blocks dy[net][l] of t["FACTORS"], l = 0, 1, 2, by name.  max |kernel - float64| per block, measured with measure() below on
the commit BEFORE this change (reduction -> S.part -> barrier -> read-back by threads 0..7 / 0..15), same seeds:

    actor dy0 8.0969e-08          actor dy1 2.7807e-07          actor dy2 5.2252e-07
    critic dy0 3.6606e-09         critic dy1 5.7088e-09         critic dy2 4.2670e-09
    central value dy0 4.6104e-09  central value dy1 9.6785e-09  central value dy2 1.0588e-08

The test allows four times these figures (sums of <= 512 fp32 terms move in their last bits between builds of the reference; a misplaced
network moves a block by the size of its entries, 1e-2 .. 3e-1 here) and requires every block to be non-zero.  This change keeps every sum's
order, so it measures the same figures.

(b) the epoch kernel at N = 16 x horizon 8 (160 optimiser steps): two handles from one state must end bit-identical in parameters, Adam
moments (logstd and its moments are part of them) and the rewritten mu / sigma rows - every cross-wave hand-over of the step sits behind a
barrier or inside one wave, so nothing may depend on timing - and within 1e-4 of the hipGraph path, the bound tests/test_gpu_ppo_parity.py
holds the fused and the explicit path to at this size."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from helpers.persist_float64 import MB, N, NETS, UNITS, Minibatch0, factor_offsets, persistent_or_skip  # noqa: E402
from test_gpu_fullsize_properties import _filled_agent  # noqa: E402

PARENT = {"actor dy0": 8.0969e-08, "actor dy1": 2.7807e-07, "actor dy2": 5.2252e-07,
          "critic dy0": 3.6606e-09, "critic dy1": 5.7088e-09, "critic dy2": 4.2670e-09,
          "central value dy0": 4.6104e-09, "central value dy1": 9.6785e-09, "central value dy2": 1.0588e-08}


def measure():
    """name -> (max |kernel - float64|, max |kernel|) of every dy block, for minibatch 0 of a filled rollout"""
    m = Minibatch0(_filled_agent(N, 9))
    dyo = factor_offsets()[1]
    dys = m.forward().backward(m.head_derivative())
    out = {}
    for net in range(3):
        for l in (2, 1, 0):
            got = m.F[dyo[net, l]:dyo[net, l] + MB * UNITS[l]].reshape(MB, UNITS[l]).double()
            out["%s dy%d" % (NETS[net], l)] = (float((got - dys[net, l]).abs().max()), float(got.abs().max()))
    return out


def test_backward_factor_blocks_against_float64():
    got = measure()
    assert set(got) == set(PARENT)
    for name in PARENT:
        print("%-18s max |kernel - float64| %.4e (before the change %.4e, bound %.4e), max |kernel| %.3e" % (
            name, got[name][0], PARENT[name], 4.0 * PARENT[name], got[name][1]))
    for name in PARENT:
        assert got[name][1] > 0.0, name                                     # the block holds gradients, not zeros
        assert got[name][0] <= 4.0 * PARENT[name], (name, got[name], PARENT[name])


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
        assert a.update_impl() == "persistent" and a.ctrl().ac_t == b.ctrl().ac_t == c.ctrl().ac_t == 5 * (N * 8 // MB) == 160
        for k in ("AC_PARAMS", "CV_PARAMS", "AC_ADAM_M", "AC_ADAM_V", "CV_ADAM_M", "CV_ADAM_V", "MB_MUS", "MB_SIGMAS"):
            np.testing.assert_array_equal(a.t[k].cpu().numpy().view(np.int32), b.t[k].cpu().numpy().view(np.int32), err_msg=k)
        assert float((a.t["AC_PARAMS"] - p0).abs().max()) > 1e-4              # the epoch did something
        d_ac = float((a.t["AC_PARAMS"] - c.t["AC_PARAMS"]).abs().max())
        d_cv = float((a.t["CV_PARAMS"] - c.t["CV_PARAMS"]).abs().max())
        print("persistent against hipGraph after 160 steps: max |diff| actor-critic %.3e, central value %.3e (bound 1e-4)" % (d_ac, d_cv))
        assert d_ac < 1e-4 and d_cv < 1e-4, (d_ac, d_cv)
    finally:
        a.close(); b.close(); c.close()
