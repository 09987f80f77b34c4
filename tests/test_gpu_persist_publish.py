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

from test_gpu_fullsize_properties import _filled_agent  # noqa: E402
from test_gpu_persist_forward_sums import ACT, MB, N, NETS, OBS, ST, UNITS, _factor_offsets, _mlp  # noqa: E402

PARENT = {"actor dy0": 8.0969e-08, "actor dy1": 2.7807e-07, "actor dy2": 5.2252e-07,
          "critic dy0": 3.6606e-09, "critic dy1": 5.7088e-09, "critic dy2": 4.2670e-09,
          "central value dy0": 4.6104e-09, "central value dy1": 9.6785e-09, "central value dy2": 1.0588e-08}


def _dy_offsets():
    """dy[net][l] of t["FACTORS"] (sdxp_create, csrc/sdxp_capi.hip): behind the x[net][l] blocks"""
    xo, _, _ = _factor_offsets()
    o = xo[2, 2] + MB * UNITS[1]
    dy = {}
    for net in range(3):
        for l in range(3):
            dy[net, l] = o
            o += MB * UNITS[l]
    return dy


def measure():
    """name -> (max |kernel - float64|, max |kernel|) of every dy block, for minibatch 0 of a filled rollout"""
    a = _filled_agent(N, 9)
    try:
        if a.update_impl() != "persistent":
            pytest.skip("persistent update kernel not selected on this device (needs >= 256 CUs)")
        a.backward_factors(-1)                     # begin of the epoch's update phase: cursor on minibatch 0
        torch.cuda.synchronize()
        f64 = lambda k: a.t[k].cpu().double()
        ac, cv = f64("AC_PARAMS"), f64("CV_PARAMS")
        rows = slice(0, MB)
        act = f64("MB_ACTIONS").reshape(-1, ACT)[rows]
        onlp, oval = f64("MB_NEGLOGP").reshape(-1)[rows], f64("MB_VALUES").reshape(-1)[rows]
        ret, adv = f64("RETURNS")[rows], f64("ADVANTAGES")[rows]
        a.backward_factors(0)
        torch.cuda.synchronize()
        F = a.t["FACTORS"].cpu()
        c = a.cfg
    finally:
        a.close()
    xo, _, _ = _factor_offsets()
    dyo = _dy_offsets()
    x0 = [F[xo[net, 0]:xo[net, 0] + MB * (ST if net == 2 else OBS)].reshape(MB, -1).double() for net in range(3)]   # the layer-0 inputs the kernel used
    actor, mu_head, o = _mlp(ac, 0, OBS, ACT)
    logstd = ac[o:o + ACT]
    critic, v_head, o = _mlp(ac, o + ACT, OBS, 1)
    assert o == ac.numel()
    cval, cv_head, o = _mlp(cv, 0, ST, 1)
    assert o == cv.numel()
    nets = (actor, critic, cval)
    xs = []                                        # xs[net][l]: ELU output of trunk layer l
    for net, layers in enumerate(nets):
        x, outs = x0[net], []
        for W, b in layers:
            x = torch.nn.functional.elu(x @ W.T + b)
            outs.append(x)
        xs.append(outs)
    mu = xs[0][2] @ mu_head[0].T + mu_head[1]
    vals = [(xs[1][2] @ v_head[0].T + v_head[1]).reshape(-1), (xs[2][2] @ cv_head[0].T + cv_head[1]).reshape(-1)]
    # d loss / d (mu, critic value, central value): the loss phase of the kernel (csrc/sdxp_ppo_terms.h) in float64
    e, inv_m = float(c.e_clip), 1.0 / MB
    sg = torch.exp(logstd)
    z = (act - mu) / sg
    nlp = (0.5 * z * z + logstd).sum(1) + 0.5 * np.log(2.0 * np.pi) * ACT
    ratio = torch.exp(onlp - nlp)
    l1, l2 = -adv * ratio, -adv * ratio.clamp(1.0 - e, 1.0 + e)
    gnlp = torch.where((l1 > l2) | ((ratio >= 1.0 - e) & (ratio <= 1.0 + e)), adv * ratio, torch.zeros_like(ratio))
    hi, lo = (mu - 1.1).clamp(min=0.0), (mu + 1.1).clamp(max=0.0)
    dhead = [gnlp[:, None] * (-(z / sg)) * inv_m + float(c.bounds_loss_coef) * (2.0 * hi + 2.0 * lo) * inv_m]
    for j, v in enumerate(vals):
        vc = oval + (v - oval).clamp(-e, e)
        c1, c2 = (v - ret) ** 2, (vc - ret) ** 2
        d = 2.0 * (v - ret)
        if c.clip_value:
            d = torch.where((c1 > c2) | ((v - oval).abs() <= e), d, torch.zeros_like(d))
        dhead.append(((0.5 * float(c.critic_coef) if j == 0 else 1.0) * d * inv_m)[:, None])
    heads = (mu_head[0], v_head[0], cv_head[0])
    elu_g = lambda h: torch.where(h > 0, torch.ones_like(h), h + 1.0)      # elu' from the layer's output
    out = {}
    for net, layers in enumerate(nets):
        dx = dhead[net] @ heads[net]               # d loss / d x3
        for l in (2, 1, 0):
            dy = dx * elu_g(xs[net][l])
            got = F[dyo[net, l]:dyo[net, l] + MB * UNITS[l]].reshape(MB, UNITS[l]).double()
            out["%s dy%d" % (NETS[net], l)] = (float((got - dy).abs().max()), float(got.abs().max()))
            dx = dy @ layers[l][0]
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
        if a.update_impl() != "persistent":
            pytest.skip("persistent update kernel not selected on this device (needs >= 256 CUs)")
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
