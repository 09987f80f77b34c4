"""-m gpu: where the forward phases of the persistent update kernel put their wave sums.  Forward L0 / L1 / L2 and the head forward reduce
twelve (wave 0 of the head forward: sixteen) partial dot products per wave with one butterfly (wave_sums, csrc/sdxp_persist_sums.h); lanes 0..3
store sample `lane` of three networks (or of the wave's head rows).  A value stored to the wrong (net, sample) or (row, sample) slot does not
crash anything: it shows as one wrong block of activations.  This test runs k_update_persistent<true> - forward + backward of ONE minibatch,
the multi-rank factor path at world size 1, same forward code as the epoch kernel - and compares, block by block and by name, what it left in
t["FACTORS"] (x1, x2, h = x3 of actor, critic and central value, and dh = d loss / d head outputs) and the mu rows it wrote to t["MB_MUS"]
with a float64 torch forward (and loss derivative) of the same parameters on the same four rows.

Bounds.  max |kernel - float64| per block, measured on the commit BEFORE the butterfly (twelve wave_sum trees, lane 0 stores), same seeds:

    actor x1 1.8669e-07          actor x2 1.2093e-07          actor h 7.5992e-08
    critic x1 2.2138e-07         critic x2 1.1805e-07         critic h 8.6248e-08
    central value x1 1.7723e-07  central value x2 9.4556e-08  central value h 6.2729e-08
    mu 3.9811e-08                dh 2.4885e-06

The test allows four times these figures: sums of <= 1 024 fp32 terms move in their last bits between builds of the reference, a misplaced
value moves by the size of an activation (0.1 .. 1).  The butterfly keeps every sum's pairs, so it measures the same figures.  (Forward L2
keeps its twelve wave_sum trees: its values are bare products w2 * x2, which the compiler contracts with the tree's first add into one fma
per lane; through the butterfly the same sums came out as actor h 7.6205e-08, central value h 6.8294e-08, mu 5.2881e-08 - inside the bound
and still not the bits of before.)"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from helpers.persist_float64 import ACT, MB, N, NETS, UNITS, Minibatch0, factor_offsets  # noqa: E402
from test_gpu_fullsize_properties import _filled_agent  # noqa: E402

PARENT = {"actor x1": 1.8669e-07, "actor x2": 1.2093e-07, "actor h": 7.5992e-08,
          "critic x1": 2.2138e-07, "critic x2": 1.1805e-07, "critic h": 8.6248e-08,
          "central value x1": 1.7723e-07, "central value x2": 9.4556e-08, "central value h": 6.2729e-08,
          "mu": 3.9811e-08, "dh": 2.4885e-06}


def measure():
    """name -> max |kernel - float64| of every block, for minibatch 0 of a filled rollout"""
    m = Minibatch0(_filled_agent(N, 9))
    F = m.F
    xo, _, ho, dho = factor_offsets()
    np.testing.assert_array_equal(m.x0[0].numpy(), m.obs.float().numpy())
    np.testing.assert_array_equal(m.x0[1].numpy(), m.obs.float().numpy())
    m.forward()
    out = {}
    for net in range(3):
        for l in range(3):
            if l < 2:
                got = F[xo[net, l + 1]:xo[net, l + 1] + MB * UNITS[l]].reshape(MB, UNITS[l])
            else:
                got = F[ho[net]:ho[net] + MB * UNITS[2]].reshape(MB, UNITS[2])
            assert float(got.abs().max()) > 0.05, (NETS[net], l)             # the block holds activations, not zeros
            out["%s %s" % (NETS[net], ("x1", "x2", "h")[l])] = float((got.double() - m.xs[net][l]).abs().max())
    out["mu"] = float((m.mu_k.double() - m.mu).abs().max())
    d_head = m.head_derivative()
    want = torch.zeros(MB, 34, dtype=torch.float64)
    want[:, :ACT] = d_head[0]
    for j in range(2):
        want[:, 32 + j] = d_head[1 + j]
    dh = F[dho:dho + MB * 34].reshape(MB, 34)
    assert float(dh[:, :ACT].abs().max()) > 1e-3 and float(dh[:, 32].abs().max()) > 0.0 and float(dh[:, 33].abs().max()) > 0.0
    out["dh"] = float((dh.double() - want).abs().max())
    return out


def test_forward_blocks_and_head_outputs_against_float64():
    got = measure()
    assert set(got) == set(PARENT)
    for name in PARENT:
        print("%-18s max |kernel - float64| %.3e (before the butterfly %.3e, bound %.3e)" % (name, got[name], PARENT[name], 4.0 * PARENT[name]))
    for name in PARENT:
        assert got[name] <= 4.0 * PARENT[name], (name, got[name], PARENT[name])
