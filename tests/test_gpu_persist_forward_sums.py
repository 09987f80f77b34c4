"""-m gpu: where the forward phases of the persistent update kernel put their wave sums.  Forward L0 / L1 / L2 and the head forward reduce
twelve (wave 0 of the head forward: sixteen) partial dot products per wave with one butterfly (wave_sums, csrc/sdxp_persist.hip); lanes 0..3
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

from test_gpu_fullsize_properties import _filled_agent  # noqa: E402

N, MB, OBS, ST, ACT = 16, 4, 396, 564, 23
UNITS = (1024, 512, 256)
NETS = ("actor", "critic", "central value")
PARENT = {"actor x1": 1.8669e-07, "actor x2": 1.2093e-07, "actor h": 7.5992e-08,
          "critic x1": 2.2138e-07, "critic x2": 1.1805e-07, "critic h": 8.6248e-08,
          "central value x1": 1.7723e-07, "central value x2": 9.4556e-08, "central value h": 6.2729e-08,
          "mu": 3.9811e-08, "dh": 2.4885e-06}


def _factor_offsets():
    """layout of t["FACTORS"] (sdxp_create, csrc/sdxp_capi.hip): x[net][l], dy[net][l], h[net], dh"""
    o, x, h = 0, {}, {}
    for net in range(3):
        for l in range(3):
            x[net, l] = o
            o += MB * ((ST if net == 2 else OBS) if l == 0 else UNITS[l - 1])
    o += 3 * MB * sum(UNITS)                      # dy[net][l]
    for net in range(3):
        h[net] = o
        o += MB * UNITS[2]
    return x, h, o


def _mlp(flat, o, in_dim, out_dim):
    """(trunk [(W, b)] x 3, head (W, b), offset behind the head) of one network in a flat float64 parameter array"""
    layers, k = [], in_dim
    for u in UNITS:
        layers.append((flat[o:o + u * k].reshape(u, k), flat[o + u * k:o + u * k + u]))
        o += u * k + u
        k = u
    head = (flat[o:o + out_dim * k].reshape(out_dim, k), flat[o + out_dim * k:o + out_dim * k + out_dim])
    return layers, head, o + out_dim * k + out_dim


def measure():
    """name -> max |kernel - float64| of every block, for minibatch 0 of a filled rollout"""
    a = _filled_agent(N, 9)
    try:
        if a.update_impl() != "persistent":
            pytest.skip("persistent update kernel not selected on this device (needs >= 256 CUs)")
        a.backward_factors(-1)                     # begin of the epoch's update phase: cursor on minibatch 0
        torch.cuda.synchronize()
        f64 = lambda k: a.t[k].cpu().double()
        ac, cv = f64("AC_PARAMS"), f64("CV_PARAMS")
        rows = slice(0, MB)
        obs = f64("MB_OBS").reshape(-1, OBS)[rows]
        act = f64("MB_ACTIONS").reshape(-1, ACT)[rows]
        onlp, oval = f64("MB_NEGLOGP").reshape(-1)[rows], f64("MB_VALUES").reshape(-1)[rows]
        ret, adv = f64("RETURNS")[rows], f64("ADVANTAGES")[rows]
        a.backward_factors(0)
        torch.cuda.synchronize()
        F = a.t["FACTORS"].cpu()
        mu_k = a.t["MB_MUS"].cpu().reshape(-1, ACT)[rows]      # update_mu_sigma: the kernel writes the minibatch's new mu rows back
        c = a.cfg
    finally:
        a.close()
    xo, ho, dho = _factor_offsets()
    # the layer-0 inputs the kernel used (central value: rows normalised by the running mean / std) are part of the factors
    x0 = [F[xo[net, 0]:xo[net, 0] + MB * (ST if net == 2 else OBS)].reshape(MB, -1) for net in range(3)]
    np.testing.assert_array_equal(x0[0].numpy(), obs.float().numpy())
    np.testing.assert_array_equal(x0[1].numpy(), obs.float().numpy())
    actor, mu_head, o = _mlp(ac, 0, OBS, ACT)
    logstd = ac[o:o + ACT]
    critic, v_head, o = _mlp(ac, o + ACT, OBS, 1)
    assert o == ac.numel()
    cval, cv_head, o = _mlp(cv, 0, ST, 1)
    assert o == cv.numel()
    out, hs = {}, []
    for net, layers in enumerate((actor, critic, cval)):
        x = x0[net].double()
        for l, (W, b) in enumerate(layers):
            x = torch.nn.functional.elu(x @ W.T + b)
            if l < 2:
                got = F[xo[net, l + 1]:xo[net, l + 1] + MB * UNITS[l]].reshape(MB, UNITS[l])
            else:
                got = F[ho[net]:ho[net] + MB * UNITS[2]].reshape(MB, UNITS[2])
            assert float(got.abs().max()) > 0.05, (NETS[net], l)             # the block holds activations, not zeros
            out["%s %s" % (NETS[net], ("x1", "x2", "h")[l])] = float((got.double() - x).abs().max())
        hs.append(x)
    mu = hs[0] @ mu_head[0].T + mu_head[1]
    vals = [(hs[1] @ v_head[0].T + v_head[1]).reshape(-1), (hs[2] @ cv_head[0].T + cv_head[1]).reshape(-1)]
    out["mu"] = float((mu_k.double() - mu).abs().max())
    # d loss / d (mu, critic value, central value) of the minibatch: the loss phase of the kernel (csrc/sdxp_ppo_terms.h) in float64
    e, inv_m = float(c.e_clip), 1.0 / MB
    sg = torch.exp(logstd)
    z = (act - mu) / sg
    nlp = (0.5 * z * z + logstd).sum(1) + 0.5 * np.log(2.0 * np.pi) * ACT
    ratio = torch.exp(onlp - nlp)
    l1, l2 = -adv * ratio, -adv * ratio.clamp(1.0 - e, 1.0 + e)
    gnlp = torch.where((l1 > l2) | ((ratio >= 1.0 - e) & (ratio <= 1.0 + e)), adv * ratio, torch.zeros_like(ratio))
    hi, lo = (mu - 1.1).clamp(min=0.0), (mu + 1.1).clamp(max=0.0)
    want = torch.zeros(MB, 34, dtype=torch.float64)
    want[:, :ACT] = gnlp[:, None] * (-(z / sg)) * inv_m + float(c.bounds_loss_coef) * (2.0 * hi + 2.0 * lo) * inv_m
    for j, v in enumerate(vals):
        vc = oval + (v - oval).clamp(-e, e)
        c1, c2 = (v - ret) ** 2, (vc - ret) ** 2
        d = 2.0 * (v - ret)
        if c.clip_value:
            d = torch.where((c1 > c2) | ((v - oval).abs() <= e), d, torch.zeros_like(d))
        want[:, 32 + j] = (0.5 * float(c.critic_coef) if j == 0 else 1.0) * d * inv_m
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
