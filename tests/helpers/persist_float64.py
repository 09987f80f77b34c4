"""What the tests of the persistent update kernel (csrc/sdxp_persist.hip) share: the shape it is built for, the layout of t["FACTORS"], and
a float64 torch forward / loss derivative / backward of ONE minibatch from the parameters and rows the kernel used.  k_update_persistent<true>
- forward + backward of one minibatch, the multi-rank factor path at world size 1 - leaves its factors in t["FACTORS"]; the tests compare them
with these, block by block and by name."""
import numpy as np
import pytest
import torch

N, MB, OBS, ST, ACT = 16, 4, 396, 564, 23
UNITS = (1024, 512, 256)
NETS = ("actor", "critic", "central value")


def persistent_or_skip(agent):
    if agent.update_impl() != "persistent":
        pytest.skip("persistent update kernel not selected on this device (needs >= 256 CUs)")


def factor_offsets():
    """layout of t["FACTORS"] (sdxp_create, csrc/sdxp_capi.hip): x[net][l], dy[net][l], h[net], dh -> ({net, l: x}, {net, l: dy}, {net: h}, dh)"""
    o, x, dy, h = 0, {}, {}, {}
    for net in range(3):
        for l in range(3):
            x[net, l] = o
            o += MB * ((ST if net == 2 else OBS) if l == 0 else UNITS[l - 1])
    for net in range(3):
        for l in range(3):
            dy[net, l] = o
            o += MB * UNITS[l]
    for net in range(3):
        h[net] = o
        o += MB * UNITS[2]
    return x, dy, h, o


def mlp(flat, o, in_dim, out_dim):
    """(trunk [(W, b)] x 3, head (W, b), offset behind the head) of one network in a flat float64 parameter array"""
    layers, k = [], in_dim
    for u in UNITS:
        layers.append((flat[o:o + u * k].reshape(u, k), flat[o + u * k:o + u * k + u]))
        o += u * k + u
        k = u
    head = (flat[o:o + out_dim * k].reshape(out_dim, k), flat[o + out_dim * k:o + out_dim * k + out_dim])
    return layers, head, o + out_dim * k + out_dim


class Minibatch0:
    """Parameters and rows of minibatch 0 of a filled rollout in float64, read BEFORE the kernel runs, and what k_update_persistent<true> left:
    F = t["FACTORS"], mu_k = the minibatch's rows of t["MB_MUS"] (update_mu_sigma: the kernel writes the new mu rows back).  Closes the agent."""

    def __init__(self, a):
        try:
            persistent_or_skip(a)
            a.backward_factors(-1)                     # begin of the epoch's update phase: cursor on minibatch 0
            torch.cuda.synchronize()
            f64 = lambda k: a.t[k].cpu().double()
            self.ac, self.cv = f64("AC_PARAMS"), f64("CV_PARAMS")
            rows = slice(0, MB)
            self.obs = f64("MB_OBS").reshape(-1, OBS)[rows]
            self.act = f64("MB_ACTIONS").reshape(-1, ACT)[rows]
            self.onlp, self.oval = f64("MB_NEGLOGP").reshape(-1)[rows], f64("MB_VALUES").reshape(-1)[rows]
            self.ret, self.adv = f64("RETURNS")[rows], f64("ADVANTAGES")[rows]
            a.backward_factors(0)
            torch.cuda.synchronize()
            self.F = a.t["FACTORS"].cpu()
            self.mu_k = a.t["MB_MUS"].cpu().reshape(-1, ACT)[rows]
            self.cfg = a.cfg
        finally:
            a.close()
        xo = factor_offsets()[0]
        # the layer-0 inputs the kernel used (central value: rows normalised by the running mean / std) are part of the factors
        self.x0 = [self.F[xo[net, 0]:xo[net, 0] + MB * (ST if net == 2 else OBS)].reshape(MB, -1) for net in range(3)]

    def forward(self):
        """float64 forward of the three networks on x0: sets nets[net] = trunk [(W, b)], heads[net] = head W, logstd, xs[net][l] = ELU output of
        trunk layer l, mu, vals = [critic value, central value]"""
        ac, cv = self.ac, self.cv
        actor, mu_head, o = mlp(ac, 0, OBS, ACT)
        self.logstd = ac[o:o + ACT]
        critic, v_head, o = mlp(ac, o + ACT, OBS, 1)
        assert o == ac.numel()
        cval, cv_head, o = mlp(cv, 0, ST, 1)
        assert o == cv.numel()
        self.nets, self.heads = (actor, critic, cval), (mu_head[0], v_head[0], cv_head[0])
        self.xs = []
        for net, layers in enumerate(self.nets):
            x, outs = self.x0[net].double(), []
            for W, b in layers:
                x = torch.nn.functional.elu(x @ W.T + b)
                outs.append(x)
            self.xs.append(outs)
        self.mu = self.xs[0][2] @ mu_head[0].T + mu_head[1]
        self.vals = [(self.xs[1][2] @ v_head[0].T + v_head[1]).reshape(-1), (self.xs[2][2] @ cv_head[0].T + cv_head[1]).reshape(-1)]
        return self

    def head_derivative(self):
        """[d loss / d mu (MB x ACT), d loss / d critic value (MB), d loss / d central value (MB)]: the loss phase of the kernel
        (csrc/sdxp_ppo_terms.h) in float64"""
        c, mu, logstd, adv = self.cfg, self.mu, self.logstd, self.adv
        e, inv_m = float(c.e_clip), 1.0 / MB
        sg = torch.exp(logstd)
        z = (self.act - mu) / sg
        nlp = (0.5 * z * z + logstd).sum(1) + 0.5 * np.log(2.0 * np.pi) * ACT
        ratio = torch.exp(self.onlp - nlp)
        l1, l2 = -adv * ratio, -adv * ratio.clamp(1.0 - e, 1.0 + e)
        gnlp = torch.where((l1 > l2) | ((ratio >= 1.0 - e) & (ratio <= 1.0 + e)), adv * ratio, torch.zeros_like(ratio))
        hi, lo = (mu - 1.1).clamp(min=0.0), (mu + 1.1).clamp(max=0.0)
        d_head = [gnlp[:, None] * (-(z / sg)) * inv_m + float(c.bounds_loss_coef) * (2.0 * hi + 2.0 * lo) * inv_m]
        for j, v in enumerate(self.vals):
            vc = self.oval + (v - self.oval).clamp(-e, e)
            c1, c2 = (v - self.ret) ** 2, (vc - self.ret) ** 2
            d = 2.0 * (v - self.ret)
            if c.clip_value:
                d = torch.where((c1 > c2) | ((v - self.oval).abs() <= e), d, torch.zeros_like(d))
            d_head.append((0.5 * float(c.critic_coef) if j == 0 else 1.0) * d * inv_m)
        return d_head

    def backward(self, d_head):
        """{(net, l): d loss / d (pre-activation) of trunk layer l}, from the head derivative down"""
        elu_g = lambda h: torch.where(h > 0, torch.ones_like(h), h + 1.0)      # elu' from the layer's output
        d_out = (d_head[0], d_head[1][:, None], d_head[2][:, None])
        dys = {}
        for net, layers in enumerate(self.nets):
            dx = d_out[net] @ self.heads[net]          # d loss / d x3
            for l in (2, 1, 0):
                dys[net, l] = dx * elu_g(self.xs[net][l])
                dx = dys[net, l] @ layers[l][0]
        return dys
