"""-m gpu: the loss phase of the persistent update kernel (phase D, between the head forward and the heads' backward; csrc/sdxp_persist_phase_d.h:
loss_request, loss_front, loss_back).  The new form asks for the z chain's operands early, forms the two value-head losses on eight lanes of wave 3
instead of behind the ratio on lane (s, 31), and lets the dmu thread divide z by sigma and form the bounds term in front of the first barrier, so
that behind it only S.gnlp[s] is read.  Every expression keeps its operands, order and contraction, so the bits must be the former block's.

The test entry sdxpk_loss_phase_check (csrc/sdxp_persist_checks.hip, built with the epoch kernel's flags) runs the helpers beside the former block, kept
there verbatim: one workgroup of 512 threads per case; S.gnlp, S.dv, S.dmu, S.dls, the three S.stat columns of the phase and S.z out.

(a) new == former, bit for bit, every output (the padding lanes a >= 23 of S.z, S.dmu and S.dls included: zeros; S.mu holds NaN there, so a padding
    lane that used what it read would show);
(b) both against a float32 numpy restatement of sdxp_ppo_terms.h.  Bit for bit where the kernel's ISA fixes every rounding and the operations are
    correctly rounded: S.z (one subtraction, one IEEE division), S.dv and the critic / central-value columns of S.stat (subtractions, min / max, bare
    products - nothing an fma could take), and - from the DEVICE's S.gnlp - S.dmu = fma(bt, 1/4, -rn(rn(gnlp q) / 4)), q = rn(z / sigma),
    bt = rn(bounds_coef rn(2 hi + 2 lo)), and S.dls = the chain fma(rn(gnlp_s rn(1 - z_s^2)), 1/4, .) from 0 in ascending s (each fma evaluated in
    float64 and rounded once: the products are exact there).  S.gnlp and the actor column go through expf: the sample's -log p is restated exactly
    (fma(z, rn(z / 2), logstd) per action, the half-wave butterfly is a balanced pairwise tree), and the ratio is held to float64 exp within 4 ulp
    (2^-21 relative: expf 1 ulp, the float64 value rounded 1/2, the product with the advantage 1/2 each side).
(c) cases, each asserted on the host before the launch: ratio below, inside and above the clip band with both signs of the advantage; clip_value on
    and off; |v - vo| inside and outside e_clip for both value heads; mu beyond +1.1, beyond -1.1 and inside; bounds_coef 0 and non-zero."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MB, A, CASES = 4, 23, 6
F = np.float32
E_CLIP, CRITIC_COEF = F(0.2), F(4.0)
LOSS_IN = 2 * MB * 32 + 64 + 2 * MB + 4 * MB + 4
LOSS_OUT = MB + 2 * MB + MB * 32 + 32 + MB * 3 + MB * 32
NLP_CONST = F(F(0.5) * F(1.8378770664093453)) * F(A)
# (ratio, sign of the advantage) per (case, sample): every combination of below / inside / above with both signs occurs four times
RATIO = np.array([[0.7, 0.7, 1.05, 1.05], [1.4, 1.4, 0.95, 0.6], [1.3, 1.1, 0.75, 0.9], [0.7, 1.4, 1.05, 1.05], [1.4, 0.7, 0.95, 1.3], [0.65, 1.35, 1.0, 0.85]])
ADV_SIGN = np.array([[1, -1, 1, -1], [1, -1, 1, -1], [-1, 1, 1, -1], [-1, 1, -1, 1], [-1, 1, -1, 1], [1, -1, 1, -1]])
CLIP_VALUE = [1, 1, 0, 0, 1, 0]
BOUNDS_COEF = [0.0, 1e-4, 0.0, 1e-4, 0.37, 0.37]
# v - vo of the two value heads per sample: inside and outside e_clip, both heads, both signs
DV = np.array([[[0.05, -0.5, 0.5, -0.05], [0.5, 0.05, -0.05, -0.5]]] * CASES)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _nlp(act, mu, sg, ls):
    """z [.., MB, 32] and the sample's -log p [.., MB] as the kernel forms them"""
    z = np.zeros_like(act)
    z[..., :A] = ((act[..., :A] - mu[..., :A]).astype(F) / sg[..., None, :A]).astype(F)
    t = np.zeros_like(act)
    t[..., :A] = _fma(z[..., :A], (F(0.5) * z[..., :A]).astype(F), np.broadcast_to(ls[..., None, :A], z[..., :A].shape))
    while t.shape[-1] > 1:
        t = (t[..., 0::2] + t[..., 1::2]).astype(F)
    return z, (t[..., 0] + NLP_CONST).astype(F)


def _inputs():
    r = np.random.default_rng(11)
    ls = np.zeros((CASES, 32), F); ls[:, :A] = r.uniform(-1.2, 0.1, (CASES, A))
    sg = np.exp(ls.astype(np.float64)).astype(F); sg[:, A:] = 1.0
    mu = np.full((CASES, MB, 32), np.nan, F)
    mu[:, :, :A] = r.uniform(-1.0, 1.0, (CASES, MB, A))
    mu[:, :, 0] = 1.5; mu[:, :, 5] = -1.7; mu[:, 1, 11] = 2.2; mu[:, 2, 22] = -1.1005
    act = np.zeros((CASES, MB, 32), F)
    act[:, :, :A] = mu[:, :, :A] + sg[:, None, :A] * r.standard_normal((CASES, MB, A)) * 0.3
    _, nlp = _nlp(act, mu, sg, ls)
    old_nlp = (nlp.astype(np.float64) + np.log(RATIO)).astype(F)
    adv = (ADV_SIGN * r.uniform(0.2, 2.0, (CASES, MB))).astype(F)
    vo = r.uniform(-1.0, 1.0, (CASES, MB)).astype(F)
    val = (vo[:, None, :] + DV).astype(F)
    ret = (vo + r.uniform(-0.6, 0.6, (CASES, MB))).astype(F)
    x = np.zeros((CASES, LOSS_IN), F)
    x[:, :128] = act.reshape(CASES, -1); x[:, 128:256] = mu.reshape(CASES, -1); x[:, 256:288] = ls; x[:, 288:320] = sg
    x[:, 320:328] = val.reshape(CASES, -1)
    x[:, 328:344] = np.stack([adv, old_nlp, ret, vo], 1).reshape(CASES, -1)
    x[:, 344] = E_CLIP; x[:, 345] = CRITIC_COEF; x[:, 346] = BOUNDS_COEF; x[:, 347] = CLIP_VALUE
    return x, dict(act=act, mu=mu, ls=ls, sg=sg, val=val, adv=adv, old_nlp=old_nlp, ret=ret, vo=vo)


def _split(o):
    i = np.cumsum([0, MB, 2 * MB, MB * 32, 32, MB * 3, MB * 32])
    return dict(gnlp=o[..., i[0]:i[1]], dv=o[..., i[1]:i[2]].reshape(o.shape[:-1] + (2, MB)), dmu=o[..., i[2]:i[3]].reshape(o.shape[:-1] + (MB, 32)),
                dls=o[..., i[3]:i[4]], stat=o[..., i[4]:i[5]].reshape(o.shape[:-1] + (MB, 3)), z=o[..., i[5]:i[6]].reshape(o.shape[:-1] + (MB, 32)))


def test_loss_phase_keeps_the_bits():
    from seqdex_amd import _abi
    from seqdex_amd.sim import _stream_ptr
    lib, dev = _abi.load_library(), torch.device("cuda:0")
    lib.sdxpk_loss_phase_check.restype = C.c_int
    lib.sdxpk_loss_phase_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    x, d = _inputs()
    e, bc, cv = E_CLIP, np.array(BOUNDS_COEF, F), np.array(CLIP_VALUE, bool)
    # ---- numpy restatement and (c) the census of the cases
    z, nlp = _nlp(d["act"], d["mu"], d["sg"], d["ls"])
    arg = (d["old_nlp"] - nlp).astype(F)
    ratio = np.exp(arg.astype(np.float64))
    lo_b, hi_b = float(F(1.0) - e), float(F(1.0) + e)
    assert (np.abs(ratio - lo_b) > 0.02).all() and (np.abs(ratio - hi_b) > 0.02).all()        # no ratio near an edge of the band: 4 ulp cannot flip a branch
    for below, above in ((True, False), (False, False), (False, True)):
        for sign in (1, -1):
            assert (((ratio < lo_b) == below) & ((ratio > hi_b) == above) & (np.sign(d["adv"]) == sign)).any(), (below, above, sign)
    assert cv.any() and (~cv).any() and (bc == 0).any() and (bc != 0).any()
    dvo = (d["val"] - d["vo"][:, None, :]).astype(F)
    for j in range(2):
        assert (np.abs(dvo[cv, j]) < e - 0.01).any() and (np.abs(dvo[cv, j]) > e + 0.01).any() and (np.abs(np.abs(dvo[:, j]) - e) > 0.01).all()
    m = d["mu"][:, :, :A]
    assert (m > 1.1).any() and (m < -1.1).any() and (np.abs(m) < 1.1).any() and np.isnan(d["mu"][:, :, A:]).all()
    for c in range(CASES):
        assert (m[c] > 1.1).any() and (m[c] < -1.1).any()
    # value heads
    R, vo = d["ret"][:, None, :], d["vo"][:, None, :]
    v = d["val"]
    vc = (vo + np.minimum(e, np.maximum(-e, (v - vo).astype(F)))).astype(F)
    c1 = ((v - R).astype(F) * (v - R).astype(F)).astype(F); c2 = ((vc - R).astype(F) * (vc - R).astype(F)).astype(F)
    two = (F(2.0) * (v - R).astype(F)).astype(F)
    dcl = np.where((c1 > c2) | (np.abs((v - vo).astype(F)) <= e), two, F(0.0))
    dd = np.where(cv[:, None, None], dcl, two).astype(F)
    closs = np.where(cv[:, None, None], np.maximum(c1, c2), c1).astype(F)
    coef = np.array([F(0.5) * CRITIC_COEF, F(1.0)], F)[None, :, None]
    dv_ref = ((coef * dd).astype(F) * F(0.25)).astype(F)
    # ---- launch
    xin = torch.from_numpy(x).to(dev)
    out = torch.full((CASES, 2, LOSS_OUT), float("nan"), device=dev)
    assert lib.sdxpk_loss_phase_check(xin.data_ptr(), CASES, out.data_ptr(), _stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    i32 = lambda a: np.ascontiguousarray(a).view(np.int32)
    former, new = _split(out[:, 0]), _split(out[:, 1])
    for k in former:
        print("%-5s new against former: %d of %d values differ in bits" % (k, int((i32(new[k]) != i32(former[k])).sum()), new[k].size))
    assert not np.isnan(out).any()
    # (b) bit for bit
    gn = former["gnlp"]                                                                        # the device's
    q = (z / d["sg"][:, None, :]).astype(F)
    t = ((gn[:, :, None] * q).astype(F) * F(0.25)).astype(F)
    hi = np.maximum((d["mu"] + F(-1.1)).astype(F), F(0.0)); lo = np.minimum((d["mu"] + F(1.1)).astype(F), F(0.0))
    bt = (bc[:, None, None] * _fma(F(2.0), hi, (lo + lo).astype(F))).astype(F)
    dmu_ref = np.zeros((CASES, MB, 32), F)
    dmu_ref[:, :, :A] = _fma(bt[:, :, :A], F(0.25), -t[:, :, :A])
    dls_ref = np.zeros((CASES, 32), F)
    for s in range(MB):
        p = (gn[:, s, None] * _fma(-z[:, s, :A], z[:, s, :A], F(1.0))).astype(F)
        dls_ref[:, :A] = _fma(p, F(0.25), dls_ref[:, :A])
    exact = dict(z=z, dv=dv_ref, dmu=dmu_ref, dls=dls_ref)
    for k, ref in exact.items():
        print("%-5s former against numpy: %d of %d values differ in bits" % (k, int((i32(former[k]) != i32(ref)).sum()), ref.size))
    print("stat  critic / central-value columns against numpy: %d of %d differ in bits" % (int((i32(former["stat"][:, :, 1:]) != i32(closs.transpose(0, 2, 1))).sum()), closs.size))
    # gnlp and the actor column: within 4 ulp of float64
    adv = d["adv"].astype(np.float64)
    L1, L2 = -adv * ratio, -adv * np.clip(ratio, lo_b, hi_b)
    gn_ref = np.where((L1 > L2) | ((ratio >= lo_b) & (ratio <= hi_b)), adv * ratio, 0.0)
    act_ref = np.maximum(L1, L2)
    tol = 2.0 ** -21
    eg, ea = np.abs(gn - gn_ref) / np.maximum(np.abs(adv * ratio), 1e-30), np.abs(former["stat"][:, :, 0] - act_ref) / np.abs(act_ref)
    print("gnlp, actor column against float64: max relative error %.3g, %.3g (bound %.3g)" % (eg.max(), ea.max(), tol))
    assert ((gn_ref == 0) == (gn == 0)).all() and (gn_ref == 0).any() and (gn_ref != 0).any()
    # ---- assertions
    for k in former:
        np.testing.assert_array_equal(i32(new[k]), i32(former[k]), err_msg=k)
    for k, ref in exact.items():
        np.testing.assert_array_equal(i32(former[k]), i32(ref), err_msg=k)
    np.testing.assert_array_equal(i32(former["stat"][:, :, 1:]), i32(closs.transpose(0, 2, 1)))
    assert (eg <= tol).all() and (ea <= tol).all()
