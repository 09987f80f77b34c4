"""-m gpu: the backward through the heads of the persistent update kernel (phase D; csrc/sdxp_persist_phase_d.h: head_backward).  Lane (column k, row
half c) forms sum_j dmu[s][13 c + j] w[13 c + j][k] as one fma chain per sample - the upper half's rows 23, 24 are the two value heads, whose products
dv[j][s] w[23 + j][k] are its a1 / a2, and dmu[.][23..25] are zeros - the halves of a column meet through v_permlane32_swap, and elu'(x3) of the three
networks is applied.  head_backward requests its LDS operands ahead of the chains - the eight S.dv values in ONE block in front of the first chain where
the former code had eight branches with a read and a drained wait each - and keeps chains, pair sums and products, so the bits must be the former's.

The test entry sdxpk_head_backward_check (csrc/sdxp_persist_checks.hip, built with the epoch kernel's flags) runs head_backward beside the former block,
kept there verbatim: one workgroup of 512 threads per case, d2[3][4] per lane out.

(a) new == former, bit for bit, all 512 x 12 values of every case (both row halves c are lanes of every wave);
(b) asserted on the host first: the 13 terms of a chain summed in column order and as a pairwise tree differ in most outputs, so the order of the
    kernel's chain - and with it a wrong operand, row or sample - shows in the bits of (a);
(c) the former block is within 16 * 2^-24 * sum |terms| * |elu'| of float64: the standard bound for the 13 fmas of a chain, the add of the two halves
    and the product with elu' (the value heads: one product, one add, one product).  The measured ratio is printed.
(d) S.x3 holds entries > 0, < 0, +0.0 and -0.0 in every case (asserted): elu' is 1 above zero and x + 1 at and below it, and the select that drops the
    lower half's a1 / a2 must give +0.0 as the branch did.

Inputs as in test_gpu_persist_head_forward.py: 13 random significant bits, mixed signs; the chain's factors (dmu, the head matrix) at exponents spread
over seven binades each - a chain has 13 terms, not 256: over 25 binades the largest term decides most sums whatever the order and (b) fails (43 %) -
dv and x3 over 25."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MB, U2, A, NTH, CASES = 4, 256, 23, 512, 4
ROWS = A + 2


def _values(r, shape, lo=-24):
    m = r.integers(1 << 12, 1 << 13, size=shape).astype(np.float64)
    return (m * 2.0 ** r.integers(lo, 1, size=shape) * r.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def _inputs():
    r = np.random.default_rng(31)
    dmu = np.zeros((CASES, MB, 32), np.float32)
    dmu[:, :, :A] = _values(r, (CASES, MB, A), -6)
    dv = _values(r, (CASES, 2, MB))
    x3 = _values(r, (CASES, 3, MB, U2))
    # signed zeros in every network and sample of every case
    x3[:, :, :, 5::64] = 0.0
    x3[:, :, :, 37::64] = -0.0
    hw = _values(r, (CASES, ROWS, U2), -6)
    return dmu, dv, x3, hw


def test_operands_requested_ahead_keep_the_bits():
    from seqdex_amd import _abi
    from seqdex_amd.sim import _stream_ptr
    lib, dev = _abi.load_library(), torch.device("cuda:0")
    lib.sdxpk_head_backward_check.restype = C.c_int
    lib.sdxpk_head_backward_check.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    dmu, dv, x3, hw = _inputs()
    # (d)
    for c in range(CASES):
        assert (x3[c] > 0).any() and (x3[c] < 0).any()
        z = x3[c] == 0
        assert (z & ~np.signbit(x3[c])).any() and (z & np.signbit(x3[c])).any()
    # exact terms per (case, sample, half, column): 13 products of the policy rows; the value heads' products on the upper half
    d64, w64 = dmu.astype(np.float64), hw.astype(np.float64)
    rows = np.minimum(13 * np.arange(2)[:, None] + np.arange(13)[None, :], A + 1)            # [half][j]
    terms = d64[:, :, :26].reshape(CASES, MB, 2, 13)[..., None] * w64[:, rows][:, None]       # [case][s][half][j][k]; dmu[.][23..25] are zeros
    # (b)
    t32 = terms.astype(np.float32)
    seq = np.zeros(t32.shape[:3] + (U2,), np.float32)
    for j in range(13):
        seq = (seq + t32[:, :, :, j]).astype(np.float32)
    tree = np.concatenate([t32, np.zeros_like(t32[:, :, :, :3])], axis=3)
    while tree.shape[3] > 1:
        tree = (tree[:, :, :, 0::2] + tree[:, :, :, 1::2]).astype(np.float32)
    differ = int((seq.view(np.int32) != tree[:, :, :, 0].view(np.int32)).sum())
    print("column-order and tree-order sums of the same 13 terms differ in %d of %d chains" % (differ, seq.size))
    assert 2 * differ > seq.size
    d = [torch.from_numpy(v).to(dev) for v in (dmu, dv, x3, hw)]
    out = torch.full((CASES, 2, 3 * MB, NTH), float("nan"), device=dev)
    assert lib.sdxpk_head_backward_check(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), CASES, out.data_ptr(), _stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    former, new = out[:, 0], out[:, 1]
    assert not np.isnan(former).any() and not np.isnan(new).any()
    # (c) float64 reference of d2[net][s] at thread t: column k = 32 (t >> 6) + (t & 31), both halves hold the column's value
    t = np.arange(NTH)
    k = 32 * (t >> 6) + (t & 31)
    x64 = x3.astype(np.float64)
    eg = np.where(x64 > 0, 1.0, x64 + 1.0)                                                    # [case][net][s][k]
    a = np.zeros((CASES, 3, MB, U2)); mag = np.zeros((CASES, 3, MB, U2))
    a[:, 0] = terms.sum((2, 3)); mag[:, 0] = np.abs(terms).sum((2, 3))
    for j in range(2):
        p = dv.astype(np.float64)[:, j, :, None] * w64[:, A + j][:, None, :]
        a[:, 1 + j] = p; mag[:, 1 + j] = np.abs(p)
    exact, bound = (a * eg)[..., k], (16 * 2.0 ** -24 * mag * np.abs(eg))[..., k]
    err = np.abs(former.reshape(CASES, 3, MB, NTH).astype(np.float64) - exact)
    print("former block against float64: max |error| / (16 2^-24 sum |terms| |elu'|) = %.4f" % float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    # (a)
    print("head_backward against the former block: %d of %d outputs differ in bits" % (int((new.view(np.int32) != former.view(np.int32)).sum()), new.size))
    np.testing.assert_array_equal(new.view(np.int32), former.view(np.int32))
