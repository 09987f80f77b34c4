"""-m gpu: the head forward of the persistent update kernel (phase D; csrc/sdxp_persist_tails.h: head_forward).  Wave w forms head rows w, w + 8,
w + 16 (actor rows; row 23, the critic's value, on wave 7) and w + 24 (row 24, the central value, on wave 0 only): per (row, sample) each lane
runs one fma chain over its four columns, the 64 lanes meet in wave_sums, lane s adds the row's bias.  head_forward requests the value rows'
sixteen x3 operands and the rows' biases together with the actor rows' operands, in front of the first fma, where the former code read the value
rows' operands inside their chains and the biases behind the sums; chains, sums and stores are unchanged, so the bits must be too.

The test entry sdxpk_head_forward_check (csrc/sdxp_persist_checks.hip, built with the epoch kernel's flags) runs head_forward beside the former
block, kept there verbatim: one workgroup of 512 threads per case, x3 [3][4][256], the 25 x 256 head matrix and its 25 biases in, mu [4][23] and
val [2][4] out.

(a) new == former, bit for bit, every output written;
(b) asserted on the host first: the sum of the same 256 float32 terms in column order and as a pairwise tree differ in most outputs, so the
    order of the kernel's sums - and with it a wrong operand, row or sample - shows in the bits of (a);
(c) the former block is within 257 * 2^-24 * (sum |w x| + |b|) of float64: the standard bound for a float32 sum of 257 terms in any order (the fmas
    round less often than product-then-add).  The measured ratio is printed.

Inputs as in test_gpu_persist_ordered_sum.py: 13 random significant bits at exponents spread over 2^-12 .. 2^12, mixed signs (a product of two
13-bit values has 26 bits: exact in float64, the terms of (c); (b) adds the products rounded to float32)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MB, U2, A, CASES = 4, 256, 23, 6
ROWS = A + 2
NET_OF_ROW = np.array([0] * A + [1, 2])
_REF = {}


def _values(r, shape):
    m = r.integers(1 << 12, 1 << 13, size=shape).astype(np.float64)
    return (m * 2.0 ** r.integers(-24, 1, size=shape) * r.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def _inputs():
    r = np.random.default_rng(23)
    return _values(r, (CASES, 3, MB, U2)), _values(r, (CASES, ROWS, U2)), _values(r, (CASES, ROWS))


def _reference():
    """terms [CASES][ROWS][MB][U2] (float64, exact), exact [CASES][ROWS][MB], bound [CASES][ROWS][MB]: computed once"""
    if not _REF:
        x3, hw, hb = _inputs()
        terms = hw.astype(np.float64)[:, :, None, :] * x3.astype(np.float64)[:, NET_OF_ROW]          # [case][row][s][k]
        _REF["terms"] = terms
        _REF["exact"] = terms.sum(-1) + hb.astype(np.float64)[:, :, None]
        _REF["bound"] = 257 * 2.0 ** -24 * (np.abs(terms).sum(-1) + np.abs(hb.astype(np.float64))[:, :, None])
    return _REF


def _split(o):
    """out [CASES][MB A + 2 MB] -> [CASES][ROWS][MB]"""
    mu = o[:, :MB * A].reshape(CASES, MB, A).transpose(0, 2, 1)
    val = o[:, MB * A:].reshape(CASES, 2, MB)
    return np.concatenate([mu, val], axis=1)


def test_operands_requested_together_keep_the_bits():
    from seqdex_amd import _abi
    from seqdex_amd.sim import _stream_ptr
    lib, dev = _abi.load_library(), torch.device("cuda:0")
    lib.sdxpk_head_forward_check.restype = C.c_int
    lib.sdxpk_head_forward_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    x3, hw, hb = _inputs()
    ref = _reference()
    # (b) the order of the adds shows in the bits
    t32 = ref["terms"].astype(np.float32)
    seq = np.zeros(t32.shape[:-1], np.float32)
    for k in range(U2):
        seq = (seq + t32[..., k]).astype(np.float32)
    tree = t32.copy()
    while tree.shape[-1] > 1:
        tree = (tree[..., 0::2] + tree[..., 1::2]).astype(np.float32)
    differ = int((seq.view(np.int32) != tree[..., 0].view(np.int32)).sum())
    print("column-order and tree-order sums of the same 256 terms differ in %d of %d outputs" % (differ, seq.size))
    assert 2 * differ > seq.size
    d = [torch.from_numpy(v).to(dev) for v in (x3, hw, hb)]
    out = torch.full((CASES, 2, MB * A + 2 * MB), float("nan"), device=dev)
    assert lib.sdxpk_head_forward_check(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), CASES, out.data_ptr(), _stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    former, new = out[:, 0], out[:, 1]
    assert not np.isnan(former).any() and not np.isnan(new).any()
    # (c)
    err = np.abs(_split(former).astype(np.float64) - ref["exact"])
    print("former block against float64: max |error| / (257 2^-24 (sum |w x| + |b|)) = %.4f" % float((err / ref["bound"]).max()))
    assert (err <= ref["bound"]).all()
    # (a)
    print("head_forward against the former block: %d of %d outputs differ in bits" % (int((new.view(np.int32) != former.view(np.int32)).sum()), new.size))
    np.testing.assert_array_equal(new.view(np.int32), former.view(np.int32))
