"""-m gpu: row_butterfly<N> (csrc/sdxp_persist_sums.h) - the sums of N values over every 16-lane DPP row as one halving butterfly, each
level written as two fused pair sums and one select - against ONE plain tree per value (partners lane ^ 1, ^ 2, ^ 4, ^ 8, fetched with
__shfl_xor, no DPP), bit for bit, through the test entry sdxpk_row_butterfly_check of the loaded library: one workgroup of 512 threads (32
rows), N = 12 (backward L2), 30 (the Gram reductions) and 48 (backward L1).  Every block reduction of the persistent update, the forward
passes' wave_sums and k_input_grams run on this helper, so its pairs are the bits of every parameter.

The inputs have a wide dynamic range, so that the ORDER of a sum shows in its bits: the host sums every row in plain lane order and in the
tree's order and requires that most (row, value) sums differ - a butterfly that paired other lanes could not pass by accident.  The host's
tree is also compared with the device's reference, which pins what `ref` means.  Rows of zeros of both signs check that a padded or
deselected slot never turns a -0 sum into +0."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NTH, ROWS = 512, 32


def _inputs(n):
    rng = np.random.default_rng(40 + n)
    scaled = (rng.standard_normal((n, NTH)) * np.exp2(rng.integers(-20, 21, (n, NTH)))).astype(np.float32)     # mixed signs, 2^-20 .. 2^20
    zeros = np.where(rng.random((n, NTH)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    zeros[:, :16] = -0.0                                                # one row of negative zeros only: every sum of it is -0
    return {"scaled": scaled, "zeros": zeros}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _tree_order(x):
    """x [n][512] -> [n][32]: partners lane ^ 1, ^ 2, ^ 4, ^ 8 within each 16-lane row"""
    v = x.reshape(x.shape[0], ROWS, 16).astype(np.float32)
    for _ in range(4):
        v = (v[..., 0::2] + v[..., 1::2]).astype(np.float32)
    return v[..., 0]


def _lane_order(x):
    v = x.reshape(x.shape[0], ROWS, 16).astype(np.float32)
    t = np.zeros(v.shape[:2], np.float32)
    for l in range(16):
        t = (t + v[..., l]).astype(np.float32)
    return t


def _check(n, x):
    from seqdex_amd import _abi
    from seqdex_amd.sim import _stream_ptr
    lib = _abi.load_library()
    lib.sdxpk_row_butterfly_check.restype = C.c_int
    lib.sdxpk_row_butterfly_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(x).to(dev)
    ref = torch.full((n, NTH), float("nan"), device=dev)
    got = torch.full((n, NTH), float("nan"), device=dev)
    assert lib.sdxpk_row_butterfly_check(d_in.data_ptr(), ref.data_ptr(), got.data_ptr(), n, _stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    return ref.cpu().numpy(), got.cpu().numpy()


@pytest.mark.parametrize("n", [12, 30, 48])
def test_row_butterfly_equals_one_tree_per_value_bit_for_bit(n):
    sets = _inputs(n)
    differ = int((_bits(_tree_order(sets["scaled"])) != _bits(_lane_order(sets["scaled"]))).sum())
    print("N = %d: %d of %d (row, value) sums differ in bits between lane order and tree order" % (n, differ, n * ROWS))
    assert differ > n * ROWS // 2
    lanes = np.arange(NTH)
    for name, x in sets.items():
        ref, got = _check(n, x)
        r = _bits(ref).reshape(n, ROWS, 16)
        assert (r == r[:, :, :1]).all(), name                                            # the plain tree leaves one value in every lane of a row
        np.testing.assert_array_equal(r[:, :, 0], _bits(_tree_order(x)), err_msg="%s: the device's plain tree against the host's" % name)
        bad = 0
        for i in range(n):
            own = (lanes & 3) == (i & 3)                                                 # the lanes that hold value i after row_butterfly
            d = np.nonzero(_bits(ref[i])[own] != _bits(got[i])[own])[0]
            bad += d.size
            assert d.size == 0, "%s N=%d value %d: %d lanes differ, first lane %d: tree %r butterfly %r" % (
                name, n, i, d.size, lanes[own][d[0]], ref[i][own][d[0]], got[i][own][d[0]])
            assert np.isnan(got[i][~own]).all(), (name, i)                               # the other lanes' slots were not written
        print("N = %d %s: %d lanes differ in bits from the plain trees" % (n, name, bad))
    zr, _ = _check(n, sets["zeros"])
    assert np.signbit(zr[:, :16]).all() and (zr[:, :16] == 0.0).all()                    # the row of negative zeros sums to -0
