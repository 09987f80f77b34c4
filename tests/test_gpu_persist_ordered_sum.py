"""-m gpu: the serial row sums that close the block reductions of the persistent update (csrc/sdxp_persist_sums.h: ordered_sum_ahead, used by
rows_reduce and by the opened-up reductions of backward L2, backward L1 and the dY0 shadow) request all their rows in front of the first add.
The order of the additions is the plain loop's - 0.0f + row 0 + row 1 + ... - so the bits must be too: the sums feed the Grams of the gradient
norm and the dY factors, hence every parameter.  The test entry sdxpk_ordered_sum_check (csrc/sdxp_persist_checks.hip, built with the epoch
kernel's flags) runs the helper at both sizes the kernel uses (16 and 32 rows, 64 columns) beside the plain loop on the same LDS rows.

Inputs: 13 random significant bits at exponents spread over 2^-12 .. 2^12 with mixed signs, so that almost every add rounds and the order shows;
one column of zeros with a -0.0 first row (the sum must be +0.0: 0.0f + -0.0f); one column whose rows cancel in pairs.  Asserted first on the host:
a pairwise tree over the same rows differs from the ascending sum in more than a third of the columns, i.e. another order could not pass."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROWS, COLS = 32, 64


def _rows():
    r = np.random.default_rng(5)
    m = r.integers(1 << 12, 1 << 13, size=(ROWS, COLS)).astype(np.float64)
    v = (m * 2.0 ** r.integers(-24, 1, size=(ROWS, COLS)) * r.choice([-1.0, 1.0], size=(ROWS, COLS))).astype(np.float32)
    v[:, 3] = 0.0
    v[0, 3] = -0.0
    v[1::2, 9] = -v[0::2, 9]
    return v


def _ascending(v, n):
    t = np.zeros(COLS, np.float32)
    for w in range(n):
        t = (t + v[w]).astype(np.float32)
    return t


def _tree(v, n):
    x = v[:n].copy()
    while x.shape[0] > 1:
        x = (x[0::2] + x[1::2]).astype(np.float32)
    return x[0]


def test_read_ahead_sum_has_the_bits_of_the_plain_loop():
    from seqdex_amd import _abi
    from seqdex_amd.sim import _stream_ptr
    lib, dev = _abi.load_library(), torch.device("cuda:0")
    lib.sdxpk_ordered_sum_check.restype = C.c_int
    lib.sdxpk_ordered_sum_check.argtypes = [C.c_void_p] * 4
    v = _rows()
    for n in (16, 32):
        differ = int((_ascending(v, n).view(np.int32) != _tree(v, n).view(np.int32)).sum())
        print("%d rows: a pairwise tree differs from the ascending sum in %d of %d columns" % (n, differ, COLS))
        assert differ > COLS // 3
    d = torch.from_numpy(v).to(dev)
    ref, got = (torch.full((2, COLS), float("nan"), device=dev) for _ in range(2))
    assert lib.sdxpk_ordered_sum_check(d.data_ptr(), ref.data_ptr(), got.data_ptr(), _stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    ref, got = ref.cpu().numpy(), got.cpu().numpy()
    for i, n in enumerate((16, 32)):
        want = _ascending(v, n)
        print("%d rows: plain loop against the host %d, read-ahead against the plain loop %d of %d columns differ in bits" % (
            n, int((ref[i].view(np.int32) != want.view(np.int32)).sum()), int((got[i].view(np.int32) != ref[i].view(np.int32)).sum()), COLS))
        np.testing.assert_array_equal(ref[i].view(np.int32), want.view(np.int32))
        np.testing.assert_array_equal(got[i].view(np.int32), ref[i].view(np.int32))
        assert got[i].view(np.int32)[3] == 0 and got[i][9] == 0.0
