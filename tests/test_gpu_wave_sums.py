"""-m gpu: wave_sums<N> (csrc/sdxp_persist_sums.h) - N wave sums as one halving butterfly plus two permlane swaps - against N independent
wave_sum trees (csrc/sdxp_device.h), bit for bit, through the test entry sdxpk_wave_sums_check of the loaded library: one workgroup of 512
threads (8 waves), N = 12 (the forward phases) and N = 16 (the head forward on wave 0).  The inputs are chosen so that the ORDER of a sum
shows in its bits: the host sums every wave in plain lane order and in the tree's order and requires that the two differ somewhere - a
butterfly that paired other lanes than wave_sum does could then not pass by accident."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NTH, WAVES = 512, 8
SEED = 5


def _inputs(n):
    """name -> float32 [n][512]"""
    rng = np.random.default_rng(SEED + n)
    scaled = (rng.standard_normal((n, NTH)) * np.exp2(rng.integers(-20, 21, (n, NTH)))).astype(np.float32)     # mixed signs, 2^-20 .. 2^20
    big = np.ones((n, NTH), np.float32)
    for w in range(WAVES):
        for i in range(n):
            big[i, 64 * w + (7 * w + 5 * i + 3) % 64] = 1e8            # one lane per wave and value, another lane in every wave
    zeros = np.where(rng.random((n, NTH)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    zeros[0, :64] = -0.0                                                # one wave of negative zeros only: its sum is -0
    return {"scaled": scaled, "big": big, "zeros": zeros}


def _tree_order(x):
    """float32 sum of each wave's 64 lanes in wave_sum's order: partners lane ^ 1, ^ 2, ^ 4, ^ 8, ^ 16, ^ 32.  x: [n][512] -> [n][8]"""
    v = x.reshape(x.shape[0], WAVES, 64).astype(np.float32)
    for _ in range(6):
        v = (v[..., 0::2] + v[..., 1::2]).astype(np.float32)
    return v[..., 0]


def _lane_order(x):
    v = x.reshape(x.shape[0], WAVES, 64).astype(np.float32)
    t = np.zeros(v.shape[:2], np.float32)
    for l in range(64):
        t = (t + v[..., l]).astype(np.float32)
    return t


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check(n, x):
    from seqdex_amd import _abi
    from seqdex_amd.sim import _stream_ptr
    lib = _abi.load_library()
    lib.sdxpk_wave_sums_check.restype = C.c_int
    lib.sdxpk_wave_sums_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(x).to(dev)
    ref = torch.full((n, NTH), float("nan"), device=dev)
    got = torch.full((n, NTH), float("nan"), device=dev)
    assert lib.sdxpk_wave_sums_check(d_in.data_ptr(), ref.data_ptr(), got.data_ptr(), n, _stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    return ref.cpu().numpy(), got.cpu().numpy()


@pytest.mark.parametrize("n", [12, 16])
def test_wave_sums_equal_wave_sum_bit_for_bit(n):
    sets = _inputs(n)
    # the inputs can tell two orders of summation apart (a test that cannot fail is not a test)
    differ = sum(int((_bits(_tree_order(sets[k])) != _bits(_lane_order(sets[k]))).sum()) for k in ("scaled", "big"))
    print("N = %d: %d of %d (wave, value) sums differ in bits between lane order and tree order" % (n, differ, 2 * n * WAVES))
    assert differ > 0
    lanes = np.arange(NTH)
    for name, x in sets.items():
        ref, got = _check(n, x)
        # wave_sum is the tree the host restates (this also pins what `ref` means)
        np.testing.assert_array_equal(_bits(ref[:, ::64]), _bits(_tree_order(x)), err_msg="%s: wave_sum against the host's tree" % name)
        for i in range(n):
            own = (lanes & 3) == (i & 3)                        # the lanes that hold value i after wave_sums
            r, g_ = _bits(ref[i]), _bits(got[i])
            assert (r.reshape(WAVES, 64) == r.reshape(WAVES, 64)[:, :1]).all(), (name, i)      # wave_sum: every lane of a wave, one value
            bad = np.nonzero(r[own] != g_[own])[0]
            assert bad.size == 0, "%s N=%d value %d: %d lanes differ, first lane %d: wave_sum %r wave_sums %r" % (
                name, n, i, bad.size, lanes[own][bad[0]], ref[i][own][bad[0]], got[i][own][bad[0]])
            assert np.isnan(got[i][~own]).all(), (name, i)      # the other lanes' slots were not written
    zr, _ = _check(n, sets["zeros"])
    assert np.signbit(zr[0, 0]) and zr[0, 0] == 0.0             # the wave of negative zeros sums to -0
