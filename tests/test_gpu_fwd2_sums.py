"""-m gpu: fwd2_sums (csrc/sdxp_persist_sums.h) - the twelve wave sums of forward L2's bare products w2 * x2 as ONE butterfly behind an explicit
fma level - against the twelve trees it replaces, bit for bit, through the test entry sdxpk_fwd2_sums_check of the loaded library: one
workgroup of 512 threads (8 waves), w [3][512], x [3][4][512], value net * 4 + s.

What the trees were: wave_sum(w * x) compiles to v_mul / v_mov_dpp quad_perm:[1,0,3,2] / v_fmac, i.e. lane l starts from
fma(w_l, x_l, rounded product of lane l ^ 1), and five dpp_add levels carry the view of lanes 15, 13, 8, 10, 0, 2, 7, 5 of every 16-lane row to
lane 63.  The device reference restates that tree serially (explicit fma, then the dpp_add levels, lane 63); the host restates it once more in
exact rational arithmetic, every operation rounded ONCE to float32 (no float64 intermediate that could round twice), and pins the reference.
The inputs are the families of test_gpu_wave_sums.py, applied to w and to x.  They can tell the fma first level from multiply-then-add: the host
runs the tree both ways and requires that the results differ in bits somewhere - a butterfly that summed rounded products (the build
that was dropped for x3's last bit) could then not pass by accident.

After fwd2_sums the 32 lanes of a wave with (lane & 15) in {0, 2, 5, 7, 8, 10, 13, 15} hold the three networks' sums of ONE sample each
(0, 1, 2, 3 for lanes 0, 2, 5, 7 and for their mirrors 15, 13, 10, 8); the kernel stores from lanes 0, 2, 5, 7 of a wave.  The test entry writes
all 32 and leaves the other slots alone."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_wave_sums import NTH, WAVES, _bits, _inputs  # noqa: E402

NETS, MB = 3, 4
SAMPLE_OF_LANE = {0: 0, 15: 0, 2: 1, 13: 1, 5: 2, 10: 2, 7: 3, 8: 3}     # (lane & 15) -> the sample whose sums the lane holds


# ---- float32 arithmetic through exact rationals, one rounding per operation, signed zeros as IEEE 754 has them (round to nearest even)
def _round32(fr):
    """the float32 nearest to the non-zero Fraction fr, ties to even"""
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if a < Fraction(2) ** e:
        e -= 1                                   # 2^e <= a < 2^(e + 1)
    e = max(e, -126)                             # subnormals share the smallest normal exponent's spacing
    q = a / Fraction(2) ** (e - 23)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
        n += 1
    out = np.float32(float(n * Fraction(2) ** (e - 23)))     # n <= 2^24 and the scale is a power of two: exact in float64 and in float32
    assert np.isfinite(out)
    return -out if fr < 0 else out


def _fr(v):
    return Fraction(float(v))


def _mul(a, b):
    p = _fr(a) * _fr(b)
    if p == 0:
        return np.float32(-0.0) if (np.signbit(a) != np.signbit(b)) else np.float32(0.0)
    return _round32(p)


def _add(a, b):
    t = _fr(a) + _fr(b)
    if t == 0:
        return np.float32(-0.0) if (a == 0 and b == 0 and np.signbit(a) and np.signbit(b)) else np.float32(0.0)
    return _round32(t)


def _fma(a, b, c):
    p = _fr(a) * _fr(b)
    t = p + _fr(c)
    if t == 0:
        neg = p == 0 and c == 0 and (np.signbit(a) != np.signbit(b)) and np.signbit(c)
        return np.float32(-0.0) if neg else np.float32(0.0)
    return _round32(t)


def _tree(w, x):
    """the wave's result of the tree for one value: w, x are the 64 lanes' float32 operands"""
    p = [_mul(w[l], x[l]) for l in range(64)]
    v = [_fma(w[l], x[l], p[l ^ 1]) for l in range(64)]                      # v_fmac onto v_mov_dpp quad_perm:[1,0,3,2] of the rounded product
    for m in (2, 7, 15):                                                     # quad_perm:[2,3,0,1], row_half_mirror, row_mirror
        v = [_add(v[l], v[l ^ m]) for l in range(64)]
    v = [_add(v[l], v[(l & ~15) - 1]) if (l >> 4) & 1 else v[l] for l in range(64)]      # row_bcast15 into rows 1 and 3
    v = [_add(v[l], v[31]) if l >= 32 else v[l] for l in range(64)]                      # row_bcast31 into rows 2 and 3
    return v[63]


def _host(w, x):
    """w [3][512], x [12][512] -> [12][8]: the tree with the fma first level, exact rationals rounded once per operation"""
    out = np.zeros((NETS * MB, WAVES), np.float32)
    for i in range(NETS * MB):
        for wv in range(WAVES):
            sl = slice(64 * wv, 64 * wv + 64)
            out[i, wv] = _tree(w[i // MB][sl], x[i][sl])
    return out


def _host_mul_add(w, x):
    """the same tree over the ROUNDED products (multiply, then add: what a butterfly of wave_sums would form); numpy's float32 operations
    round once each"""
    l = np.arange(64)
    v = (np.repeat(w, MB, axis=0) * x).astype(np.float32).reshape(NETS * MB, WAVES, 64)
    for m in (1, 2, 7, 15):
        v = (v + v[..., l ^ m]).astype(np.float32)
    v = np.where((l >> 4) & 1, v + v[..., (l & ~15) - 1], v).astype(np.float32)
    v = np.where(l >= 32, v + v[..., 31:32], v).astype(np.float32)
    return v[..., 63]


def _check(w, x):
    from seqdex_amd import _abi
    from seqdex_amd.sim import _stream_ptr
    lib = _abi.load_library()
    lib.sdxpk_fwd2_sums_check.restype = C.c_int
    lib.sdxpk_fwd2_sums_check.argtypes = [C.c_void_p] * 5
    dev = torch.device("cuda:0")
    d_w, d_x = torch.from_numpy(w).to(dev), torch.from_numpy(x).to(dev)
    ref = torch.full((NETS * MB, NTH), float("nan"), device=dev)
    got = torch.full((NETS * MB, NTH), float("nan"), device=dev)
    assert lib.sdxpk_fwd2_sums_check(d_w.data_ptr(), d_x.data_ptr(), ref.data_ptr(), got.data_ptr(), _stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    return ref.cpu().numpy(), got.cpu().numpy()


def host_cases():
    """name -> (w [3][512], x [12][512], the tree with the fma first level [12][8], the tree with multiply-then-add [12][8])"""
    ws, xs = _inputs(NETS), _inputs(NETS * MB)
    return {k: (ws[k], xs[k], _host(ws[k], xs[k]), _host_mul_add(ws[k], xs[k])) for k in ws}


def test_fwd2_sums_equal_the_contracted_trees_bit_for_bit():
    cases = host_cases()
    # the inputs can tell the contracted first level from a sum of rounded products (a test that cannot fail is not a test)
    differ = {k: int((_bits(c[2]) != _bits(c[3])).sum()) for k, c in cases.items()}
    print("(wave, value) sums of %d that differ in bits between fma-first-level and multiply-then-add: %r" % (NETS * MB * WAVES, differ))
    assert differ["scaled"] > 0
    lanes = np.arange(NTH)
    for name, (w, x, want, _) in cases.items():
        ref, got = _check(w, x)
        # the serial device tree is the tree the host restates (this pins what `ref` means) ...
        assert (_bits(ref).reshape(-1, WAVES, 64) == _bits(ref).reshape(-1, WAVES, 64)[:, :, :1]).all(), name     # lane 63's value, on every lane
        np.testing.assert_array_equal(_bits(ref[:, ::64]), _bits(want), err_msg="%s: the serial tree against the host's exact arithmetic" % name)
        # ... and the butterfly leaves the same bits in the lanes that hold the value
        for i in range(NETS * MB):
            own = np.array([SAMPLE_OF_LANE.get(int(l) & 15) == i % MB for l in lanes])
            r, g_ = _bits(ref[i]), _bits(got[i])
            bad = np.nonzero(r[own] != g_[own])[0]
            assert bad.size == 0, "%s value %d: %d lanes differ, first lane %d: trees %r fwd2_sums %r" % (
                name, i, bad.size, lanes[own][bad[0]], ref[i][own][bad[0]], got[i][own][bad[0]])
            assert np.isnan(got[i][~own]).all(), (name, i)      # the other lanes' slots were not written
    assert (cases["zeros"][2] == 0.0).all()
