"""Inputs and host restatements for the Grams of x2 and x1 of the persistent update (the block in the shadow of the epoch kernel's x3 edge,
csrc/sdxp_persist.hip; run verbatim by k_gram_x_check in csrc/sdxp_persist_checks.hip).
numpy only: shared by tests/test_persist_gram_x_order.py (CPU) and tests/test_gpu_persist_gram_x.py.

The order held, width K = 512 (x2) or 1024 (x1): thread t < 512 holds column t of the four samples, and column t + 512 at K = 1024.  Its term of
the lower-triangle entry (hi, lo) is 0.0f + x_hi[t] x_lo[t] rounded to float32 (so a -0.0 product becomes +0.0), and at K = 1024 the second
column is accumulated onto it by ONE fma: rn(x_hi[t + 512] x_lo[t + 512] + term).  The 512 terms are summed over each 16-lane DPP row by a
butterfly (partners lane ^ 1, ^ 2, ^ 4, ^ 8) and the 32 row sums are added from 0.0f in ascending order.

The inputs have 13 significant bits, exponents within 2^-6 .. 2^6: a product has at most 26 bits, the first column's ROUNDED product 24, and
their exponents lie at most 26 apart - the float64 sum x_hi x_lo + term is exact (test_persist_gram_x_order.py checks that against
rationals), so its single rounding to float32 IS the device's fma and the restatement can be compared bit for bit."""
import numpy as np

from helpers.input_gram_cases import MB, NTH, rows

U0, U1, BITS = 1024, 512, 13
TRI = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (3, 3)]      # gram_acc10's order of the lower triangle


def tri16(i):
    a, b = i >> 2, i & 3
    hi, lo = max(a, b), min(a, b)
    return hi * (hi + 1) // 2 + lo


def quantised(x):
    """float32 -> float32 with BITS significant bits (round to nearest)"""
    m, e = np.frexp(x.astype(np.float64))
    return np.ldexp(np.round(m * 2.0 ** BITS) / 2.0 ** BITS, e).astype(np.float32)


def inputs():
    """(x1 [3][MB][1024], x2 [3][MB][512]): minibatches 3, 4, 5 of input_gram_cases.rows stand for the three networks - the all-zero row is
    (network 0, sample 2), the column that is negative in all rows (network 2, column 7)"""
    x1 = quantised(rows(71, U0))[3 * MB:6 * MB].reshape(3, MB, U0)
    x2 = quantised(rows(72, U1))[3 * MB:6 * MB].reshape(3, MB, U1)
    return np.ascontiguousarray(x1), np.ascontiguousarray(x2)


def _first(x):
    """x [3][MB][K] -> the rounded products of the first column [3][10][512], as 0.0f + product"""
    hi = np.array([p[0] for p in TRI]); lo = np.array([p[1] for p in TRI])
    return (x[:, hi, :NTH] * x[:, lo, :NTH] + np.float32(0.0)).astype(np.float32)


def _second64(x):
    hi = np.array([p[0] for p in TRI]); lo = np.array([p[1] for p in TRI])
    return x[:, hi, NTH:].astype(np.float64) * x[:, lo, NTH:].astype(np.float64)             # exact: 26 bits


def terms(x):
    """x [3][MB][512 or 1024] -> [30][512] float32: what thread t holds in front of the butterfly, value net 10 + e"""
    q = _first(x)
    if x.shape[2] > NTH:
        q = (_second64(x) + q.astype(np.float64)).astype(np.float32)
    return q.reshape(30, NTH)


def terms_other_contraction(x1):
    """the diagonal's other fma: the FIRST column's square contracted, the second column's rounded"""
    hi = np.array([p[0] for p in TRI]); lo = np.array([p[1] for p in TRI])
    second = (x1[:, hi, NTH:] * x1[:, lo, NTH:] + np.float32(0.0)).astype(np.float32)
    first64 = x1[:, hi, :NTH].astype(np.float64) * x1[:, lo, :NTH].astype(np.float64)
    return (first64 + second.astype(np.float64)).astype(np.float32).reshape(30, NTH)


def terms_multiply_then_add(x1):
    hi = np.array([p[0] for p in TRI]); lo = np.array([p[1] for p in TRI])
    second = (x1[:, hi, NTH:] * x1[:, lo, NTH:]).astype(np.float32)
    return (_first(x1) + second).astype(np.float32).reshape(30, NTH)


DIAG = [net * 10 + e for net in range(3) for e in (0, 2, 5, 9)]


def entries(t):
    """terms [30][512] -> the finished 16-entry matrices [48] float32 (net 16 + i), in the kernel's order of adds"""
    q = t.reshape(30, NTH // 16, 16)
    l = np.arange(16)
    for m in (1, 2, 4, 8):
        q = (q + q[..., l ^ m]).astype(np.float32)
    s = np.zeros(30, np.float32)
    for w in range(NTH // 16):
        s = (s + q[:, w, 0]).astype(np.float32)
    return np.array([s[(i >> 4) * 10 + tri16(i & 15)] for i in range(48)], np.float32)


def entries_ascending(t):
    s = np.zeros(30, np.float32)
    for k in range(NTH):
        s = (s + t[:, k]).astype(np.float32)
    return np.array([s[(i >> 4) * 10 + tri16(i & 15)] for i in range(48)], np.float32)
