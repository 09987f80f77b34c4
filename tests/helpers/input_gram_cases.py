"""Inputs and host restatements for the Grams of the persistent update's layer-0 inputs (csrc/sdxp_persist.hip: k_input_grams, and the form the
epoch kernel gave them in its x1 shadow, kept as k_input_grams_reference in csrc/sdxp_persist_checks.hip).  numpy only: shared by the CPU test of
the restatement (tests/test_persist_input_grams_order.py) and the GPU tests (tests/test_gpu_persist_input_grams.py).

The order held: thread tid < 512 of the workgroup holds column tid of the four rows (and column tid + 512 where that is below the width: the 564
wide central-value rows); its term of entry (s, t) is the rounded product x_s[tid] x_t[tid], with the second column accumulated by one fma; the
512 terms are summed over each 16-lane DPP row by a butterfly (partners lane ^ 1, ^ 2, ^ 4, ^ 8) and the 32 row sums are added from 0.0f in
ascending order."""
import numpy as np

MB, NTH, OBS, ST, N_MB = 4, 512, 396, 564, 8
PAIRS = [(i >> 2, i & 3) for i in range(16)]          # entry i of the 16-entry form is (row i >> 2, row i & 3) of the symmetric 4 x 4 Gram
ZERO_ROW = (3, 2)                                      # (minibatch, sample): an all-zero row
NEG_COL = (5, 7)                                       # (minibatch, column): negative in all four rows


def rows(seed, width):
    """[4 N_MB][width] float32 with a wide dynamic range (sign * 2^e * m, e uniform in [-6, 6], m in [1, 2)): the rounding of a sum of their
    products depends on the order of the adds.  One minibatch has an all-zero row, one a column that is negative in all its rows."""
    g = np.random.default_rng(seed)
    n = MB * N_MB
    x = (g.choice([-1.0, 1.0], (n, width)) * np.exp2(g.uniform(-6.0, 6.0, (n, width))) * g.uniform(1.0, 2.0, (n, width))).astype(np.float32)
    x[MB * ZERO_ROW[0] + ZERO_ROW[1]] = 0.0
    c = slice(MB * NEG_COL[0], MB * NEG_COL[0] + MB)
    x[c, NEG_COL[1]] = -np.abs(x[c, NEG_COL[1]])
    return x


def _pairs(x):
    """x [4 n_mb][K] -> (a, b) [n_mb][16][K]: the two rows of every entry, hi row first (gram_acc10 forms x_hi * x_lo)"""
    m = x.reshape(-1, MB, x.shape[1])
    hi = np.array([max(p) for p in PAIRS]); lo = np.array([min(p) for p in PAIRS])
    return m[:, hi], m[:, lo]


def gram_kernel_order(x):
    """x [4 n_mb][K <= 564] float32 -> [n_mb][16] float32 in the order of the kernels (module docstring).  The fma of the second column is
    formed in float64 (the product of two float32 is exact there) and rounded once more to float32: a double rounding can differ from the
    device's fma in a last bit on rare inputs, so this restatement serves the counts, not a bit comparison."""
    a, b = _pairs(x)
    K = x.shape[1]
    q = np.zeros(a.shape[:2] + (NTH,), np.float32)
    n1 = min(K, NTH)
    q[..., :n1] = a[..., :n1] * b[..., :n1]                                   # float32 product, rounded once
    if K > NTH:
        q[..., :K - NTH] = (a[..., NTH:].astype(np.float64) * b[..., NTH:].astype(np.float64) + q[..., :K - NTH].astype(np.float64)).astype(np.float32)
    q = q.reshape(q.shape[:2] + (NTH // 16, 16))
    l = np.arange(16)
    for m in (1, 2, 4, 8):
        q = (q + q[..., l ^ m]).astype(np.float32)
    t = np.zeros(q.shape[:2], np.float32)
    for w in range(NTH // 16):
        t = (t + q[..., w, 0]).astype(np.float32)
    return t


def gram_ascending(x):
    """the same entries as a plain float32 sum over ascending k of the rounded products"""
    a, b = _pairs(x)
    p = (a * b).astype(np.float32)
    t = np.zeros(p.shape[:2], np.float32)
    for k in range(x.shape[1]):
        t = (t + p[..., k]).astype(np.float32)
    return t


def gram_float64(x):
    """(the entries in float64, sum_k |a_k b_k| of every entry)"""
    a, b = _pairs(x)
    p = a.astype(np.float64) * b.astype(np.float64)
    return p.sum(-1), np.abs(p).sum(-1)


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.int32)
