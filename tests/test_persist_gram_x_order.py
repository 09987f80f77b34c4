"""The host restatement of the persistent update's Grams of x1 / x2 (helpers/gram_x_cases.py) and the properties of its inputs that let
tests/test_gpu_persist_gram_x.py compare the device's terms with it BIT FOR BIT, checked without a GPU:

(a) the float64 sum b b + rn(a a) that restates the device's fma is exact - 400 terms against rationals - so its one rounding to float32 is
    the fma's;
(b) the inputs discriminate: the per-thread diagonal terms of the Gram of x1 differ in at least 10 % of the cases under the OTHER contraction
    (the first column's square taken into the fma, the second's rounded), and under multiply-then-add (printed); the FINISHED entries differ
    in only a few of 32 - which is why the GPU test compares the terms;
(c) the order of the adds shows: the kernel's tree and a plain ascending sum of the same terms differ in most finished entries."""
from fractions import Fraction

import numpy as np

from helpers.gram_x_cases import DIAG, NTH, TRI, U0, U1, BITS, entries, entries_ascending, inputs, terms, terms_multiply_then_add, terms_other_contraction
from helpers.input_gram_cases import bits


def test_inputs_have_13_bits_and_the_special_rows():
    x1, x2 = inputs()
    assert x1.shape == (3, 4, U0) and x2.shape == (3, 4, U1)
    for x in (x1, x2):
        m, _ = np.frexp(x.astype(np.float64))
        assert (m * 2.0 ** BITS == np.round(m * 2.0 ** BITS)).all()
        assert (x[0, 2] == 0).all() and (x[2, :, 7] < 0).all()
        assert np.abs(x[x != 0]).min() >= 2.0 ** -6 and np.abs(x).max() < 2.0 ** 7


def test_float64_restatement_of_the_fma_is_exact():
    x1, _ = inputs()
    t = terms(x1)
    g = np.random.default_rng(5)
    exact = 0
    for _ in range(400):
        net, e, k = int(g.integers(3)), int(g.integers(10)), int(g.integers(NTH))
        hi, lo = TRI[e]
        first = np.float32(x1[net, hi, k] * x1[net, lo, k] + np.float32(0.0))
        want = Fraction(float(x1[net, hi, k + NTH])) * Fraction(float(x1[net, lo, k + NTH])) + Fraction(float(first))
        got64 = float(x1[net, hi, k + NTH]) * float(x1[net, lo, k + NTH]) + float(first)
        exact += Fraction(got64) == want
        assert bits(np.float32(got64)) == bits(t[net * 10 + e, k])
    print("%d of 400 float64 sums b b + rn(a a) are exact" % exact)
    assert exact == 400


def test_inputs_tell_the_contractions_apart():
    x1, _ = inputs()
    t, other, mta = terms(x1), terms_other_contraction(x1), terms_multiply_then_add(x1)
    d_other = float((bits(t[DIAG]) != bits(other[DIAG])).mean())
    d_mta = float((bits(t[DIAG]) != bits(mta[DIAG])).mean())
    e, e_other = entries(t), entries(other)
    diag_e = [net * 16 + 5 * s for net in range(3) for s in range(4)]
    print("diagonal terms of G_x1: %.1f %% differ under the other contraction, %.1f %% under multiply-then-add; finished entries: %d of 48 (%d of 12 diagonal)" % (
        100 * d_other, 100 * d_mta, int((bits(e) != bits(e_other)).sum()), int((bits(e[diag_e]) != bits(e_other[diag_e])).sum())))
    assert d_other >= 0.10


def test_order_of_the_adds_shows_in_the_finished_entries():
    for x in inputs():
        t = terms(x)
        e, asc = entries(t), entries_ascending(t)
        live = [i for i in range(48) if not (i >> 4 == 0 and 2 in ((i & 15) >> 2, i & 3))]      # (the zero row's entries are +0.0 either way)
        differ = int((bits(e[live]) != bits(asc[live])).sum())
        print("width %d: %d of %d finished entries differ between the kernel's tree and an ascending sum" % (x.shape[2], differ, len(live)))
        assert differ > len(live) // 2
        zero = [i for i in range(16) if 2 in (i >> 2, i & 3)]
        assert (bits(e[zero]) == 0).all()
        # symmetric 16-entry form
        for net in range(3):
            m = e[net * 16:net * 16 + 16].reshape(4, 4)
            np.testing.assert_array_equal(bits(m), bits(m.T))
