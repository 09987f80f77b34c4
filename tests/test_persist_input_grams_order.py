"""The inputs of tests/test_gpu_persist_input_grams.py can tell the summation order of the persistent update's input Grams from another one:
on the host, the numpy restatement of the kernels' order (helpers/input_gram_cases.py) and a plain ascending float32 sum differ in the bits of
more than half of the entries, for every width the GPU test uses, and both stay within the GPU test's bound of the float64 value."""
import numpy as np
import pytest

from helpers.input_gram_cases import MB, N_MB, NEG_COL, ZERO_ROW, bits, gram_ascending, gram_float64, gram_kernel_order, rows


@pytest.mark.parametrize("width", [396, 188, 564])
def test_generator_separates_the_kernel_order_from_an_ascending_sum(width):
    x = rows(width, width)
    ko, asc = gram_kernel_order(x), gram_ascending(x)
    differ = int((bits(ko) != bits(asc)).sum())
    print("width %d: %d of %d entries differ in bits between the kernels' order and an ascending sum" % (width, differ, ko.size))
    assert differ > ko.size // 2
    exact, mag = gram_float64(x)
    for got in (ko, asc):          # (an ascending sum of up to 564 terms needs more than the 40 roundings of the kernels' tree: its own bound)
        assert (np.abs(got - exact) <= (40 if got is ko else 600) * 2.0 ** -24 * mag).all()
    # the special rows are there: the zero row's entries are +0.0 in both orders, the negative column is negative in all four rows
    z = [i for i in range(16) if ZERO_ROW[1] in (i >> 2, i & 3)]
    assert (bits(ko[ZERO_ROW[0]][z]) == 0).all() and (bits(asc[ZERO_ROW[0]][z]) == 0).all()
    assert (x[MB * NEG_COL[0]:MB * NEG_COL[0] + MB, NEG_COL[1]] < 0).all() and x.shape == (MB * N_MB, width)
