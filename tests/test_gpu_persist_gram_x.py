"""-m gpu: the Grams of x2 and x1 of the persistent update, as the epoch kernel forms them in the shadow of its x3 edge (csrc/sdxp_persist.hip),
held to a host restatement BIT FOR BIT - per thread and finished.  The Grams enter the squared gradient norm (<G_dY1, G_x1>, <G_dY2, G_x2>),
hence the clip scale and every parameter; the Gram of x1 sums two columns per thread, and which of a diagonal entry's two squares is contracted
into the fma once moved with code elsewhere in the kernel (the opaque copy in that block keeps the first rounded).  The block runs verbatim in
the test entry sdxpk_gram_x_check (csrc/sdxp_persist_checks.hip, built with the epoch kernel's flags) on row_butterfly, rows_store and
rows_reduce of csrc/sdxp_persist_sums.h: a change to any of them that moves a bit of a Gram fails here.

(a) the block against the host restatement (helpers/gram_x_cases.py), bit for bit: every thread's 2 x 30 terms in front of the butterfly and
    the 2 x 48 finished entries.  The inputs have 13 significant bits, so the float64 restatement of the fma is exact
    (tests/test_persist_gram_x_order.py).  The finished entries alone could hardly tell the diagonal's two contractions apart (they differ in a
    few entries only); the per-thread terms do, in more than 10 % of the diagonal terms - asserted here on the host as a condition on the
    inputs.
(b) two persistent handles from one state at 16 actors x horizon 8 (160 optimiser steps): parameters, Adam moments and the rewritten
    mu / sigma rows bit-identical - nothing may depend on timing."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from helpers.gram_x_cases import DIAG, NTH, entries, inputs, terms, terms_other_contraction  # noqa: E402
from helpers.input_gram_cases import MB, bits  # noqa: E402
from helpers.persist_float64 import persistent_or_skip  # noqa: E402
from test_gpu_fullsize_properties import _filled_agent  # noqa: E402

_cache = {}


def _device():
    """(x1, x2, terms [gram][30][NTH], entries [gram][48]) of sdxpk_gram_x_check; gram 0 = x2, 1 = x1.  Computed once."""
    if not _cache:
        from seqdex_amd import _abi
        from seqdex_amd.sim import _stream_ptr
        lib, dev = _abi.load_library(), torch.device("cuda:0")
        vp = C.c_void_p
        lib.sdxpk_gram_x_check.restype = C.c_int
        lib.sdxpk_gram_x_check.argtypes = [vp, vp, vp, vp, vp]
        x1, x2 = inputs()
        d1, d2 = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)
        t = torch.full((2, 30, NTH), float("nan"), device=dev)
        e = torch.full((2, 48), float("nan"), device=dev)
        assert lib.sdxpk_gram_x_check(d1.data_ptr(), d2.data_ptr(), t.data_ptr(), e.data_ptr(), _stream_ptr(dev)) == 0
        torch.cuda.synchronize()
        _cache["v"] = (x1, x2, t.cpu().numpy(), e.cpu().numpy())
    return _cache["v"]


def _same(name, got, want):
    bad = np.argwhere(bits(got) != bits(want))
    print("%s: %d of %d differ in bits" % (name, len(bad), got.size))
    assert len(bad) == 0, "%s: first at %r: %r against %r" % (name, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def test_shadow_block_equals_the_host_restatement_bit_for_bit():
    x1, x2, t, e = _device()
    assert np.isfinite(t).all() and np.isfinite(e).all()
    other = terms_other_contraction(x1)
    want1 = terms(x1)
    d = float((bits(want1[DIAG]) != bits(other[DIAG])).mean())
    print("inputs: %.1f %% of the diagonal terms of G_x1 differ under the other contraction" % (100 * d))
    assert d >= 0.10
    for gram, name, x in ((0, "x2", x2), (1, "x1", x1)):
        want = terms(x)
        _same("terms of G_%s, x3 shadow's block against the host" % name, t[gram], want)
        _same("entries of G_%s, x3 shadow's block against the host" % name, e[gram], entries(want))


def test_two_persistent_handles_end_bit_identical():
    n = 16
    a, b = _filled_agent(n, 9), _filled_agent(n, 9)
    try:
        persistent_or_skip(a)
        assert b.update_impl() == "persistent"
        p0 = a.t["AC_PARAMS"].clone()
        a.update(); b.update()
        torch.cuda.synchronize()
        assert a.update_impl() == "persistent" and a.ctrl().ac_t == b.ctrl().ac_t == 5 * (n * 8 // MB) == 160
        for k in ("AC_PARAMS", "CV_PARAMS", "AC_ADAM_M", "AC_ADAM_V", "CV_ADAM_M", "CV_ADAM_V", "MB_MUS", "MB_SIGMAS"):
            np.testing.assert_array_equal(a.t[k].cpu().numpy().view(np.int32), b.t[k].cpu().numpy().view(np.int32), err_msg=k)
        assert float((a.t["AC_PARAMS"] - p0).abs().max()) > 1e-4              # the epoch did something
    finally:
        a.close(); b.close()
