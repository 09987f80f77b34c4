"""CPU: the SOURCE of the large-minibatch trunk products (seqdex_amd/csrc/sdx_gemm_nt.h: k_gemm_nt, k_stage) executed on the SIMT
emulator (tests/hipemu: MFMA as a wave collective with the ISA's lane layouts, global_load_lds as the lane-linear copy it is) against
numpy: source-side swizzle vs fragment reads, accumulator layout, the three epilogues incl. the transposed copies and the ones-MFMA
row sums, split reductions, ragged edges, both element types.  What the emulator cannot show - bank conflicts, timing - is measured on
the GPU (profiles/r4_bigmb_*).  The cases and what they assert live in tests/gemm_nt_cases.py: tests/test_gpu_gemm_products.py runs the
same ones on the COMPILED kernels (where the emulator build's replacements under #ifdef HIPEMU - the v_dot2c row sums, global_load_lds -
are the real instructions), and the GPU parity tests (tests/test_gpu_ppo_parity.py::test_large_minibatch_*,
tests/test_gpu_ppo_branches.py) hold the assembled step to the autograd oracle on every path."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gemm_nt_cases as GC  # noqa: E402
from gemm_nt_cases import EPI_FWD, EPI_TN, elems as _elems, from_elems as _from_elems  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"), reason="needs ROCm's clang++ for the host build")


@pytest.fixture(scope="module")
def lib():
    from tests import hipemu
    l = C.CDLL(hipemu.build_gemm())
    vp, i, fp = C.c_void_p, C.c_int, C.c_void_p
    l.emu_gemm_nt.argtypes = [i, i, vp, i, vp, i, i, i, i, i, i, fp, i, C.c_longlong, vp, i, vp, i, fp, vp, i, vp, i, fp]
    l.emu_gemm_nt_narrow.argtypes = [i, vp, i, vp, i, i, i, i, fp, i, vp, i, fp]
    l.emu_stage.argtypes = [i, fp, i, i, i, i, vp, i, vp, i]
    l.emu_gemm_nt_wide.argtypes = [i, i, vp, i, vp, i, i, i, i, fp, i, vp, i, vp, i, fp, vp, i, vp, i]
    l.emu_gemm_tt.argtypes = [vp, i, vp, i, i, i, i, i, i, fp, i, C.c_longlong, vp, i]
    return l


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Emulated:
    """backend of gemm_nt_cases: one product per launch through the entry points of tests/hipemu/gemm_driver.cpp.  tile 0: the launcher
    (emu_gemm_nt); a forced tile of k_gemm_nt has an entry of its own (emu_gemm_nt_narrow: forward, no element copy;
    emu_gemm_nt_wide: forward / data gradient)"""

    def __init__(self, lib):
        self.lib = lib

    def nt(self, bf, epi, tile, splits, problems):
        (g,) = problems
        rowsum = None if g.rowsum_off is None else C.c_void_p(g.Cf.ctypes.data + 4 * g.rowsum_off)
        if tile == 0:
            self.lib.emu_gemm_nt(bf, epi, _p(g.A), g.lda, _p(g.B), g.ldb, g.M, g.N, g.K, g.kchunk, splits, _p(g.Cf), g.ldc, g.cz, _p(g.Cn), g.ldn,
                                 _p(g.Ct), g.ldt, _p(g.bias), _p(g.H), g.ldh, _p(g.Ht), g.ldht, rowsum)
        elif tile == 1:
            assert epi == EPI_FWD and splits == 1 and g.Cn is None and g.kchunk == g.K
            self.lib.emu_gemm_nt_narrow(bf, _p(g.A), g.lda, _p(g.B), g.ldb, g.M, g.N, g.K, _p(g.Cf), g.ldc, _p(g.Ct), g.ldt, _p(g.bias))
        else:
            assert epi != EPI_TN and splits == 1 and g.kchunk == g.K
            self.lib.emu_gemm_nt_wide(bf, epi, _p(g.A), g.lda, _p(g.B), g.ldb, g.M, g.N, g.K, _p(g.Cf), g.ldc, _p(g.Cn), g.ldn, _p(g.Ct), g.ldt,
                                      _p(g.bias), _p(g.H), g.ldh, _p(g.Ht), g.ldht)

    def tt(self, tile, splits, problems):
        (g,) = problems
        self.lib.emu_gemm_tt(_p(g.A), g.lda, _p(g.B), g.ldb, g.M, g.N, g.K, g.kchunk, splits, _p(g.Cf), g.ldc, g.cz,
                             C.c_void_p(g.Cf.ctypes.data + 4 * g.rowsum_off), tile)


@pytest.fixture(scope="module")
def emu(lib):
    return Emulated(lib)


@pytest.mark.parametrize("bf", GC.BF)
@pytest.mark.parametrize("M,N,K", GC.FORWARD_SHAPES)
def test_forward_product_all_outputs(emu, bf, M, N, K):
    GC.forward_product_all_outputs(emu, bf, M, N, K)


@pytest.mark.parametrize("bf", GC.BF)
def test_narrow_tile_shape(emu, bf):
    GC.narrow_tile_shape(emu, bf)


@pytest.mark.parametrize("bf", GC.BF)
@pytest.mark.parametrize("epi", GC.WIDE_EPIS)
@pytest.mark.parametrize("M", GC.WIDE_M)
def test_wide_tile_shape_all_copies(emu, bf, epi, M):
    GC.wide_tile_shape_all_copies(emu, bf, epi, M)


@pytest.mark.parametrize("bf", GC.BF)
def test_data_gradient_product(emu, bf):
    GC.data_gradient_product(emu, bf)


@pytest.mark.parametrize("bf", GC.BF)
@pytest.mark.parametrize("splits", GC.SPLITS)
def test_weight_gradient_product_with_row_sums(emu, bf, splits):
    GC.weight_gradient_product_with_row_sums(emu, bf, splits)


@pytest.mark.parametrize("bf", [0, 1])
def test_stage_kernel(lib, bf):
    rng = np.random.default_rng(3)
    R, K, lds = 150, 100, 104
    KC = 64 if bf else 32
    Kp = (K + KC - 1) // KC * KC
    src = rng.standard_normal((R, lds)).astype(np.float32)
    ldt = 200
    dn = np.full((R, Kp), 77, np.int16 if bf else np.float32)
    dt = np.zeros((Kp, ldt), np.int16 if bf else np.float32)
    lib.emu_stage(bf, _p(src), lds, R, K, Kp, _p(dn), Kp, _p(dt), ldt)
    _, want = _elems(src[:, :K], bf)
    n, t = _from_elems(dn, bf), _from_elems(dt, bf)
    np.testing.assert_array_equal(n[:, :K], want)
    assert not n[:, K:].any()
    np.testing.assert_array_equal(t[:K, :R], want.T)
    assert not t[K:].any() and not t[:, R:].any()


@pytest.mark.parametrize("tile", [1, 2, 0])
@pytest.mark.parametrize("R,Nl,Kl,ldb,splits", GC.TT_SHAPES)
def test_weight_gradient_from_row_major_operands(emu, tile, R, Nl, Kl, ldb, splits):
    GC.weight_gradient_from_row_major_operands(emu, tile, R, Nl, Kl, ldb, splits)
